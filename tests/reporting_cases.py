"""Sentinel inputs for the reductions that report on a solve (the two energies, the max update norm and its arg-max) and plain
numpy restatements of what the reference's reductions return on them (src/sobfu/cuda/reductor.cu, src/sobfu/reductor.cpp:38-94,
src/sobfu/precomp.cpp:20-43).

A sentinel input is zero except at a few cells.  The cells sit where a tree reduction goes wrong: the first and the last cell,
block and grid-stride trip boundaries, the tail of a partial block.  Arrays start as np.zeros (calloc'd: pages that are only read
cost no memory), so even 2**26 + 1 cells of float4 stay cheap on the host."""
import numpy as np

SIZES = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 26, 2 ** 26 + 1]
BIG = 2 ** 20  # above this, cases that need a dense non-zero array are left out


def next_pow2(x):
    return 1 << max(0, int(x - 1).bit_length())


def reduce_config(n):
    """get_num_blocks_and_threads(n, 65536, 512) -- precomp.cpp:20-43"""
    t = next_pow2((n + 1) // 2) if n < 1024 else 512
    return min((n + 2 * t - 1) // (2 * t), 65536), t


def sentinel_cells(n):
    """first / last cell, both halves of the first and the last block, block and trip boundaries, the partial block's tail"""
    b, t = reduce_config(n)
    grid = 2 * t * b
    last_block = ((n - 1) // (2 * t)) * (2 * t)
    cand = [0, n - 1, t - 1, t, 2 * t - 1, 2 * t, 2 * t * 3 + 5, 2 * 512 * 7, 2 * 512 * 7 + 512, grid - 1, grid, grid + 1, 2 ** 24 - 1,
            2 ** 24, 2 ** 24 + 1, 2 ** 26, 2 ** 26 + 1, last_block, last_block + t, (n - 1 + last_block) // 2]
    return sorted({c for c in cand if 0 <= c < n})


def sum_sentinels(n):
    """{cell: v}: v = +-2**(k mod 10), so every v*v is a power of two <= 2**18 and, with at most 20 cells, every partial sum is an
    integer below 2**24: the fp32 tree sum is exact in any order, and a dropped or doubled cell changes it"""
    cells = sentinel_cells(n)
    assert len(cells) <= 20
    return {c: np.float32((-1.0) ** k * 2.0 ** (k % 10)) for k, c in enumerate(cells)}


def data_inputs(n, sent):
    """phi_global, phi_n (n x 2): the sentinel in phi_global.x or (negated) in phi_n.x, junk in the weight channel"""
    g, f = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    for k, (c, v) in enumerate(sent.items()):
        (g if k % 2 == 0 else f)[c, 0] = v if k % 2 == 0 else -v
        g[c, 1], f[c, 1] = 1e30, -7.0  # weights: not part of the data term
    return g, f


def jacobian_inputs(n, sent):
    """J (n x 4 x 4): the sentinel in one of the nine x / y / z entries of rows 0 - 2, junk in the w column and row 3"""
    J = np.zeros((n, 4, 4), np.float32)
    for k, (c, v) in enumerate(sent.items()):
        J[c, k % 3, (k // 3) % 3] = v
        J[c, :, 3] = 1e30
        J[c, 3, :] = 3e30
    return J


def exact_energy(sent):
    """0.5 * sum v*v in float64 (exact for sum_sentinels)"""
    return 0.5 * float(sum(np.float64(v) ** 2 for v in sent.values()))


def sum_bound(terms64):
    """|fp32 sum - exact| <= gamma_n * sum |terms| (any summation order, n terms; Higham 2002, eq. 4.4) + the result's own rounding"""
    n = max(1, len(terms64))
    u = 2.0 ** -24
    return n * u / (1 - n * u) * float(np.abs(terms64).sum())


# ---- max update norm ------------------------------------------------------------------------------------------------------
def norm_rd(u):
    """norm(u) of utils.hpp:279-283 in fp32: (x*x + y*y) + z*z, no contraction, sqrt rounded toward -inf"""
    u = np.asarray(u, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]
        r = np.sqrt(s, dtype=np.float32)
        down = (r > 0) & np.isfinite(r) & (r.astype(np.float64) ** 2 > s.astype(np.float64))
    return np.where(down, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float32)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def scan_key(i, n):
    """The reference keeps the first of equal maxima in the order in which reduce_max_kernel meets them (strict '>' everywhere):
    blocks in index order (final_reduce_max), then the threads of a block in the order of the stride-halving tree -- at level h slot
    t keeps its own value against slot t + h on a tie, so the tree prefers an even thread to an odd one, then bit 1 clear to bit 1
    set, ...: threads in BIT-REVERSED index order (not the lowest index) -- then the cells of a thread in its sequence.
    Returns (block, bit-reversed thread, position in the thread's sequence)."""
    b, t = reduce_config(n)
    grid = 2 * t * b
    tid = (i % (2 * t)) % t
    return ((i % grid) // (2 * t), bitrev(tid, t.bit_length() - 1), 2 * (i // grid) + ((i % (2 * t)) >= t))


def index_value(i, n):
    """the float-encoded index the reference stores: (float) i, or (float) base + threads for the upper half (reductor.cu:371)"""
    _, t = reduce_config(n)
    if (i % (2 * t)) >= t:
        return float(np.float32(np.float32(i - t) + np.float32(t)))
    return float(np.float32(i))


def expected_max(cells, n):
    """(max norm, index) of Reductor::max_update_norm for an updates array that is zero except at cells = {i: float4}"""
    best = None
    for i, u in cells.items():
        v = float(norm_rd(np.asarray(u, np.float32)))
        if not v > 0.0:  # NaN and 0 never beat the running maximum, which starts at 0
            continue
        if best is None or v > best[0] or (v == best[0] and scan_key(i, n) < scan_key(best[1], n)):
            best = (v, i)
    return (0.0, 0.0) if best is None else (best[0], index_value(best[1], n))


def max_cases(n):
    """[(name, {cell: float4})] of the max-norm sentinels"""
    b, t = reduce_config(n)
    grid = 2 * t * b
    cells = sentinel_cells(n)
    out = [("zero", {})]
    out.append(("distinct", {c: (np.float32(k + 1), np.float32(-0.5 * k), np.float32(0.25), 0) for k, c in enumerate(cells)}))
    big = (np.float32(3), np.float32(-4), np.float32(12), 0)  # 13 exactly
    small = (np.float32(1), np.float32(2), np.float32(2), 0)  # 3
    base = {c: small for c in cells}

    def tie(name, *at):
        at = [a for a in at if 0 <= a < n]
        if len(at) >= 2:
            d = dict(base)
            d.update({a: big for a in at})
            out.append((name, d))

    tie("tie within a thread", t - 1 + t, t - 1 + grid, t - 1)  # positions 1, 2, 0 of thread t-1 (block 0)
    tie("tie across lanes", t + 0, 1)  # thread 0's second cell beats thread 1's first
    tie("tie across lanes, odd", t + 3, 2)  # thread 2 beats thread 3 (the tree pairs 2 with 3 last but one)
    tie("tie across waves", t + 3, 69)  # thread 69 (bit-reversed 324 of 512) beats thread 3 (384)
    tie("tie across waves, even", t + 64, 3)  # thread 64 beats thread 3
    tie("tie across blocks", 2 * t * (b - 1), 2 * t + t - 1)
    tie("tie across trips", grid, 2 * t + 5)  # block 0 on the second trip beats block 1 on the first
    tie("tie last cell", n - 1, n - 2)
    nan = dict(base)
    for k, c in enumerate(cells):
        if k % 2 == 0:
            nan[c] = (np.float32(np.nan), np.float32(1), np.float32(0), 0) if k % 4 == 0 else (np.float32(0), np.float32(0), np.float32(-np.nan), 0)
    out.append(("NaN cells ignored", nan))
    inf = dict(base)
    inf.update({cells[-1]: (np.float32(0), np.float32(np.inf), np.float32(0), 0), cells[0]: (np.float32(-np.inf), np.float32(1), np.float32(1), 0)})
    out.append(("+inf wins, first in scan order", inf))
    out.append(("overflow to inf", {cells[-1]: (np.float32(3e19), np.float32(0), np.float32(0), 0), cells[0]: small}))
    out.append(("-0 components", {c: (np.float32(-0.0), np.float32(-0.0), np.float32(-0.0), np.float32(-0.0)) for c in cells}
                | ({cells[-1]: (np.float32(-3), np.float32(-0.0), np.float32(-4), 0)} if len(cells) > 1 else {})))
    return out


def updates_array(n, cells, fill=None):
    """n x 4 float32, zero (or `fill` everywhere) except at cells"""
    u = np.zeros((n, 4), np.float32) if fill is None else np.full((n, 4), fill, np.float32)
    for i, v in cells.items():
        u[i] = v
    return u
