"""numpy restatement of the warp-field diagnostics (sobfu_amd/csrc/sobfu_warp_stats.hpp): float32 operation by operation
for det J, the lengths and the sampler (fma / tri_setup are tests/render_reference.py's: its fma is an exact fmaf), Python integers for
the exact sums and the keys.  Also the fields, masks and cases shared by tests/test_warp_stats_cpu.py and tests/test_gpu_warp_stats.py.

Arrays are indexed [z, y, x]: psi and psi^-1 (Z, Y, X, 4) float32, masks (Z, Y, X, 2) {tsdf, weight}."""
from __future__ import annotations

import numpy as np

import render_reference as RR

F = np.float32
WORDS = 64
(N_DET, N_FOLD, N_DET_NONFINITE, N_DISP, N_DISP_NONFINITE, N_RES, N_RES_ABOVE, N_RES_OUTSIDE, N_RES_NONFINITE) = range(9)
DET_BELOW, DET_SUM_HI, DET_SUM_LO, DISP_SUM_HI, DISP_SUM_LO, RES_SUM_HI, RES_SUM_LO = 9, 25, 26, 27, 28, 29, 30
DET_MIN_KEY, DET_MAX_KEY, DISP_MAX_KEY, RES_MAX_KEY = 31, 32, 33, 34
EMPTY_KEY = (1 << 64) - 1
QNAN = np.array([0x7FC00000], np.uint32).view(F)[0]
MIN_CHUNK, TILE_X, TILE_Y, WORKGROUPS = 4, 64, 4, 1024  # ws_launch's constants


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def identity(dims):
    X, Y, Z = dims
    psi = np.zeros((Z, Y, X, 4), F)
    psi[..., 0], psi[..., 1], psi[..., 2] = np.arange(X, dtype=F)[None, None, :], np.arange(Y, dtype=F)[None, :, None], np.arange(Z, dtype=F)[:, None, None]
    return psi


def disp(psi):
    """u = psi - id, (Z, Y, X, 3)"""
    Z, Y, X = psi.shape[:3]
    with np.errstate(all="ignore"):
        return (psi[..., :3] - identity((X, Y, Z))[..., :3]).astype(F)


def deriv(u, axis):
    """along numpy axis `axis` of extent n: n == 1 -> 0; one-sided and not halved at both ends; (u(i + 1) - u(i - 1)) / 2 inside"""
    n = u.shape[axis]
    d = np.zeros_like(u)
    if n == 1:
        return d
    u, dm = np.moveaxis(u, axis, 0), np.moveaxis(d, axis, 0)
    with np.errstate(all="ignore"):
        dm[0] = u[1] - u[0]
        dm[n - 1] = u[n - 1] - u[n - 2]
        dm[1:n - 1] = (u[2:] - u[:n - 2]) / F(2)
    return d


def det_volume(psi):
    u = disp(psi)
    dx, dy, dz = deriv(u, 2), deriv(u, 1), deriv(u, 0)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        j00, j01, j02 = one + dx[..., 0], zero + dy[..., 0], zero + dz[..., 0]
        j10, j11, j12 = zero + dx[..., 1], one + dy[..., 1], zero + dz[..., 1]
        j20, j21, j22 = zero + dx[..., 2], zero + dy[..., 2], one + dz[..., 2]
        c00, c01, c02 = j11 * j22 - j12 * j21, j12 * j20 - j10 * j22, j10 * j21 - j11 * j20
        det = (j00 * c00 + j01 * c01) + j02 * c02
    assert det.dtype == F
    return det


def length(a, vs):
    """metres: sqrtf(((a.x vs.x)^2 + (a.y vs.y)^2) + (a.z vs.z)^2)"""
    with np.errstate(all="ignore"):
        sx, sy, sz = a[..., 0] * F(vs[0]), a[..., 1] * F(vs[1]), a[..., 2] * F(vs[2])
        out = np.sqrt((sx * sx + sy * sy) + sz * sz)
    assert out.dtype == F
    return out


def canonical(v):
    return np.where(np.isnan(v), QNAN, v).astype(F)


def in_mask(mask, band):
    with np.errstate(invalid="ignore"):
        return (mask[..., 1] > 0) & (np.abs(mask[..., 0]) < F(band))


def interp_disp(psi, px, py, pz):
    """sobfu_device.hpp's interp_disp at n points (finite, inside): the lerp chain z, then y, then x; lerp1(upper, lower, t)"""
    Z, Y, X = psi.shape[:3]
    ag, ah, tx = RR.tri_setup(px, X)
    bg, bh, ty = RR.tri_setup(py, Y)
    cg, ch, tz = RR.tri_setup(pz, Z)

    def corner(a, b, c):
        with np.errstate(all="ignore"):
            return (psi[c, b, a, :3] - np.stack([a.astype(F), b.astype(F), c.astype(F)], -1)).astype(F)

    def lerp(u, v, t):
        return RR.lerp1(u, v, t[:, None])

    return lerp(lerp(lerp(corner(ah, bh, ch), corner(ah, bh, cg), tz), lerp(corner(ah, bg, ch), corner(ah, bg, cg), tz), ty),
                lerp(lerp(corner(ag, bh, ch), corner(ag, bh, cg), tz), lerp(corner(ag, bg, ch), corner(ag, bg, cg), tz), ty), tx)


def residual_volume(psi, psi_inv, voxel_size):
    """-> (|e| per voxel with NaN where p is outside or non-finite, class per voxel: 0 counted, 1 non-finite, 2 outside)"""
    Z, Y, X = psi.shape[:3]
    p = psi_inv[..., :3].reshape(-1, 3)
    idn = identity((X, Y, Z))[..., :3].reshape(-1, 3)
    cls = np.zeros(len(p), np.int64)
    finite = np.isfinite(p).all(1)
    top = np.array([X - 1, Y - 1, Z - 1], F)
    with np.errstate(invalid="ignore"):
        outside = ((p < 0) | (p > top)).any(1)
    cls[~finite] = 1
    cls[finite & outside] = 2
    ok = cls == 0
    res = np.full(len(p), QNAN, F)
    if ok.any():
        q = p[ok]
        u = interp_disp(psi, q[:, 0], q[:, 1], q[:, 2])
        with np.errstate(all="ignore"):
            e = ((q + u) - idn[ok]).astype(F)
        ln = canonical(length(e, voxel_size))
        res[ok] = ln
        bad = np.flatnonzero(ok)[~np.isfinite(ln)]
        cls[bad] = 1
    return res.reshape(Z, Y, X), cls.reshape(Z, Y, X)


def fx44(v):
    """llrint(clamp((double) v, -1024, 1024) 2^44) of finite float32 values, as int64"""
    return np.rint(np.clip(np.asarray(v, F).astype(np.float64), -1024.0, 1024.0) * 2.0 ** 44).astype(np.int64)


def sum_words(v):
    """(sum(q >> 24), sum(q & 0xffffff)) as Python integers (|q >> 24| <= 2^30 and fewer than 2^31 terms: the int64 sums are exact)"""
    q = fx44(v)
    return int((q >> 24).sum(dtype=np.int64)), int((q & 0xFFFFFF).sum(dtype=np.int64))


def ordered(v):
    b = (np.asarray(v, F) + F(0)).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def min_key(v, index):
    if v.size == 0:
        return EMPTY_KEY
    return int(((ordered(v).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)).min())


def max_key(v, index):
    if v.size == 0:
        return EMPTY_KEY
    return int((((~ordered(v)).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)).min())


def warp_stats(psi, psi_inv=None, mask_det=None, mask_res=None, voxel_size=(1.0, 1.0, 1.0), band=1.0, edges=(), res_tol=0.0):
    """-> dict(words: (64,) uint64, det: (Z, Y, X) float32, res: (Z, Y, X) float32 or None)"""
    Z, Y, X = psi.shape[:3]
    assert psi.dtype == F and X * Y * Z <= 2 ** 31 and 0 <= len(edges) <= 16
    w = [0] * WORDS
    index = np.arange(X * Y * Z, dtype=np.uint64)
    det = det_volume(psi).reshape(-1)
    sel = np.ones(det.shape, bool) if mask_det is None else in_mask(mask_det, band).reshape(-1)
    fin = sel & np.isfinite(det)
    d = det[fin]
    w[N_DET], w[N_DET_NONFINITE] = int(fin.sum()), int((sel & ~np.isfinite(det)).sum())
    w[N_FOLD] = int((d <= 0).sum())
    for k, e in enumerate(edges):
        w[DET_BELOW + k] = int((d < F(e)).sum())
    w[DET_SUM_HI], w[DET_SUM_LO] = sum_words(d)
    w[DET_MIN_KEY], w[DET_MAX_KEY] = min_key(d, index[fin]), max_key(d, index[fin])

    ln = length(disp(psi), voxel_size).reshape(-1)
    fin = sel & np.isfinite(ln)
    w[N_DISP], w[N_DISP_NONFINITE] = int(fin.sum()), int((sel & ~np.isfinite(ln)).sum())
    w[DISP_SUM_HI], w[DISP_SUM_LO] = sum_words(ln[fin])
    w[DISP_MAX_KEY] = max_key(ln[fin], index[fin])

    res = None
    w[RES_MAX_KEY] = EMPTY_KEY
    if psi_inv is not None:
        res, cls = residual_volume(psi, psi_inv, voxel_size)
        r, cls = res.reshape(-1), cls.reshape(-1)
        sel = np.ones(r.shape, bool) if mask_res is None else in_mask(mask_res, band).reshape(-1)
        okm = sel & (cls == 0)
        w[N_RES], w[N_RES_NONFINITE], w[N_RES_OUTSIDE] = int(okm.sum()), int((sel & (cls == 1)).sum()), int((sel & (cls == 2)).sum())
        w[N_RES_ABOVE] = int((r[okm] > F(res_tol)).sum())
        w[RES_SUM_HI], w[RES_SUM_LO] = sum_words(r[okm])
        w[RES_MAX_KEY] = max_key(r[okm], index[okm])
    words = np.array([v & EMPTY_KEY for v in w], dtype=np.uint64)
    return dict(words=words, det=canonical(det).reshape(Z, Y, X), res=res)


# ---- decoding the words ----------------------------------------------------------------------------------------------------------------
def signed(word):
    word = int(word)
    return word - (1 << 64) if word >> 63 else word


def exact_sum(hi, lo):
    """the sum of the quantised terms times 2^44, a Python integer"""
    return signed(hi) * (1 << 24) + signed(lo)


def decode_key(key, maximum, dims):
    """-> (float32 value, (x, y, z)); an empty group: (NaN, (-1, -1, -1))"""
    key = int(key)
    o, index = key >> 32, key & 0xFFFFFFFF
    if key == EMPTY_KEY:
        return F(np.nan), (-1, -1, -1)
    if maximum:
        o = ~o & 0xFFFFFFFF
    b = o ^ 0x80000000 if o & 0x80000000 else ~o & 0xFFFFFFFF
    X, Y, _ = dims
    return np.array([b], np.uint32).view(F)[0], (index % X, (index // X) % Y, index // (X * Y))


def launch(dims):
    """ws_launch: (tiles along x, tiles along y, chunks along z, planes per chunk)"""
    X, Y, Z = dims
    gx, gy = (X + TILE_X - 1) // TILE_X, (Y + TILE_Y - 1) // TILE_Y
    want = max(WORKGROUPS // (gx * gy), 1)
    zc = max((Z + want - 1) // want, MIN_CHUNK)
    return gx, gy, (Z + zc - 1) // zc, zc


# ---- fields and masks ------------------------------------------------------------------------------------------------------------------
def affine(dims, A, b):
    """psi = A x + b (float64 arithmetic, rounded once)"""
    idn = identity(dims)[..., :3].astype(np.float64)
    psi = np.zeros(idn.shape[:3] + (4,), F)
    psi[..., :3] = (idn @ np.asarray(A, np.float64).T + np.asarray(b, np.float64)).astype(F)
    return psi


def reflection(dims):
    """x -> (X - 1) - x: det J = -1 at every voxel"""
    return affine(dims, np.diag([-1.0, 1.0, 1.0]), [dims[0] - 1.0, 0.0, 0.0])


def smooth_random(dims, seed, amplitude=0.6):
    """identity plus a few low-frequency waves of `amplitude` voxels, on a dyadic grid of 2^-10 so that equal values are exactly equal"""
    rng = np.random.default_rng(seed)
    idn = identity(dims)
    x, y, z = (idn[..., k].astype(np.float64) for k in range(3))
    u = np.zeros(idn.shape[:3] + (3,))
    for k in range(3):
        for _ in range(3):
            f, ph = rng.uniform(0.05, 0.35, 3), rng.uniform(0, 2 * np.pi)
            u[..., k] += amplitude / 3.0 * np.sin(f[0] * x + f[1] * y + f[2] * z + ph)
    psi = idn.copy()
    psi[..., :3] += (np.round(u * 1024.0) / 1024.0).astype(F)
    return psi


def plant_fold(psi, at, back=3.0):
    """the voxel `at` = (x, y, z) pushed `back` cells along -x"""
    x, y, z = at
    psi[z, y, x, 0] -= F(back)
    return psi


def planted(dims, seed):
    """smooth_random with, on grids of at least 16 x 5 x 5, two sites whose 5 x 3 x 3 neighbourhood is the identity and whose centre is pushed
    3 cells back: det = -0.5 exactly at the voxel before each (two equal minima: the lower index wins).  -> (psi, the two folded voxels)"""
    X, Y, Z = dims
    psi, idn, sites = smooth_random(dims, seed), identity(dims), []
    if X >= 16 and Y >= 5 and Z >= 5:
        for x in (5, X - 6):
            y, z = Y // 2, Z // 2
            psi[z - 1:z + 2, y - 1:y + 2, x - 2:x + 3] = idn[z - 1:z + 2, y - 1:y + 2, x - 2:x + 3]
            plant_fold(psi, (x, y, z))
            sites.append((x - 1, y, z))
    return psi, sites


def sphere_mask(dims, band, seed=0):
    """a sphere TSDF (units of the truncation distance, 4 voxels) with a fifth of the weights 0 and, inside the band, some |tsdf| set
    to exactly `band` (excluded: the test is <)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    idn = identity(dims)[..., :3].astype(np.float64)
    r = np.sqrt(((idn - np.array([(X - 1) / 2.0, (Y - 1) / 2.0, (Z - 1) / 2.0])) ** 2).sum(-1))
    m = np.zeros((Z, Y, X, 2), F)
    m[..., 0] = np.clip((r - 0.35 * min(X, Y, Z)) / 4.0, -1.0, 1.0).astype(F)
    m[..., 1] = (rng.random((Z, Y, X)) > 0.2).astype(F) * F(3)
    flat = m.reshape(-1, 2)
    inside = np.flatnonzero(np.abs(flat[:, 0]) < F(band))
    for k, i in enumerate(inside[::7]):
        flat[i, 0] = F(band) if k % 2 else -F(band)
    return m


def naive_inverse(psi):
    """x - u(x): the first sweep's estimate, a non-zero residual"""
    Z, Y, X = psi.shape[:3]
    out = np.zeros_like(psi)
    out[..., :3] = identity((X, Y, Z))[..., :3] - disp(psi)
    return out


EDGES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)
EDGES16 = tuple(float(v) for v in np.linspace(-1.0, 2.75, 16))


def cases():
    """(name, kwargs of warp_stats) on grids small enough for the CPU tool: every path of the rules"""
    out = []
    for dims in ((1, 1, 1), (2, 3, 4), (5, 1, 7), (1, 6, 3), (9, 8, 7)):
        out.append(("identity %s" % (dims,), dict(psi=identity(dims), psi_inv=identity(dims), edges=EDGES)))
    dims = (11, 9, 10)
    A = np.array([[1.1, 0.2, -0.1], [0.05, 0.9, 0.15], [-0.2, 0.1, 1.2]])
    out.append(("affine", dict(psi=affine(dims, A, [0.5, -0.25, 1.0]), edges=EDGES, voxel_size=(0.01, 0.02, 0.03))))
    out.append(("reflection", dict(psi=reflection(dims), psi_inv=reflection(dims), edges=EDGES)))
    psi = smooth_random(dims, 1)
    plant_fold(psi, (5, 4, 5))
    mask = sphere_mask(dims, 0.75)
    out.append(("random, no mask", dict(psi=psi, psi_inv=naive_inverse(psi), edges=EDGES16, res_tol=0.001, voxel_size=(0.004, 0.004, 0.004))))
    out.append(("random, masks", dict(psi=psi, psi_inv=naive_inverse(psi), mask_det=mask, mask_res=sphere_mask(dims, 0.75, 1), band=0.75, edges=EDGES,
                                      res_tol=0.0005, voxel_size=(0.004, 0.005, 0.006))))
    out.append(("random, det mask only", dict(psi=psi, mask_det=mask, band=0.75, edges=(1.0,))))
    empty = mask.copy()
    empty[..., 1] = 0
    out.append(("empty masks", dict(psi=psi, psi_inv=naive_inverse(psi), mask_det=empty, mask_res=empty, edges=EDGES)))
    bad = psi.copy()
    bad[3, 3, 3, 1], bad[6, 2, 8, 0], bad[0, 0, 0, 2] = np.nan, np.inf, -np.inf
    inv = naive_inverse(psi)
    inv[2, 2, 2, 0], inv[4, 4, 4, 2], inv[5, 5, 5, 1], inv[1, 1, 1, 0], inv[7, 7, 7, 2] = np.nan, np.inf, -0.5, dims[0] - 0.5, 1e30
    out.append(("non-finite and outside", dict(psi=bad, psi_inv=inv, edges=EDGES, res_tol=0.01)))
    big = affine(dims, np.eye(3) * 3000.0, [0, 0, 0])  # |u| and det beyond the sums' clamp
    out.append(("beyond the clamp", dict(psi=big, edges=())))
    return out


def same_bits(got, want, what):
    assert np.array_equal(np.asarray(got["words"], np.uint64), want["words"]), "%s: words %s" % (what, np.flatnonzero(np.asarray(got["words"], np.uint64) != want["words"]))
    for k in ("det", "res"):
        if want.get(k) is not None and got.get(k) is not None:
            g, w = np.ascontiguousarray(got[k], F).reshape(-1).view(np.uint32), np.ascontiguousarray(want[k], F).reshape(-1).view(np.uint32)
            assert np.array_equal(g, w), "%s: %s differs at %s" % (what, k, np.flatnonzero(g != w)[:8])
