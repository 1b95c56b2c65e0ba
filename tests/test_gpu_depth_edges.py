"""The depth front end (bilateral, truncate, compute_dists), integrate(depth), the fusion and the TSDF builders at their edges:
image shapes across the 64 x 4 block, pitched rows, volumes across the 64 x 4 x 16 launch geometry, rotated and in-volume cameras,
exact ties, odd fusion tails.

Every GPU result is checked twice: bit for bit against the CPU oracle on identical inputs, and against the float64 statements of
tests/depth_front_reference.py under the thresholds recorded there (tests/test_depth_front_cpu.py shows on the CPU that the oracle
meets the same conditions on the same cases).  Pitched calls go through the C ABI with ctypes; the ops wrappers pass dense images.
"""
import ctypes as C

import numpy as np
import pytest

import depth_front_reference as D

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device; the product path has no CPU fallback")
    from sobfu_amd import ops as _ops

    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def host_u16(t):
    return t.detach().cpu().numpy().view(np.uint16)


def same(a, b):
    """bitwise equality (NaN-safe, distinguishes -0/+0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _abi():
    from sobfu_amd import _lib

    return _lib, _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _f(v):
    return C.c_float(float(v))


# ---------------------------------------------------------------------------------------------------
# bilateral
# ---------------------------------------------------------------------------------------------------
def gpu_bilateral_pitched(src_buf, sstep, dst_buf, dstep, rows, cols, ksz, ss, sd):
    _lib, L, st = _abi()
    s, d = dev_u16(src_buf), dev_u16(dst_buf)
    _lib.check(L.sobfu_hip_bilateral_filter(_p(s), C.c_int(sstep), _p(d), C.c_int(dstep), C.c_int(rows), C.c_int(cols), C.c_int(ksz), _f(ss), _f(sd), st),
               "bilateral")
    return host_u16(s), host_u16(d)


@pytest.mark.parametrize("case", D.BILATERAL_CASES, ids=lambda c: "%dx%d-k%d-%s-sd%g" % (c[0], c[1], c[2], c[5], c[4]))
def test_bilateral(ops, oracle, case):
    rows, cols, ksz, ss, sd, kind = case
    depth = D.depth_image(rows, cols, D.BILATERAL_SEED, kind)
    q64, poisoned, _ = D.bilateral64(depth, ksz, ss, sd)
    band = D.in_band(q64, poisoned)
    # pitched, src and dst: the padding of src is a depth that would wrap the square if it were read; dst's must come back untouched
    src_buf, _, sstep = D.padded(depth, D.U16_PAD, D.U16_SENTINEL)
    dst_o, view_o, dstep = D.padded(np.zeros_like(depth), D.U16_PAD + 4, D.U16_SENTINEL)
    D.oracle_bilateral(oracle, src_buf[:, :cols], view_o, ksz, ss, sd)
    assert np.array_equal(view_o, oracle.bilateral(depth, ksz, ss, sd))  # the oracle itself honours the steps
    dst_g = dst_o.copy()
    dst_g[:, :cols] = 0
    src_back, dst_g = gpu_bilateral_pitched(src_buf, sstep, dst_g, dstep, rows, cols, ksz, ss, sd)
    assert np.array_equal(src_back, src_buf)
    assert np.array_equal(dst_g[:, cols:], dst_o[:, cols:]) and (dst_g[:, cols:] == D.U16_SENTINEL).all()
    out = dst_g[:, :cols]
    # dense, through ops: the same image
    assert np.array_equal(host_u16(ops.bilateral_filter(dev_u16(depth), ksz, ss, sd)), out)
    # against the oracle: libm's and the device's expf differ in the last place, so +-1 -- but only where q sits in the delta band
    diff = np.abs(out.astype(np.int32) - view_o.astype(np.int32))
    print("bilateral %s: %d pixels differ from the oracle, %d in the band, %d poisoned" % (case, (diff != 0).sum(), band.sum(), poisoned.sum()))
    assert diff.max(initial=0) <= 1
    assert not (diff != 0)[~band].any()
    assert np.array_equal(out[poisoned], view_o[poisoned])  # wrapped squares / starved windows: pinned against the oracle alone
    # against float64
    wrong, nband = D.check_bilateral(out, q64, poisoned)
    assert wrong == 0 and nband <= D.BAND_CAP * rows * cols
    if min(rows, cols) == 1:
        assert not out.any()  # empty window: 0 / 0 -> 0


# ---------------------------------------------------------------------------------------------------
# truncate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", D.IMAGE_SHAPES)
@pytest.mark.parametrize("thr_m,max_mm", [(0.7005, 700), (1.4999, 1499), (40.0, 40000)])
def test_truncate(ops, oracle, rows, cols, thr_m, max_mm):
    """max_mm is what the threshold means: whole millimetres, fraction dropped.  A pixel equal to it is kept, one above it is zeroed;
    the comparison is unsigned (40000 and 65535 are large depths, not negative ones)."""
    depth = D.depth_image(rows, cols, 11, "far")
    flat = depth.reshape(-1)
    for i, v in enumerate((max_mm, max_mm + 1, max_mm - 1, 32767, 32768, 65535, 0)):  # the edges, wherever the image has room
        if i < flat.size:
            flat[(i * 7) % flat.size] = v
    want = np.where(depth > max_mm, 0, depth).astype(np.uint16)
    buf, view, step = D.padded(depth, D.U16_PAD, D.U16_SENTINEL)
    buf_o = buf.copy()
    D.oracle_truncate(oracle, buf_o[:, :cols], thr_m)
    _lib, L, st = _abi()
    t = dev_u16(buf)
    _lib.check(L.sobfu_hip_truncate_depth(_p(t), C.c_int(step), C.c_int(rows), C.c_int(cols), _f(thr_m), st), "truncate")
    got = host_u16(t)
    assert np.array_equal(got, buf_o)                                  # the oracle, padding included
    assert (got[:, cols:] == D.U16_SENTINEL).all()                     # a sentinel above every threshold: touched = zeroed
    assert np.array_equal(got[:, :cols], want)                         # the meaning
    dense = dev_u16(depth)
    ops.truncate_depth(dense, thr_m)
    assert np.array_equal(host_u16(dense), want)


# ---------------------------------------------------------------------------------------------------
# compute_dists
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", D.IMAGE_SHAPES)
def test_compute_dists(ops, oracle, rows, cols):
    intr = D.intrinsics(rows, cols)
    for kind in ("scene", "far"):
        depth = D.depth_image(rows, cols, 5, kind)
        src, _, dstep = D.padded(depth, D.U16_PAD, D.U16_SENTINEL)
        dst_o, view_o, sstep = D.padded(np.zeros(depth.shape, F32), D.F32_PAD, D.F32_SENTINEL)
        assert sstep % 4 == 0 and sstep > cols * 4
        D.oracle_dists(oracle, src[:, :cols], view_o, intr)
        _lib, L, st = _abi()
        s, d = dev_u16(src), dev(D.padded(np.zeros(depth.shape, F32), D.F32_PAD, D.F32_SENTINEL)[0])
        _lib.check(L.sobfu_hip_compute_dists(_p(s), C.c_int(dstep), _p(d), C.c_int(sstep), C.c_int(rows), C.c_int(cols), *[_f(v) for v in intr], st), "dists")
        got = host(d)
        assert same(got, dst_o)  # bit for bit, padding (the sentinel) included
        assert same(host(ops.compute_dists(dev_u16(depth), intr)), got[:, :cols])
        rel = D.check_dists(got[:, :cols], depth, intr)
        print("compute_dists %dx%d %s: relative error %.3e (bound %.3e)" % (rows, cols, kind, rel, D.DISTS_REL_BOUND))
        assert rel <= D.DISTS_REL_BOUND


# ---------------------------------------------------------------------------------------------------
# integrate(depth)
# ---------------------------------------------------------------------------------------------------
def gpu_integrate(ops, c, dims, poison, pitched):
    vol = dev(poison)
    if not pitched:
        ops.integrate_depth(dev(c["dists"]), vol, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        return host(vol)
    buf, _, step = D.padded(c["dists"], D.F32_PAD, D.F32_SENTINEL, guard_rows=1)  # a row of sentinels below the image as well
    _lib, L, st = _abi()
    X, Y, Z = dims
    dd = dev(buf)
    F3, F9 = C.c_float * 3, C.c_float * 9
    _lib.check(L.sobfu_hip_integrate_depth(_p(dd), C.c_int(step), C.c_int(c["dists"].shape[0]), C.c_int(c["dists"].shape[1]), _p(vol), C.c_int(X), C.c_int(Y),
                                           C.c_int(Z), F3(*[float(v) for v in c["vs"]]), _f(c["trunc"]), _f(c["eta"]),
                                           F9(*[float(v) for v in np.asarray(c["R"], F32).reshape(9)]), F3(*[float(v) for v in c["t"]]),
                                           *[_f(v) for v in c["intr"]], st), "integrate_depth")
    assert same(host(dd), buf)
    return host(vol)


@pytest.mark.parametrize("dims,pose", D.INTEGRATE_CASES)
def test_integrate_depth(ops, oracle, dims, pose):
    c = D.integrate_case(dims, pose)
    poison = D.poison_volume(dims)
    v_o = poison.copy()
    oracle.integrate_depth(c["dists"], v_o, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
    assert same(gpu_integrate(ops, c, dims, poison, pitched=True), v_o)  # written cells AND the poison of every skipped one, NaN payloads included
    v_d = gpu_integrate(ops, c, dims, poison, pitched=False)
    assert same(v_d, v_o)
    ref = D.integrate64(c["dists"], dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
    unexplained, explained, written = D.check_integrate(v_d, poison, ref)
    print("integrate %s %s: %d written, %d explained, %d unexplained" % (dims, pose, written, explained, unexplained))
    assert unexplained == 0 and explained <= D.EXPLAINED_CAP * written
    skipped = ~ref["written"] & (ref["m_px"] >= D.COO_MARGIN) & (ref["m_camz"] >= D.CAMZ_MARGIN)
    assert same(v_d[skipped], poison[skipped])  # outside the image, camz <= 0, Dp <= 0: the poison survives bit for bit


def test_integrate_depth_exact_ties(ops, oracle):
    """Constant dists images at which psdf == trunc, == -trunc and == -eta EXACTLY on one plane (identity pose, camz rebuilt in float32):
    `>=`, `<=` and `>` at equality.  The float64 reference cannot be asked here -- every cell of the plane is a tie by construction --
    so the plane is checked against what the comparisons mean: value 1, value -1, weight 0."""
    dims = (17, 9, 17)
    c = D.integrate_case(dims, "identity")
    ties = D.find_ties(dims, c)
    assert set(ties) == {"trunc", "-trunc", "-eta"}
    poison = D.poison_volume(dims)
    for name, (k, Dp) in ties.items():
        cc = dict(c, dists=np.full(D.DISTS_SHAPE, Dp, F32))
        v_o = poison.copy()
        oracle.integrate_depth(cc["dists"], v_o, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        v_d = gpu_integrate(ops, cc, dims, poison, pitched=False)
        assert same(v_d, v_o), name
        plane, pp = v_d[k], poison[k]
        wr = (plane.view(np.uint32) != pp.view(np.uint32)).any(-1)
        assert wr.sum() > 20, name
        if name == "trunc":
            assert (plane[wr][:, 0] == 1.0).all() and (plane[wr][:, 1] == 1.0).all()
        elif name == "-trunc":
            assert (plane[wr][:, 0] == -1.0).all() and (plane[wr][:, 1] == 0.0).all()
        else:
            assert (plane[wr][:, 1] == 0.0).all()  # psdf == -eta is NOT > -eta
            assert (v_d[k - 1][..., 1][(v_d[k - 1].view(np.uint32) != poison[k - 1].view(np.uint32)).any(-1)] == 1.0).all()  # one plane nearer: inside eta


def test_tile3_integrate_depth(ops, oracle):
    """tiles of a (40, 24, 35) volume under the rotated pose: each equals the slice of the whole volume (xbase / ybase / zbase replay)"""
    dims = D.TILE_DIMS
    X, Y, Z = dims
    c = D.integrate_case(dims, "rotated")
    poison = D.poison_volume(dims)
    full = gpu_integrate(ops, c, dims, poison, pitched=False)
    v_o = poison.copy()
    oracle.integrate_depth(c["dists"], v_o, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
    assert same(full, v_o)
    dd = dev(c["dists"])
    for xb, yb, zb in D.TILE_BASES:
        tile = dev(poison[zb:, yb:, xb:])
        ops.tile3_integrate_depth(dd, tile, (xb, yb, zb), c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        assert same(host(tile), full[zb:, yb:, xb:]), (xb, yb, zb)
        assert (host(tile).view(np.uint32) != poison[zb:, yb:, xb:].view(np.uint32)).any()


# ---------------------------------------------------------------------------------------------------
# fusion
# ---------------------------------------------------------------------------------------------------
COMBOS = ((0.31, 0.0), (0.0, 1.0), (-1.0, 1.0), (0.42, 1.0))  # (value, weight) of phi_n o psi: weight 0 / (0, 1) / (-1, 1) are skipped, the last is kept


def fuse_inputs(dims, variant):
    X, Y, Z = dims
    N = X * Y * Z
    i = np.arange(N)
    combo = np.where(i % 2 == 0, (i // 2) % 4, (i // 8) % 4)  # all 16 pairs of combinations among the interior pairs (N permitting)
    combo[-1] = (variant + variant // 4) % 4                   # the lone tail
    if N >= 3:
        combo[-3], combo[-2] = variant % 4, variant // 4       # the last pair
    n = np.array(COMBOS, F32)[combo]
    n[:, 0] = np.where((combo == 3) | (combo == 0), n[:, 0] + (i % 7) * F32(0.01), n[:, 0])
    n[(combo == 1) & (i % 3 == 0), 0] = -0.0                    # -0 == 0: skipped too
    g = np.empty((N, 2), F32)
    g[:, 0] = ((i % 13) - 6) * F32(0.15)
    g[:, 1] = np.array([0, 1, 2, 63, 64, 70, 5], F32)[i % 7]
    skipped = combo != 3
    return g.reshape(Z, Y, X, 2), n.reshape(Z, Y, X, 2), skipped.reshape(Z, Y, X), combo


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 1, 1), (3, 3, 3), (17, 9, 5)])
def test_integrate_fuse_odd_sizes(ops, oracle, dims):
    assert (dims[0] * dims[1] * dims[2]) % 2 == 1
    tails, last_pairs = set(), set()
    for variant in range(16):
        g, n, skipped, combo = fuse_inputs(dims, variant)
        tails.add(int(combo[-1]))
        last_pairs.add(tuple(int(v) for v in combo[-3:-1]))
        for max_weight in (1.0, 2.0, 64.0):
            g_o = g.copy()
            oracle.integrate_fuse(g_o, n, max_weight)
            g_d = dev(g)
            ops.integrate_fuse(g_d, dev(n), max_weight)
            out = host(g_d)
            assert same(out, g_o), (variant, max_weight)
            assert same(out[skipped], g[skipped])  # skipped cells keep what they held
            kept = ~skipped
            if kept.any():
                p, t = g[kept].astype(np.float64), n[kept].astype(np.float64)
                assert np.abs(out[kept][:, 0] - (p[:, 1] * p[:, 0] + t[:, 0]) / (p[:, 1] + 1)).max() < 1e-6
                assert np.array_equal(out[kept][:, 1], np.minimum(p[:, 1] + 1, max_weight).astype(F32))
                if kept.sum() > 7:
                    assert (out[kept][:, 1] == max_weight).any()
    assert tails == {0, 1, 2, 3} and (len(last_pairs) == 16 or dims == (1, 1, 1))  # the tail and the last pair saw every combination
    if dims == (17, 9, 5):
        assert len({(int(a), int(b)) for a, b in combo[:-3].reshape(-1, 2)}) == 16  # and so did the interior pairs


# ---------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------
def gpu_prim(ops, kind, dims, c):
    v = torch.full((dims[2], dims[1], dims[0], 2), 7.0, dtype=torch.float32, device="cuda")
    p = c["params"]
    if kind == "sphere":
        ops.init_sphere(v, c["vs"], c["trunc"], c["eta"], p[:3], p[3])
    elif kind == "plane":
        ops.init_plane(v, c["vs"], c["trunc"], p[0])
    else:
        getattr(ops, "init_" + kind)(v, c["vs"], c["trunc"], p)
    return host(v)


@pytest.mark.parametrize("dims", D.BUILDER_DIMS)
@pytest.mark.parametrize("kind", D.PRIMS)
def test_builders(ops, oracle, kind, dims):
    c = D.builder_case(kind, dims)
    o = D.oracle_prim(oracle, kind, dims, c)
    d = gpu_prim(ops, kind, dims, c)
    ref = D.prim64(kind, dims, c["vs"], c["trunc"], c["eta"], c["params"])
    if kind == "sphere":
        # the reference's powf(d, 2): libm on the host, a correctly rounded d * d on the device (test_gpu_parity.py::test_tsdf_builders' bounds)
        assert np.max(np.abs(d[..., 0] - o[..., 0])) <= 4e-6
        flips = d[..., 1] != o[..., 1]
        assert int(flips.sum()) <= 2
        assert (np.abs(ref["sdf"] + np.float64(c["eta"]))[flips] < D.PRIM_VALUE_TOL * np.float64(c["trunc"])).all()
    else:
        assert same(d, o)
    bad_v, bad_f, singular = D.check_prim(d, ref, c["trunc"], c["eta"])
    assert bad_v == 0 and bad_f == 0
    assert singular == (1 if kind == "ellipsoid" and all(n % 2 for n in dims) else 0)


def test_clear_volume_odd(ops):
    v = torch.full((5, 9, 17, 2), 7.0, dtype=torch.float32, device="cuda")
    guard = torch.full((9 * 17 * 5 * 2 + 6,), 7.0, dtype=torch.float32, device="cuda")
    inner = guard[3:-3].view(5, 9, 17, 2)
    ops.clear_volume(v)
    ops.clear_volume(inner)
    assert not host(v).any() and not host(inner).any()
    assert (host(guard[:3]) == 7.0).all() and (host(guard[-3:]) == 7.0).all()
