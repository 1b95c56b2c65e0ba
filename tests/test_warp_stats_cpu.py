"""Warp-field diagnostics on the CPU: the C ABI's entry point (exported, ABI version unchanged, every argument check before
any device call), the numpy restatement tests/warp_stats_reference.py against the header itself as a host compiler takes it
(sobfu_amd/csrc/sobfu_warp_stats.hpp) bit for bit, the same cases through a build of the tool with the address and undefined-behaviour
sanitizers, and the properties of the restatement -- which the GPU shares, because tests/test_gpu_warp_stats.py holds it to the
restatement bit for bit."""
import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import warp_stats_reference as WS

F = np.float32
A, B, D, E, G, H, K = (C.c_void_p(4096 * k) for k in range(1, 8))  # 16-byte aligned addresses that are never dereferenced


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_warp_stats_tool()


@pytest.fixture(scope="module")
def sanitized_tool():
    from sobfu_amd import build_host

    return build_host.build_warp_stats_tool(flags=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], out="warp_stats_tool_sanitized")


def test_symbol_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    assert "sobfu_hip_warp_stats" in _lib.declared_symbols() and hasattr(lib, "sobfu_hip_warp_stats")
    assert lib.sobfu_hip_abi_version() == 3


# ---- argument checks: every case is refused before any device call ---------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(psi=A, inv=B, mdet=D, mres=E, X=8, Y=8, Z=8, vs=(0.01, 0.01, 0.01), band=1.0, edges=(0.0, 0.5, 1.0), n_edges=None, tol=0.001, result=G,
             det=H, res=K)
    a.update(kw)
    edges = a["edges"]
    n_edges = a["n_edges"] if a["n_edges"] is not None else (len(edges) if edges is not None else 0)
    earr = (C.c_float * max(len(edges), 1))(*edges) if edges is not None else None
    vs = (C.c_float * 3)(*a["vs"]) if a["vs"] is not None else None
    return lib.sobfu_hip_warp_stats(a["psi"], a["inv"], a["mdet"], a["mres"], a["X"], a["Y"], a["Z"], vs, C.c_float(a["band"]), earr, n_edges, C.c_float(a["tol"]),
                                    a["result"], a["det"], a["res"], None)


NAN, INF = float("nan"), float("inf")
BAD = [dict(psi=None), dict(result=None), dict(vs=None),
       dict(psi=C.c_void_p(A.value + 8)), dict(inv=C.c_void_p(B.value + 8)), dict(mdet=C.c_void_p(D.value + 4)), dict(mres=C.c_void_p(E.value + 4)),
       dict(result=C.c_void_p(G.value + 4)), dict(det=C.c_void_p(H.value + 2)), dict(res=C.c_void_p(K.value + 2)),
       dict(inv=None), dict(inv=None, mres=None), dict(inv=None, res=None),  # d_res or d_mask_res without d_psi_inv
       dict(X=0), dict(Y=0), dict(Z=0), dict(X=-1), dict(Z=-4), dict(X=2048, Y=2048, Z=513), dict(X=65536, Y=65536, Z=1), dict(X=1 << 30, Y=1 << 30, Z=1 << 30),
       dict(vs=(0.0, 0.01, 0.01)), dict(vs=(0.01, -0.01, 0.01)), dict(vs=(0.01, 0.01, NAN)), dict(vs=(INF, 0.01, 0.01)),
       dict(band=0.0), dict(band=-1.0), dict(band=NAN), dict(band=INF),
       dict(tol=-1e-9), dict(tol=NAN),
       dict(n_edges=-1), dict(n_edges=17, edges=tuple(range(17))), dict(edges=None, n_edges=2),
       dict(edges=(0.0, 0.0)), dict(edges=(1.0, 0.5)), dict(edges=(0.0, NAN)), dict(edges=(0.0, INF)), dict(edges=(-INF, 0.0))]


@pytest.mark.parametrize("kw", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_arguments(lib, kw):
    assert _call(lib, **kw) == -1


# ---- the header through a host compiler ------------------------------------------------------------------------------------------------
def _run(tool, tmp_path, psi, psi_inv=None, mask_det=None, mask_res=None, voxel_size=(1.0, 1.0, 1.0), band=1.0, edges=(), res_tol=0.0):
    Z, Y, X = psi.shape[:3]
    e16 = np.zeros(16, F)
    e16[:len(edges)] = edges
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([X, Y, Z, psi_inv is not None, mask_det is not None, mask_res is not None, len(edges)], np.int32).tobytes())
        fh.write(np.array(list(voxel_size) + [band, res_tol], F).tobytes() + e16.tobytes())
        for arr in (psi, psi_inv, mask_det, mask_res):
            if arr is not None:
                fh.write(np.ascontiguousarray(arr, F).tobytes())
    r = subprocess.run([tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=300)
    assert r.returncode == 0
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = X * Y * Z
    assert raw.size == 8 * 64 + 4 * n * (2 if psi_inv is not None else 1)
    vols = raw[512:].view(F)
    return dict(words=raw[:512].view(np.uint64), det=vols[:n].reshape(Z, Y, X), res=vols[n:].reshape(Z, Y, X) if psi_inv is not None else None)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_on_the_cpu_equals_the_restatement(which, tool, sanitized_tool, tmp_path):
    """result words and both volumes bit for bit; the second round runs the same cases through the tool built with
    -fsanitize=address,undefined"""
    exe = sanitized_tool if which == "sanitized" else tool
    for name, kw in WS.cases():
        want = WS.warp_stats(**kw)
        got = _run(exe, tmp_path, **kw)
        w = want["words"]
        print("%s: n_det %d folds %d non-finite %d, n_res %d above %d outside %d non-finite %d" % (name, w[WS.N_DET], w[WS.N_FOLD], w[WS.N_DET_NONFINITE], w[WS.N_RES],
                                                                                                   w[WS.N_RES_ABOVE], w[WS.N_RES_OUTSIDE], w[WS.N_RES_NONFINITE]))
        WS.same_bits(got, want, name)


def test_the_cases_are_what_the_tests_need():
    got = {name: WS.warp_stats(**kw)["words"] for name, kw in WS.cases()}
    w = got["random, no mask"]
    assert w[WS.N_FOLD] > 0 and w[WS.N_RES_ABOVE] > 0 and w[WS.N_RES_OUTSIDE] > 0 and w[WS.N_RES] + w[WS.N_RES_OUTSIDE] == 11 * 9 * 10 and w[WS.DET_BELOW + 15] > w[WS.DET_BELOW + 4] > 0
    w = got["random, masks"]
    assert 0 < w[WS.N_DET] < 11 * 9 * 10 and 0 < w[WS.N_RES] < 11 * 9 * 10 and w[WS.N_DET] != w[WS.N_RES]
    w = got["non-finite and outside"]
    assert w[WS.N_DET_NONFINITE] > 3 and w[WS.N_DISP_NONFINITE] == 3 and w[WS.N_RES_OUTSIDE] >= 3 and w[WS.N_RES_NONFINITE] >= 3
    w = got["beyond the clamp"]
    assert WS.exact_sum(w[WS.DET_SUM_HI], w[WS.DET_SUM_LO]) == 990 * 1024 * 2 ** 44  # every det = 2.7e10, clamped to 1024


@pytest.mark.parametrize("dims", [(1, 1, 1), (63, 4, 2), (65, 9, 5), (64, 32, 40), (96, 96, 96), (1, 262145, 1), (256, 256, 256), (3, 1, 5000)])
def test_the_launch_covers_the_volume_once(tool, dims):
    """ws_launch / ws_tile as g++ takes them: every (tile, chunk) exactly once (the tool's exit status), the chunks cover Z, and the
    restatement's launch() agrees"""
    r = subprocess.run([tool, "launch"] + [str(v) for v in dims], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert tuple(int(v) for v in r.stdout.split()) == WS.launch(dims)


# ---- properties of the restatement -----------------------------------------------------------------------------------------------------
def _decode(words, dims):
    n = int(words[WS.N_DET])
    return dict(det_min=WS.decode_key(words[WS.DET_MIN_KEY], False, dims), det_max=WS.decode_key(words[WS.DET_MAX_KEY], True, dims),
                disp_max=WS.decode_key(words[WS.DISP_MAX_KEY], True, dims), res_max=WS.decode_key(words[WS.RES_MAX_KEY], True, dims),
                det_mean=WS.exact_sum(words[WS.DET_SUM_HI], words[WS.DET_SUM_LO]) / 2.0 ** 44 / n if n else float("nan"))


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 4), (5, 1, 7), (1, 6, 3), (9, 8, 7)])
def test_identity(dims):
    """det == 1 at every voxel, boundary included; no displacement; no residual against psi^-1 = identity; both det keys report linear
    index 0 (the tie rule)"""
    psi = WS.identity(dims)
    s = WS.warp_stats(psi, psi_inv=psi, edges=WS.EDGES, voxel_size=(0.01, 0.02, 0.03))
    n, w = dims[0] * dims[1] * dims[2], s["words"]
    assert np.all(s["det"].view(np.uint32) == F(1).view(np.uint32)) and np.all(s["res"].view(np.uint32) == 0)
    assert w[WS.N_DET] == n and w[WS.N_FOLD] == 0 and w[WS.N_DISP] == n and w[WS.N_RES] == n and w[WS.N_RES_ABOVE] == 0
    assert [int(v) for v in w[WS.DET_BELOW:WS.DET_BELOW + 6]] == [0, 0, 0, 0, n, n]
    dec = _decode(w, dims)
    assert dec["det_min"] == (F(1), (0, 0, 0)) and dec["det_max"] == (F(1), (0, 0, 0)) and dec["det_mean"] == 1.0
    assert dec["disp_max"] == (F(0), (0, 0, 0)) and dec["res_max"] == (F(0), (0, 0, 0))
    assert WS.exact_sum(w[WS.DET_SUM_HI], w[WS.DET_SUM_LO]) == n << 44 and WS.exact_sum(w[WS.DISP_SUM_HI], w[WS.DISP_SUM_LO]) == 0


def test_affine_has_det_A_everywhere():
    """psi = A x + b: u = (A - I) x + b is linear, so the one-sided boundary differences equal the central ones.  Each u is rounded once at
    a magnitude <= c = |A - I| 12 + |b| < 8 (relative 2^-24), a difference of two adds 2 c 2^-24 plus its own rounding: every entry of J is
    within 4 c 2^-24 of A's, and det (six products of three entries <= 1.3, each chain a few roundings) within 6 x 3 x 1.3^2 x 4 c 2^-24
    plus 16 roundings of a value <= 3: tol = (122 c + 48) 2^-24"""
    dims = (11, 9, 10)
    A_ = np.array([[1.1, 0.2, -0.1], [0.05, 0.9, 0.15], [-0.2, 0.1, 1.2]])
    b = [0.5, -0.25, 1.0]
    c = np.abs(A_ - np.eye(3)).sum(1).max() * 12 + 1.0
    tol = (122 * c + 48) * 2.0 ** -24
    s = WS.warp_stats(WS.affine(dims, A_, b))
    err = np.abs(s["det"].astype(np.float64) - np.linalg.det(A_)).max()
    print("affine: det A %.9g, max |det - det A| %.3g, tol %.3g" % (np.linalg.det(A_), err, tol))
    assert err <= tol and s["words"][WS.N_FOLD] == 0


def test_a_reflection_folds_every_voxel():
    dims = (7, 5, 6)
    s = WS.warp_stats(WS.reflection(dims), edges=(0.0,))
    assert np.all(s["det"] == F(-1)) and s["words"][WS.N_FOLD] == 210 and s["words"][WS.DET_BELOW] == 210


def test_one_voxel_pushed_back_folds_the_voxels_that_see_it():
    """identity with voxel (5, 4, 5) pushed 3 cells back along x.  Its own x derivative does not see it; d_x u_x of (4, 4, 5) is
    (-3 - 0) / 2 = -1.5, J_00 = -0.5: folded; of (6, 4, 5) it is (0 - -3) / 2 = 1.5, J_00 = 2.5: not folded.  The y and z neighbours
    see d_y u_x, d_z u_x = -+1.5 in an off-diagonal entry of a matrix that is otherwise the identity: det stays 1.  So exactly one voxel
    folds, the minimum is -0.5 there and the maximum 2.5 at (6, 4, 5)"""
    dims = (11, 9, 10)
    s = WS.warp_stats(WS.plant_fold(WS.identity(dims), (5, 4, 5)), edges=(0.0,))
    dec = _decode(s["words"], dims)
    assert s["words"][WS.N_FOLD] == 1 and dec["det_min"] == (F(-0.5), (4, 4, 5)) and dec["det_max"] == (F(2.5), (6, 4, 5))
    assert int((s["det"] != 1).sum()) == 2
    # at the boundary the one-sided difference is not halved: voxel (1, 4, 5) pushed back is seen by (0, 4, 5) as -3, J_00 = -2
    s = WS.warp_stats(WS.plant_fold(WS.identity(dims), (1, 4, 5)))
    assert _decode(s["words"], dims)["det_min"] == (F(-2), (0, 4, 5)) and s["words"][WS.N_FOLD] == 1


def test_translating_psi_changes_no_det():
    dims = (11, 9, 10)
    psi = WS.smooth_random(dims, 3)  # on a 2^-10 grid: psi + t is exact for a dyadic t, so u moves by exactly t
    moved = psi.copy()
    moved[..., :3] += np.array([2.5, -1.25, 0.75], F)
    a, b = WS.warp_stats(psi), WS.warp_stats(moved)
    assert np.array_equal(a["det"].view(np.uint32), b["det"].view(np.uint32))
    assert all(a["words"][k] == b["words"][k] for k in (WS.N_DET, WS.N_FOLD, WS.DET_SUM_HI, WS.DET_SUM_LO, WS.DET_MIN_KEY, WS.DET_MAX_KEY))


def test_the_sum_is_the_exact_rational_sum_of_the_quantised_terms():
    dims = (11, 9, 10)
    psi = WS.smooth_random(dims, 4, amplitude=2.0)
    s = WS.warp_stats(psi, voxel_size=(0.004, 0.004, 0.004))
    det = s["det"].reshape(-1)
    want = sum(Fraction(int(round(Fraction(float(v)) * 2 ** 44))) for v in det)  # round(): half to even, as llrint
    assert Fraction(WS.exact_sum(s["words"][WS.DET_SUM_HI], s["words"][WS.DET_SUM_LO])) == want
    assert abs(float(want) / 2 ** 44 - det.astype(np.float64).sum()) <= len(det) * 2.0 ** -45
    assert 0 <= int(s["words"][WS.DET_SUM_LO]) < len(det) << 24


def test_an_empty_mask_decodes_to_nan_and_minus_one():
    dims = (5, 4, 3)
    mask = np.zeros((3, 4, 5, 2), F)
    psi = WS.smooth_random(dims, 5)
    s = WS.warp_stats(psi, psi_inv=psi, mask_det=mask, mask_res=mask)
    assert not s["words"][:31].any() and all(int(k) == WS.EMPTY_KEY for k in s["words"][31:35])
    for k, maximum in ((WS.DET_MIN_KEY, False), (WS.DET_MAX_KEY, True), (WS.DISP_MAX_KEY, True), (WS.RES_MAX_KEY, True)):
        v, at = WS.decode_key(s["words"][k], maximum, dims)
        assert np.isnan(v) and at == (-1, -1, -1)
    assert np.isfinite(s["det"]).all()  # the volume is written irrespective of the mask


def test_keys_order_like_floats_and_ties_take_the_lowest_index():
    v = np.array([-np.inf, -2.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, np.inf], F)
    o = WS.ordered(v).astype(np.int64)
    assert np.all(np.diff(o)[[0, 1, 2, 4, 5, 6]] > 0) and o[3] == o[4]  # -0 is +0
    idx = np.arange(4, dtype=np.uint64)
    vals = np.array([2.0, -1.0, -1.0, 2.0], F)
    assert WS.decode_key(WS.min_key(vals, idx), False, (4, 1, 1)) == (F(-1), (1, 0, 0))
    assert WS.decode_key(WS.max_key(vals, idx), True, (4, 1, 1)) == (F(2), (0, 0, 0))
