"""Warp-field diagnostics on the MI355X: sobfu_hip_warp_stats against the numpy restatement tests/warp_stats_reference.py --
the 64 result words and both volumes bit for bit, and the same again on a second run into the uncleared result buffer -- at shapes that
cross every boundary of the launch, with both the plain and the nontemporal instantiations, on identity, affine, reflected, folded and
non-finite fields, with and without masks; then ops.WarpStats' decoding, SobFusion.warp_stats and the headless app's --warp-stats."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import warp_stats_reference as WS

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")


def _gpu(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


def _run(kw, volumes=True, result=None):
    """ops.warp_stats on the arrays and settings of a restatement call -> (WarpStats, what same_bits compares)"""
    from sobfu_amd import ops

    s = ops.warp_stats(_gpu(kw["psi"]), _gpu(kw.get("psi_inv")), mask=_gpu(kw.get("mask_det")), mask_inv=_gpu(kw.get("mask_res")),
                       voxel_size=kw.get("voxel_size", (1.0, 1.0, 1.0)), band=kw.get("band", 1.0), edges=kw.get("edges", ()), res_tol=kw.get("res_tol", 0.0),
                       volumes=volumes, result=result)
    return s, dict(words=s.words, det=_cpu(s.det), res=_cpu(s.res))


def _check(name, kw, want=None):
    """both volumes and the words against the restatement; then statistics only, into a result buffer that still holds other values"""
    import torch

    want = WS.warp_stats(**kw) if want is None else want
    _, got = _run(kw)
    WS.same_bits(got, want, name)
    dirty = torch.full((64,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    for _ in range(2):  # the second run finds the first one's result
        _, again = _run(kw, volumes=False, result=dirty)
        WS.same_bits(again, want, name + ", reused buffer")
    return want


# (63 | 64 | 65, ...): around the tile's 64 lanes; Y 1, 4, 5, 9: around its 4 rows; (65, 5, 5): a chunk is 4 planes on so few tiles, so
# Z = chunk + 1 with X and Y one past a tile; (65, 32, 9) and (70, 64, 3): 8 and 16 tile rows, the XCD band mapping; (1, 262145, 1): more
# tile rows than a grid's y extent would hold
SHAPES = [(1, 1, 1), (2, 3, 4), (5, 1, 7), (1, 6, 3), (63, 4, 2), (64, 4, 2), (65, 9, 5), (65, 5, 5), (65, 32, 9), (70, 64, 3), (1, 262145, 1)]


@functools.lru_cache(maxsize=None)
def _shape_case(dims):
    """the two calls of a shape with their restatements, computed once for both instantiations"""
    psi, _ = WS.planted(dims, 7)
    masked = dict(psi=psi, psi_inv=WS.naive_inverse(psi), mask_det=WS.sphere_mask(dims, 0.75), mask_res=WS.sphere_mask(dims, 0.75, 1), band=0.75, edges=WS.EDGES,
                  res_tol=0.0005, voxel_size=(0.004, 0.005, 0.006))
    plain = dict(psi=psi, edges=WS.EDGES16)
    return (masked, WS.warp_stats(**masked)), (plain, WS.warp_stats(**plain))


@functools.lru_cache(maxsize=None)
def _field_cases():
    return [(name, kw, WS.warp_stats(**kw)) for name, kw in WS.cases()]


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("dims", SHAPES, ids=["x".join(str(v) for v in d) for d in SHAPES])
def test_shapes_match_the_restatement(dims, nt, monkeypatch):
    monkeypatch.setenv("SOBFU_LAUNCHER_NT", nt)
    assert WS.launch((65, 5, 5))[3] + 1 == 5  # the shape above that is one plane past a chunk
    (masked, want_masked), (plain, want_plain) = _shape_case(dims)
    _check("%s masked, NT=%s" % (dims, nt), masked, want_masked)
    _check("%s, NT=%s" % (dims, nt), plain, want_plain)


def test_two_equal_minima_resolve_to_the_lowest_index():
    dims = (65, 9, 5)
    psi, sites = WS.planted(dims, 7)
    want = _check("planted", dict(psi=psi, edges=(0.0,)))
    (a, b) = sites
    assert want["det"][a[2], a[1], a[0]] == want["det"][b[2], b[1], b[0]] == F(-0.5) and a[0] < b[0]
    s, _ = _run(dict(psi=psi, edges=(0.0,)))
    assert (s.det_min, s.det_min_at) == (-0.5, a) and s.n_fold >= 2 and s.det_below == (s.n_fold - int((want["det"] == 0).sum()),)


@pytest.mark.parametrize("nt", ["0", "1"])
def test_fields_and_masks_match_the_restatement(nt, monkeypatch):
    """identity, affine, reflection, folds, masks with zero weights and |tsdf| == band, empty masks, NaN / Inf in psi and psi^-1, a psi^-1
    that leaves the volume, values beyond the sums' clamp, 0 / 1 / 6 / 16 edges"""
    monkeypatch.setenv("SOBFU_LAUNCHER_NT", nt)
    assert sorted({len(kw.get("edges", ())) for _, kw in WS.cases()}) == [0, 1, 6, 16]
    for name, kw, want in _field_cases():
        _check(name, kw, want)


def test_a_thousand_workgroups_on_one_result_block():
    dims = (96, 96, 96)
    gx, gy, chunks, zc = WS.launch(dims)
    assert gx * gy * chunks >= 900 and gy % 8 == 0  # about all the workgroups the launch ever makes: it aims at 1024
    psi, _ = WS.planted(dims, 11)
    mask = WS.sphere_mask(dims, 0.9)
    want = _check("96^3", dict(psi=psi, psi_inv=WS.naive_inverse(psi), mask_det=mask, band=0.9, edges=WS.EDGES16, res_tol=0.0002, voxel_size=(0.004, 0.004, 0.004)))
    w = want["words"]
    print("96^3: %d workgroups; n_det %d folds %d n_res %d above %d outside %d" % (gx * gy * chunks, w[WS.N_DET], w[WS.N_FOLD], w[WS.N_RES], w[WS.N_RES_ABOVE], w[WS.N_RES_OUTSIDE]))
    assert w[WS.N_DET] > 50000 and w[WS.N_RES] > 500000 and w[WS.N_RES_ABOVE] > 0


@pytest.mark.parametrize("sweeps", [2, 48])
def test_the_residual_of_estimate_inverse(sweeps):
    from sobfu_amd import ops

    dims = (40, 36, 32)
    psi = WS.smooth_random(dims, 5, amplitude=1.5)
    inv = _gpu(WS.identity(dims))
    ops.estimate_inverse(_gpu(psi), inv, sweeps)
    kw = dict(psi=psi, psi_inv=_cpu(inv), res_tol=0.001, edges=WS.EDGES)
    want = _check("estimate_inverse x %d" % sweeps, kw)
    s, _ = _run(kw)
    print("sweeps %d: residual max %.9g at %s, mean %.9g, above %d, outside %d" % (sweeps, s.res_max, s.res_max_at, s.res_mean, s.n_res_above, s.n_res_outside))
    assert s.n_res + s.n_res_outside + s.n_res_nonfinite == 40 * 36 * 32 and s.n_res > 0
    if sweeps == 2:
        assert s.n_res_above > 0  # two sweeps have not converged on a field of 1.5 voxels
    else:
        assert s.res_mean < 0.01  # 48 have: a hundredth of a voxel, against ~ 0.1 after two


def test_the_decoded_values_are_the_restatements():
    dims = (11, 9, 10)
    name, kw = [c for c in WS.cases() if c[0] == "random, masks"][0]
    want = WS.warp_stats(**kw)["words"]
    s, _ = _run(kw)
    assert (s.n_det, s.n_fold, s.n_disp, s.n_res, s.n_res_above, s.n_res_outside) == tuple(int(want[k]) for k in (WS.N_DET, WS.N_FOLD, WS.N_DISP, WS.N_RES, WS.N_RES_ABOVE, WS.N_RES_OUTSIDE))
    for got, at, key, maximum in ((s.det_min, s.det_min_at, WS.DET_MIN_KEY, False), (s.det_max, s.det_max_at, WS.DET_MAX_KEY, True),
                                  (s.disp_max, s.disp_max_at, WS.DISP_MAX_KEY, True), (s.res_max, s.res_max_at, WS.RES_MAX_KEY, True)):
        v, where = WS.decode_key(want[key], maximum, dims)
        assert got == float(v) and at == where
    assert s.det_mean == WS.exact_sum(want[WS.DET_SUM_HI], want[WS.DET_SUM_LO]) / 2 ** 44 / s.n_det  # exact here: the sum is below 2^53
    assert s.fold_fraction == s.n_fold / s.n_det and s.det_below == tuple(int(v) for v in want[WS.DET_BELOW:WS.DET_BELOW + 6])
    assert s.line(3).startswith("warp 3: voxels=%d det min=%.9g @%d,%d,%d max=" % ((s.n_det, s.det_min) + s.det_min_at)) and " inv res max=" in s.line(3)


def _reference_of_fusion(arrays, vs, band):
    return WS.warp_stats(arrays["psi"], arrays["psi_inv"], arrays["phi_global"], arrays["phi_global_psi_inv"], voxel_size=vs, band=band, edges=(0, .25, .5, 1, 2, 4),
                         res_tol=float(F(0.1 * float(min(F(v) for v in vs)))))


def test_sobfusion_warp_stats():
    from sobfu_amd import ops
    from sobfu_amd import synthetic as S
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    fusion = SobFusion(P, max_iter=4)
    try:
        fusion(_gpu(S.render_sphere_depth((0.0, 0.0, 0.75), 0.1, P["intr"])))
        assert fusion.warp_stats() is None  # no solve has run
        fusion(_gpu(S.render_sphere_depth((0.005, 0.0, 0.75), 0.1, P["intr"])))
        s = fusion.warp_stats(band=0.5, volumes=True)
        arrays = {k: _cpu(getattr(fusion, k)) for k in ("psi", "psi_inv", "phi_global", "phi_global_psi_inv")}
        want = _reference_of_fusion(arrays, P["vs"], 0.5)
        WS.same_bits(dict(words=s.words, det=_cpu(s.det), res=_cpu(s.res)), want, "SobFusion")
        print(s.line(1))
        assert isinstance(s, ops.WarpStats) and 0 < s.n_det < 64 ** 3 and s.n_res > 0 and s.disp_max > 0
        assert fusion.warp_stats().words[WS.N_DET] >= s.n_det  # the default band, 1, holds the narrower one
    finally:
        fusion.close()


WARP = re.compile(r"^warp (\d+): (.*)$", re.M)


def test_app_warp_stats(tmp_path):
    from sobfu_amd import build_host, ops
    from sobfu_amd.params import read_ini

    exe = build_host.build_app()  # over the library the package has loaded: nothing of it is built here
    r = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "2", "--max-iter", "4", "--warp-stats", "--warp-stats-dump", str(tmp_path), "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    ((n, line),) = WARP.findall(r.stdout)
    print("warp %s: %s" % (n, line))
    arrays = {k: np.load(tmp_path / (k + ".npy")) for k in ("psi", "psi_inv", "phi_global", "phi_global_psi_inv")}
    want = _reference_of_fusion(arrays, read_ini(CONFIG1)["vs"], 1.0)
    twin = ops.WarpStats.from_words(want["words"], (64, 64, 64), (0, .25, .5, 1, 2, 4))
    assert int(n) == 1 and "warp 1: " + line == twin.line(1)
    det, res = np.load(tmp_path / "detJ_1.npy"), np.load(tmp_path / "invres_1.npy")
    assert det.shape == res.shape == (64, 64, 64) and det.dtype == res.dtype == F
    WS.same_bits(dict(words=want["words"], det=det, res=res), want, "the app's volumes")
    # without the flag the app prints no such line; a band that is not a positive number is refused
    r0 = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "2", "--max-iter", "4"], capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and not WARP.findall(r0.stdout)
    rb = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "2", "--warp-stats", "-1"], capture_output=True, text=True, timeout=60)
    assert rb.returncode == 2 and "--warp-stats" in rb.stdout
