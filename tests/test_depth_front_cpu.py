"""The CPU oracle against independent float64 statements of the depth front end, integrate(depth) and the TSDF builders
(tests/depth_front_reference.py), on the case list the GPU tests (tests/test_gpu_depth_edges.py) run.

Nothing here runs the HIP kernels.  These tests fix what the GPU tests may assume: the float32 error of each operation (measured here,
recorded as constants in depth_front_reference.py, times four), that the oracle -- whose every line restates the kernels -- agrees with
the float64 meaning of each operation up to that error, and that the chosen inputs keep the share of undecidable cells / pixels small.
"""
import functools

import numpy as np
import pytest

import depth_front_reference as D

F32 = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the measurements ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measure_integrate():
    coo = psdf = camz = value = 0.0
    for dims, pose in D.INTEGRATE_CASES:
        c = D.integrate_case(dims, pose)
        ref = D.integrate64(c["dists"], dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        poison = D.poison_volume(dims)
        vol, p32, px, py, wr = D.integrate32(c["dists"], poison, dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        cz32, u32, v32 = D.integrate32_chain(dims, c["vs"], c["R"], c["t"], c["intr"])
        rows, cols = c["dists"].shape
        camz = max(camz, float(np.abs(cz32.astype(np.float64) - ref["camz"]).max()))
        with np.errstate(invalid="ignore"):
            near = (ref["camz"] > 0) & (cz32 > 0) & (ref["u"] > -1) & (ref["u"] < cols + 1) & (ref["v"] > -1) & (ref["v"] < rows + 1)
        if near.any():  # (NaN / inf projections are outside `near`; the subtraction still sees them)
            with np.errstate(invalid="ignore"):
                d_u, d_v = np.abs(u32.astype(np.float64) - ref["u"]), np.abs(v32.astype(np.float64) - ref["v"])
            coo = max(coo, float(d_u[near].max()), float(d_v[near].max()))
        both = wr & ref["written"] & (px == ref["px"]) & (py == ref["py"]) & np.isfinite(ref["psdf"])
        if both.any():
            with np.errstate(invalid="ignore"):
                d_p, d_val = np.abs(p32.astype(np.float64) - ref["psdf"]), np.abs(vol[..., 0].astype(np.float64) - ref["value"])
            psdf = max(psdf, float(d_p[both].max()))
            value = max(value, float(d_val[both].max()))
    return dict(coo=coo, psdf=psdf, camz=camz, value=value)


@functools.lru_cache(maxsize=None)
def measure_images():
    import oracle

    oracle.build()
    rel = q = 0.0
    for rows, cols in D.IMAGE_SHAPES:
        for kind in ("scene", "far"):
            depth = D.depth_image(rows, cols, 5, kind)
            rel = max(rel, D.check_dists(oracle.compute_dists(depth, D.intrinsics(rows, cols)), depth, D.intrinsics(rows, cols)))
    for rows, cols, ksz, ss, sd, kind in D.BILATERAL_CASES:
        depth = D.depth_image(rows, cols, D.BILATERAL_SEED, kind)
        assert depth[depth != 65535].max(initial=0) <= 8000
        q64, poisoned, _ = D.bilateral64(depth, ksz, ss, sd)
        q32 = D.bilateral32(depth, ksz, ss, sd).astype(np.float64)
        ok = ~poisoned & ~np.isnan(q64)
        assert not np.isnan(q32[ok]).any()
        if ok.any():
            q = max(q, float(np.abs(q32 - q64)[ok].max()))
    return dict(dists_rel=rel, bilateral_q=q)


@functools.lru_cache(maxsize=None)
def measure_builders():
    import oracle

    oracle.build()
    v = 0.0
    for dims in D.BUILDER_DIMS:
        for kind in D.PRIMS:
            c = D.builder_case(kind, dims)
            ref = D.prim64(kind, dims, c["vs"], c["trunc"], c["eta"], c["params"])
            o = D.oracle_prim(oracle, kind, dims, c)
            v = max(v, float(np.abs(o[..., 0].astype(np.float64) - ref["value"])[~ref["singular"]].max()))
    return dict(prim_value=v)


def test_print_measured(capsys):
    """prints the figures the constants of depth_front_reference.py record (pytest -s)"""
    m = {**measure_integrate(), **measure_images(), **measure_builders()}
    with capsys.disabled():
        print()
        for k, v in m.items():
            print("measured %-12s %.6e   threshold (x4) %.6e" % (k, v, 4 * v))


def test_recorded_thresholds_match_measurement():
    """the recorded figures are the measured ones rounded up to two digits, not looser; the thresholds are 4 x them"""
    m = {**measure_integrate(), **measure_images(), **measure_builders()}
    rec = dict(coo=D.MEASURED_COO, psdf=D.MEASURED_PSDF, camz=D.MEASURED_CAMZ, value=D.MEASURED_VALUE, dists_rel=D.MEASURED_DISTS_REL,
               bilateral_q=D.MEASURED_BILATERAL_Q, prim_value=D.MEASURED_PRIM_VALUE)
    for k in rec:
        assert m[k] <= rec[k] <= 1.05 * m[k], (k, m[k], rec[k])
    assert (D.COO_MARGIN, D.PSDF_MARGIN, D.CAMZ_MARGIN, D.VALUE_TOL) == (4 * D.MEASURED_COO, 4 * D.MEASURED_PSDF, 4 * D.MEASURED_CAMZ, 4 * D.MEASURED_VALUE)
    assert (D.DISTS_REL_BOUND, D.BILATERAL_DELTA, D.PRIM_VALUE_TOL) == (4 * D.MEASURED_DISTS_REL, 4 * D.MEASURED_BILATERAL_Q, 4 * D.MEASURED_PRIM_VALUE)
    assert D.MEASURED_DISTS_REL < 8 * 2.0 ** -24  # "a few units of 2^-24"


# ---- integrate(depth) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,pose", D.INTEGRATE_CASES)
def test_integrate_oracle_vs_float64(oracle, dims, pose):
    c = D.integrate_case(dims, pose)
    poison = D.poison_volume(dims)
    vol = poison.copy()
    oracle.integrate_depth(c["dists"], vol, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
    # the float32 chain the figures were measured on IS the oracle's
    assert same(vol, D.integrate32(c["dists"], poison, dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])[0])
    ref = D.integrate64(c["dists"], dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
    unexplained, explained, written = D.check_integrate(vol, poison, ref)
    assert unexplained == 0
    assert explained <= D.EXPLAINED_CAP * written, (explained, written)


def test_integrate_cases_reach_every_branch():
    """the case list holds what the issue asks of it: every skip reason, both clamps, both weights, NaN and inf measurements, camz == 0"""
    for pose in D.POSES:
        dims = (40, 24, 35)
        c = D.integrate_case(dims, pose)
        ref = D.integrate64(c["dists"], dims, c["vs"], c["trunc"], c["eta"], c["R"], c["t"], c["intr"])
        rows, cols = c["dists"].shape
        with np.errstate(invalid="ignore"):
            outside = (ref["camz"] > 0) & ~ref["inside"]
        assert outside.sum() > 50 and (ref["inside"] & ~ref["written"]).sum() > 50  # off the image; Dp <= 0
        w = ref["written"]
        assert (w & (ref["value"] == 1)).sum() > 50 and (w & (ref["value"] == -1)).sum() > 50 and (w & (np.abs(ref["value"]) < 1)).sum() > 50
        assert (w & (ref["weight"] == 0)).sum() > 50 and (w & np.isnan(ref["value"])).sum() > 10 and (w & np.isinf(ref["psdf"])).sum() > 10
        seen = np.zeros((rows, cols), bool)
        seen[ref["py"][ref["inside"]], ref["px"][ref["inside"]]] = True
        assert not seen.all()  # part of the image is seen by no voxel
        if pose == "inside":
            assert (ref["camz"] < 0).sum() > 50 and (ref["camz"] == 0).sum() == 40 * 24
            cz, u, v = D.integrate32_chain(dims, c["vs"], c["R"], c["t"], c["intr"])
            assert (cz == 0).sum() == 40 * 24 and np.isnan(u).sum() == 24 and np.isnan(v).sum() == 40 and np.isinf(u).sum() > 0
            assert (np.isnan(u) & np.isnan(v)).sum() == 1  # the camera's own voxel: 0 / 0 in both
            assert ((v == F32(rows)) & (cz > 0)).sum() >= 40 and (ref["v"] == rows).sum() >= 40  # cooy == rows exactly: `>=` skips them
            for a, n in ((ref["u"], cols), (ref["v"], rows)):  # off every side
                with np.errstate(invalid="ignore"):
                    assert ((ref["camz"] > 0) & (a < 0)).any() and ((ref["camz"] > 0) & (a >= n)).any()


def test_tie_search_finds_all_three():
    dims = (17, 9, 17)
    c = D.integrate_case(dims, "identity")
    ties = D.find_ties(dims, c)
    assert set(ties) == {"trunc", "-trunc", "-eta"}
    camz = D.integrate32_chain(dims, c["vs"], c["R"], c["t"], c["intr"])[0][:, 0, 0]
    for name, T in (("trunc", c["trunc"]), ("-trunc", -c["trunc"]), ("-eta", -c["eta"])):
        k, Dp = ties[name]
        assert F32(Dp - camz[k]) == F32(T)


# ---- dists ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", D.IMAGE_SHAPES)
def test_dists_oracle_vs_float64(oracle, rows, cols):
    intr = D.intrinsics(rows, cols)
    for kind in ("scene", "far"):
        depth = D.depth_image(rows, cols, 5, kind)
        assert D.check_dists(oracle.compute_dists(depth, intr), depth, intr) <= D.DISTS_REL_BOUND


# ---- bilateral ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.BILATERAL_CASES, ids=lambda c: "%dx%d-k%d-%s-sd%g" % (c[0], c[1], c[2], c[5], c[4]))
def test_bilateral_oracle_vs_float64(oracle, case):
    rows, cols, ksz, ss, sd, kind = case
    depth = D.depth_image(rows, cols, D.BILATERAL_SEED, kind)
    out = oracle.bilateral(depth, ksz, ss, sd)
    q64, poisoned, starved = D.bilateral64(depth, ksz, ss, sd)
    assert starved.sum() <= 0.005 * rows * cols and not starved[:-1, :-1].any()
    wrong, band = D.check_bilateral(out, q64, poisoned)
    assert wrong == 0
    assert band <= D.BAND_CAP * rows * cols, (band, rows * cols)
    if min(rows, cols) == 1:
        assert not out.any() and np.isnan(q64).all()  # the window is empty: 0 / 0 -> 0
    if kind == "saturated":
        assert poisoned.sum() > 4 and (depth == 65535).sum() > 2 and not out[poisoned].any()  # inf weights: NaN -> 0


def test_bilateral_ksz1_is_identity_off_the_last_row_and_column(oracle):
    depth = D.depth_image(9, 130, D.BILATERAL_SEED)
    out = oracle.bilateral(depth, 1, 4.5, 0.005)
    assert np.array_equal(out[:-1, :-1], depth[:-1, :-1]) and not out[-1].any() and not out[:, -1].any()


# ---- builders -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", D.BUILDER_DIMS)
@pytest.mark.parametrize("kind", D.PRIMS)
def test_builders_oracle_vs_float64(oracle, kind, dims):
    c = D.builder_case(kind, dims)
    ref = D.prim64(kind, dims, c["vs"], c["trunc"], c["eta"], c["params"])
    o = D.oracle_prim(oracle, kind, dims, c)
    bad_v, bad_f, singular = D.check_prim(o, ref, c["trunc"], c["eta"])
    assert bad_v == 0 and bad_f == 0
    assert singular == (1 if kind == "ellipsoid" and all(n % 2 for n in dims) else 0)


@pytest.mark.parametrize("kind", D.PRIMS)
def test_builder_cases_reach_every_branch(kind):
    v, w = [], []
    for dims in D.BUILDER_DIMS:
        c = D.builder_case(kind, dims)
        ref = D.prim64(kind, dims, c["vs"], c["trunc"], c["eta"], c["params"])
        v.append(ref["value"][~ref["singular"]].reshape(-1))
        w.append(ref["weight"].reshape(-1))
    v, w = np.concatenate(v), np.concatenate(w)
    assert (v == 1).sum() > 20 and (v == -1).sum() > 20 and (np.abs(v) < 1).sum() > 20
    assert kind != "sphere" or ((w == 0).sum() > 50 and (w == 1).sum() > 50)
