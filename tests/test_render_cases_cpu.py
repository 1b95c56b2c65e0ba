"""The cases of tests/test_gpu_render_edges.py, checked on the CPU with the numpy restatement alone (tests/render_cases.py,
tests/render_reference.py): every case reaches the edge it is named for -- hits and misses among the rays that enter the box, clamped
central differences, exact D == 0 components inside and outside their slabs, a camera centre exactly on a face, a valid -> invalid ->
valid march, NaN weights and non-finite voxels that change a pixel, a crossing whose gradient is exactly zero -- and no march reaches
the host's step bound.  Run with -s to see the figures."""
import numpy as np
import pytest

import render_cases as K
import render_reference as RR


def _hit(name):
    return K.reference(name)["normals"][..., 3] != 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", K.CASES)
def test_case_reaches_its_edge(name):
    c, r = K.case(name), K.reference(name)
    tr, hit = r["trace"], _hit(name)
    X, Y, Z = K.dims_of(c["vol"])
    enters = tr["enters"]
    n_hit, n_miss = int(hit.sum()), int((enters & ~hit).sum())
    print(f"\n{name}: {X} x {Y} x {Z}, {c['rows']} x {c['cols']}: {int(enters.sum())} rays enter, {n_hit} hit, {n_miss} of them miss; "
          f"{int(tr['crossing'].sum())} crossings, {int(tr['regained'].sum())} regain validity; at most {int(tr['samples'].max())} samples, bound {tr['max_steps']}")
    assert max(X, Y, Z) <= 40 and X * Y * Z <= 24 ** 3 and c["rows"] <= 40 and c["cols"] <= 70
    assert r["points"].shape == (c["rows"], c["cols"], 4) and not hit[~enters].any()
    assert (_bits(r["points"])[~hit] == 0).all() and (_bits(r["normals"])[~hit] == 0).all()  # a miss is all +0
    assert np.isfinite(r["points"]).all() and np.isfinite(r["normals"]).all()
    assert int(tr["samples"].max()) < tr["max_steps"]  # "a bound, never reached by a march"
    if name in K.ALL_MISS_CASES:
        assert n_hit == 0
    elif name not in K.COUNT_EXEMPT:
        assert n_hit >= 20 and n_miss >= 20
    if name in K.SIZE_CASES:
        assert (c["rows"], c["cols"]) in K.SIZES
    if name == "size_1x1":
        assert n_hit == 1
    if name == "away":
        assert not enters.any()  # tmax < tmin, or the z >= 0 clip
    if name == "cleared":
        assert enters.sum() >= 100 and not c["vol"].any()
    if name == "far":
        assert 1 <= enters.sum() <= 8 and n_hit >= 1
    if name == "inside":
        o = -c["R"].astype(np.float64).T @ c["t"].astype(np.float64)
        assert ((o > 0.015) & (o < K.extent((X, Y, Z), c["vs"]) - 0.015)).all() and enters.all()  # more than a voxel inside every face
    if name == "vol_2x2x2":
        f = c["vol"][..., 0]
        assert (f[0] > 0).all() and (f[1] < 0).all() and (c["vol"][..., 1] > 0).all()


@pytest.mark.parametrize("name", K.PLANE_CASES)
def test_face_planes_clamp_the_central_difference(name):
    """hits whose g + 1 is above top (faces *1) or whose g - 1 is below 0 (faces *0) on the face's axis: fminf / fmaxf act"""
    c = K.case(name)
    axis, top = "xyz".index(name[6]), name[7] == "1"
    g = K.hit_grid(name)[axis][_hit(name)]
    t = np.float32(K.dims_of(c["vol"])[axis] - 1)
    clamped = (g + np.float32(1) > t) if top else (g - np.float32(1) < 0)
    print(f"\n{name}: {int(clamped.sum())} of {g.size} hits clamped, g in [{g.min():.3f}, {g.max():.3f}]")
    assert clamped.sum() >= 20 and ((g >= t - 1) if top else (g <= 1)).all()  # the crossing is within a voxel of the face


def test_clamps_on_both_sides_of_every_axis_elsewhere_too():
    for name in ("rotated", "on_face_z0", "vol_2x2x2"):
        c, hit = K.case(name), _hit(name)
        for axis, d in enumerate(K.dims_of(c["vol"])):
            g = K.hit_grid(name)[axis][hit]
            assert ((g + np.float32(1) > d - 1) | (g - np.float32(1) < 0)).any()
    g = [a[_hit("vol_2x2x2")] for a in K.hit_grid("vol_2x2x2")]  # top == 1: both clamps at once, on every hit
    assert all(((a + np.float32(1) > 1) & (a - np.float32(1) < 0)).all() for a in g)


@pytest.mark.parametrize("name", K.AXIS_CASES)
def test_axis_parallel_rays(name):
    """the principal ray has two D components that are exactly 0; in *_in both lie inside their slabs and the ray enters, in *_out one
    lies outside and the ray is clipped by `tmin = inf`; its row and column have one zero component each"""
    c, tr = K.case(name), K.reference(name)["trace"]
    cx, cy = int(c["intr"][2]), int(c["intr"][3])
    assert (cx, cy) == c["intr"][2:] and 0 < cx < c["cols"] - 1 and 0 < cy < c["rows"] - 1
    D, O = [d[cy, cx] for d in tr["D"]], tr["O"]
    zero = [i for i in range(3) if D[i] == 0]
    assert len(zero) == 2
    tops = [d - 1 for d in K.dims_of(c["vol"])]
    inside = [bool(0 <= O[i] <= tops[i]) for i in zero]
    print(f"\n{name}: D = {D}, O = {O}, zero axes {zero}, inside their slabs {inside}")
    if name.endswith("_in"):
        assert all(inside) and tr["enters"][cy, cx] and tr["samples"][cy, cx] > 5
    else:
        assert inside.count(False) == 1 and not tr["enters"][cy, cx]
        assert tr["enters"].sum() >= 40  # other rays still reach the box
    assert sum(int((d == 0).sum()) for d in tr["D"]) == c["rows"] + c["cols"]  # one row and one column, the principal ray in both


@pytest.mark.parametrize("name", K.ON_FACE_CASES)
def test_camera_centre_exactly_on_a_face(name):
    """O is exactly 0 or dim - 1 on the face's axis, so the first sample of every ray has cf == 0 or cf == top there (tri_setup: h = g)"""
    c, tr = K.case(name), K.reference(name)["trace"]
    axis, top = "xyz".index(name[8]), name[9] == "1"
    want = np.float32(K.dims_of(c["vol"])[axis] - 1 if top else 0)
    assert tr["O"][axis] == want and tr["enters"].all()
    g0 = RR.fma(np.float32(0), tr["D"][axis], tr["O"][axis])  # tmin == 0
    assert (g0 == want).all()
    g, h, t = RR.tri_setup(g0, K.dims_of(c["vol"])[axis])
    assert (h == g).all() and (t == 0).all()
    D = tr["D"][axis]
    assert ((D < 0) if top else (D > 0)).all()  # into the volume


def test_some_ray_regains_validity():
    names = [n for n in K.CASES if K.reference(n)["trace"]["regained"].any()]
    hits_after = [n for n in names if (K.reference(n)["trace"]["regained"] & _hit(n)).any()]
    print("\nvalid -> invalid -> valid:", names, "\nand then a hit:", hits_after)
    assert "outside" in names and "rotated" in hits_after
    w = K.field_volume()[..., 1]
    assert set(np.unique(w)) == {0, 1, 2, 3, 4} and 0.02 < (w == 0).mean() < 0.04
    f = K.field_volume()[..., 0]
    assert f.min() == -1 and f.max() == 1 and (np.abs(f) < 1).mean() > 0.5


def test_planted_voxels_are_seen():
    """each planted kind changes a pixel of `outside`: NaN weights turn hits into other results (the samples they are corners of would
    be crossings with the weight 1 they replace), NaN / +-Inf tsdf values make crossings without a hit (a NaN gradient) or move hits"""
    base = K.reference("outside")
    bvol = K.case("outside")["vol"]
    for name in tuple(K.NONFINITE) + ("nan_weight",):
        c, r = K.case(name), K.reference(name)
        ch = 1 if name == "nan_weight" else 0
        planted = _bits(c["vol"][..., ch]) != _bits(bvol[..., ch])
        assert 1 <= planted.sum() <= 3 and np.array_equal(_bits(c["vol"][..., 1 - ch]), _bits(bvol[..., 1 - ch]))
        v = c["vol"][..., ch][planted]
        assert (np.isnan(v).all() if "nan" in name else (v == K.NONFINITE[name]).all()) and (c["vol"][..., 1][planted] != 0).all()
        changed = (_bits(r["points"]) != _bits(base["points"])).any(-1) | (_bits(r["normals"]) != _bits(base["normals"])).any(-1)
        lost = (base["normals"][..., 3] != 0) & (r["normals"][..., 3] == 0)
        print(f"\n{name}: {int(planted.sum())} voxels planted, {int(changed.sum())} pixels change, {int(lost.sum())} hits become misses, "
              f"{int((r['trace']['crossing'] & (r['normals'][..., 3] == 0)).sum())} crossings without a hit")
        assert changed.sum() >= 1
        if name == "nan_weight":
            # with the NaN read as "observed" (weight 1 in its place) the result is `outside`'s: the pixels that change are exactly those where
            # a sample with a NaN corner would have been one side of a crossing
            one = c["vol"].copy()
            one[..., 1][planted] = 1
            p1, n1 = RR.raycast(one, *K.args(c), step_factor=c["step_factor"])
            assert lost.sum() >= 1 and (n1[..., 3] != 0)[lost].all() and (bvol[..., 1][planted] > 0).all()
        else:
            assert (r["trace"]["crossing"] & (r["normals"][..., 3] == 0)).any()


def test_zero_gradient_crossings_exist():
    """crossings whose three central differences cancel exactly: the restatement (and the kernel) writes a miss"""
    c, r = K.case("zero_gradient"), K.reference("zero_gradient")
    tr, hit = r["trace"], _hit("zero_gradient")
    dead = tr["crossing"] & ~hit
    print(f"\nzero_gradient: {int(tr['crossing'].sum())} crossings, {int(dead.sum())} with a zero gradient, {int(hit.sum())} hits")
    assert dead.sum() >= 20 and np.isfinite(c["vol"]).all()
    assert not r["points"][dead].any() and not r["normals"][dead].any()


def test_step_factors_and_truncation_change_the_march():
    s = {n: K.reference(n)["trace"]["samples"] for n in ("step_0.25", "step_0.75", "step_2.0", "trunc_wide")}
    assert s["step_0.25"].max() > s["step_0.75"].max() > s["step_2.0"].max()
    assert not np.array_equal(s["trunc_wide"], s["step_0.75"]) and K.case("trunc_wide")["trunc"] != K.case("step_0.75")["trunc"]
    assert [K.case(n)["step_factor"] for n in ("step_0.25", "step_0.75", "step_2.0")] == [0.25, 0.75, 2.0]
    vs = K.case("outside")["vs"]
    assert len(set(vs.tolist())) == 3 and K.dims_of(K.case("outside")["vol"]) == (24, 20, 18)
