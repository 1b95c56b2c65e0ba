"""Exact point-to-mesh distances on the GPU (sobfu_amd/csrc/mesh_distance_kernels.hip): dist, tri and closest against the numpy restatement
tests/mesh_distance_reference.py bit for bit -- whatever the grid's cells, the mode and the ring cap -- on a soup with every degenerate
shape, on two triangles spanning a fine grid and on a marching-cubes mesh; max_dist; the edges; compare_meshes' statistics."""
import numpy as np
import pytest

import mesh_distance_reference as MD

pytestmark = pytest.mark.gpu
MIN_BOUND = 1e-6  # the per-point bound tests/test_mesh_distance_cpu.py asserts for float32 against float64, in units of L


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what=""):
    for name, g, w in zip(("dist", "tri", "closest"), got, want):
        g = _cpu(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(len(w), -1).any(1))[0]
        assert bad.size == 0, "%s %s differs at %d points, first %d: got %r want %r" % (what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.fixture(scope="module")
def soup():
    p, v, f, lo, hi = MD.indexed_soup()
    return dict(p=p, v=v, f=f, lo=lo, hi=hi, ref=MD.brute_force(p, v, f))


CELLS = {"1x1x1": (10.0, [1, 1, 1]), "5x4x3": (0.55, [5, 4, 3]), "auto": (None, [7, 6, 5])}


@pytest.mark.parametrize("cells", list(CELLS))
def test_soup_equals_the_restatement_on_every_path(soup, cells):
    """700 triangles (all degenerate shapes, shared and unreferenced vertices) x 3000 points (a tenth beyond the box, 150 at distance 0).
    ring_cap=1: a point is finished by brute force unless shells 0 and 1 settle it, i.e. its distance + margin <= h, or cover the grid."""
    from sobfu_amd import ops

    cell, dims = CELLS[cells]
    p, v, f = _gpu(soup["p"]), _gpu(soup["v"]), _gpu(soup["f"])
    g = ops.TriangleGrid(v, f, cell=cell)
    assert list(g.dims) == dims and g.references >= len(soup["f"])
    assert (soup["ref"][0] == 0).sum() >= 50 and np.all(soup["ref"][1] >= 0)
    n = len(soup["p"])
    for mode, cap in (("grid", None), ("grid", 1), ("brute", None), ("auto", None)):
        _same(g.query(p, closest=True, mode=mode, ring_cap=cap), soup["ref"], "%s %s cap %s" % (cells, mode, cap))
        un = g.unresolved()
        print("%s: mode %s ring_cap %s: %d of %d points finished by brute force (%d references, h = %.4g)" % (cells, mode, cap, un, n, g.references, g.h))
        if mode == "brute":
            assert un == 0
        elif cells == "1x1x1":
            assert un == 0  # shell 0 is the whole grid
        elif cap == 1:
            assert 0.05 * n <= un <= 0.95 * n
        else:
            assert un <= 0.05 * n  # the default cap of 8 shells covers these grids from almost every cell
    d, t = g.query(p)  # without the closest points
    assert np.array_equal(_bits(_cpu(d)), _bits(soup["ref"][0])) and np.array_equal(_cpu(t), soup["ref"][1])


def test_large_triangles_on_a_fine_grid():
    """two triangles spanning the whole box, referenced from every cell of a 32^3 grid their boxes overlap (the first build attempt's
    room for references is too small: the build asks for more)"""
    from sobfu_amd import ops

    rng = np.random.default_rng(4)
    v = np.array([[0, 0, 0, 1], [1, 0, 1, 1], [0, 1, 1, 1], [1, 1, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    p = np.ones((2000, 4), np.float32)
    p[:, :3] = rng.uniform(-0.2, 1.2, (2000, 3))
    ref = MD.brute_force(p, v, f)
    g = ops.TriangleGrid(_gpu(v), _gpu(f), cell=1.0 / 32)
    assert list(g.dims) == [32, 32, 32] and g.references > 8 * 2 + 1024
    for mode, cap in (("grid", None), ("grid", 1), ("brute", None)):
        _same(g.query(_gpu(p), closest=True, mode=mode, ring_cap=cap), ref, "%s cap %s" % (mode, cap))
    assert len(set(ref[1])) == 2


def test_a_marching_cubes_mesh():
    """The indexed mesh of a sphere (r = 0.1 m in a 40 x 33 x 29 volume of 1 cm voxels).  Its own vertices are at distance 0 within the
    fp32 bound.  Moved t = 3 mm along their normals, p = v + t n: the mesh is closed and star-shaped about the centre c and lies in the
    shell rho_min <= |x - c| <= rho_max (rho_max: the farthest vertex, faces being convex combinations; rho_min: the float64 distance from
    c to the mesh), so a point at R = |p - c| > rho_max is at least R - rho_max from it, and at most R - rho_min (the mesh point on
    the ray from c through p)."""
    from sobfu_amd import ops

    dims, vs = (40, 33, 29), 0.01
    c = np.array([0.2, 0.165, 0.145])
    vol = ops.new_volume(dims)
    ops.init_sphere(vol, (vs,) * 3, 5 * vs, 2 * vs, tuple(c), 0.1)
    v, nrm, f = ops.marching_cubes_indexed(vol, tuple(d * vs for d in dims))
    hv, hn, hf = _cpu(v), _cpu(nrm), _cpu(f)
    assert len(hv) > 1000 and len(hf) > 2000
    L = float(np.abs(hv[:, :3]).max())
    g = ops.TriangleGrid(v, f)
    own = g.query(v, closest=True)
    _same(own, MD.brute_force(hv, hv, hf), "own vertices")
    d_own = _cpu(own[0])
    print("marching-cubes sphere: %d vertices, %d faces, dims %s; own vertices max dist %.3g (bound %.3g)" % (len(hv), len(hf), list(g.dims), d_own.max(), MIN_BOUND * L))
    assert d_own.max() <= MIN_BOUND * L
    t = np.float32(0.003)
    moved = hv.copy()
    moved[:, :3] = hv[:, :3] + t * hn[:, :3]
    got = g.query(_gpu(moved), closest=True)
    _same(got, MD.brute_force(moved, hv, hf), "moved vertices")
    cf = c * np.array([1.0, -1.0, -1.0])  # the centre in the mesh's frame (x, -y, -z)
    rho_max = np.linalg.norm(hv[:, :3].astype(np.float64) - cf, axis=1).max()
    centre = np.ones((1, 4))
    centre[0, :3] = cf
    rho_min = float(MD.brute_force(centre, hv, hf, dtype=np.float64)[0][0])
    R = np.linalg.norm(moved[:, :3].astype(np.float64) - cf, axis=1)
    d = _cpu(got[0]).astype(np.float64)
    assert R.min() > rho_max and 0.09 < rho_min <= rho_max < 0.11
    bound = np.maximum(np.abs(R - rho_max - float(t)), np.abs(R - rho_min - float(t))) + MIN_BOUND * L
    print("moved 3 mm: |dist - 3 mm| max %.3g m, faceting bound max %.3g m (rho in [%.6f, %.6f])" % (np.abs(d - float(t)).max(), bound.max(), rho_min, rho_max))
    assert np.all(d >= R - rho_max - MIN_BOUND * L) and np.all(d <= R - rho_min + MIN_BOUND * L)
    assert np.all(np.abs(d - float(t)) <= bound)


def test_max_dist(soup):
    from sobfu_amd import ops

    p, v, f = _gpu(soup["p"]), _gpu(soup["v"]), _gpu(soup["f"])
    limit = float(np.median(soup["ref"][0]))
    want = MD.brute_force(soup["p"], soup["v"], soup["f"], max_dist=limit)
    far = soup["ref"][0] > np.float32(limit)
    assert 0.3 * len(far) < far.sum() < 0.7 * len(far)  # both sides of the threshold
    assert np.all(np.isinf(want[0][far])) and np.all(want[1][far] == -1) and np.all(want[2][far] == 0)
    assert np.array_equal(_bits(want[0][~far]), _bits(soup["ref"][0][~far]))
    for cell in (None, 0.55, 0.05):
        g = ops.TriangleGrid(v, f, cell=cell)
        for mode, cap in (("grid", None), ("grid", 1), ("brute", None)):
            _same(g.query(p, max_dist=limit, closest=True, mode=mode, ring_cap=cap), want, "max_dist cell %s %s cap %s" % (cell, mode, cap))
    g = ops.TriangleGrid(v, f)
    for unlimited in (None, 0.0, -1.0, float("inf")):
        _same(g.query(p, max_dist=unlimited, closest=True), soup["ref"], "max_dist %r" % (unlimited,))
    _same(ops.mesh_distance(p, v, f, max_dist=limit, closest=True), want, "mesh_distance")


def test_edges(soup):
    import torch

    from sobfu_amd import ops
    from sobfu_amd._lib import HipError

    p, v, f = _gpu(soup["p"][:500]), _gpu(soup["v"]), _gpu(soup["f"])
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    for verts in (v, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):  # no triangles, with and without vertices
        for mode in ("auto", "grid", "brute"):
            d, t, q = ops.TriangleGrid(verts, none).query(p, closest=True, mode=mode)
            assert np.all(np.isposinf(_cpu(d))) and np.all(_cpu(t) == -1) and not _cpu(q).any()
    g = ops.TriangleGrid(v, f)
    d, t, q = g.query(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), closest=True)  # no points
    assert d.shape == (0,) and t.shape == (0,) and q.shape == (0, 4)
    one_v = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 2, 0, 1]], np.float32)  # one triangle, one point
    one_p = np.array([[0.5, 0.5, 3, 1]], np.float32)
    for mode in ("auto", "grid", "brute"):
        d, t, q = ops.mesh_distance(_gpu(one_p), _gpu(one_v), _gpu(np.array([[0, 1, 2]], np.int32)), closest=True, mode=mode)
        assert _cpu(d)[0] == 3 and _cpu(t)[0] == 0 and np.array_equal(_cpu(q)[0], [0.5, 0.5, 0, 1])
    # a repeated call gives the same bits and leaves its inputs as they were
    first = [_cpu(x).copy() for x in g.query(p, closest=True, mode="grid", ring_cap=1)]
    again = [_cpu(x) for x in g.query(p, closest=True, mode="grid", ring_cap=1)]
    rebuilt = [_cpu(x) for x in ops.TriangleGrid(v, f).query(p, closest=True, mode="grid", ring_cap=1)]
    for a, b, c in zip(first, again, rebuilt):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert np.array_equal(_bits(_cpu(p)), _bits(soup["p"][:500])) and np.array_equal(_bits(_cpu(v)), _bits(soup["v"]))
    assert np.array_equal(_cpu(f), soup["f"])
    # a face index out of range, a NaN corner: the build refuses, no grid exists to launch through
    for bad_f, bad_v in ((len(soup["v"]), None), (-1, None), (None, float("nan")), (None, float("inf"))):
        hv, hf = soup["v"].copy(), soup["f"].copy()
        if bad_f is not None:
            hf[333, 2] = bad_f
        else:
            hv[hf[333, 1], 1] = bad_v
        with pytest.raises(HipError) as e:
            ops.TriangleGrid(_gpu(hv), _gpu(hf))
        assert "(code -1)" in str(e.value)
    hv = soup["v"].copy()
    unused = np.setdiff1d(np.arange(len(hv)), soup["f"].ravel())
    assert unused.size > 100
    hv[unused[:5], 0] = np.nan  # a vertex no face uses may hold anything
    _same(ops.TriangleGrid(_gpu(hv), f).query(p, closest=True), [x[:500] for x in soup["ref"]], "unused NaN vertices")
    with pytest.raises(ValueError):
        g.query(p, mode="fast")


def test_compare_meshes_statistics():
    """sobfu_amd.evaluate.compare_meshes against numpy float64 statistics of the restatement's distances, to relative 1e-12"""
    from sobfu_amd.evaluate import compare_meshes

    av, af = MD.icosphere(0.1, 3, (0.01, -0.02, 0.5))
    bv, bf = MD.icosphere(0.11, 2, (0.0, 0.0, 0.5))
    for limit in (None, 0.012):
        r, d_ab, d_ba = compare_meshes(_gpu(av), _gpu(af), bv, bf, max_dist=limit, return_distances=True)
        want = {"a_to_b": MD.brute_force(av, bv, bf, max_dist=limit)[0], "b_to_a": MD.brute_force(bv, av, af, max_dist=limit)[0]}
        assert np.array_equal(_bits(_cpu(d_ab)), _bits(want["a_to_b"])) and np.array_equal(_bits(_cpu(d_ba)), _bits(want["b_to_a"]))
        for side, d in want.items():
            fin = d[np.isfinite(d)].astype(np.float64)
            assert r[side]["n"] == len(d) and r[side]["within"] == len(fin) and (limit is None) == (len(fin) == len(d)) and len(fin) > 10
            for key, val in (("mean", fin.mean()), ("rms", np.sqrt((fin * fin).mean())), ("median", np.median(fin)), ("max", fin.max())):
                assert abs(r[side][key] - val) <= 1e-12 * abs(val), (side, key)
        assert abs(r["chamfer"] - 0.5 * (r["a_to_b"]["mean"] + r["b_to_a"]["mean"])) <= 1e-12 * r["chamfer"]
        assert r["hausdorff"] == max(r["a_to_b"]["max"], r["b_to_a"]["max"])
