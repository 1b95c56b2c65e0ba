"""Rays against triangle meshes on the GPU (sobfu_amd/csrc/mesh_ray_kernels.hip): t, tri, barycentrics and side against the numpy
restatement tests/mesh_ray_reference.py bit for bit -- whatever the grid's cells and the mode -- on a soup with every degenerate shape, on
rays through the corners, edges and planes of the cell lattice, on sheets spanning a fine grid, at the edges of the interface and on a
closed icosphere."""
import numpy as np
import pytest

import mesh_ray_reference as MR

pytestmark = pytest.mark.gpu
MODES = ("grid", "brute", "auto")
CELLS = {"1x1x1": (10.0, [1, 1, 1]), "5x4x3": (0.55, [5, 4, 3]), "auto": (None, [7, 6, 5])}  # as in tests/test_gpu_mesh_distance.py


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, what=""):
    for name, g, w in zip(("t", "tri", "bary", "side"), got, want):
        g = _cpu(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.nonzero((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).reshape(len(w), -1).any(1))[0]
        assert bad.size == 0, "%s %s differs at %d rays, first %d: got %r want %r" % (what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


def _cast(g, o, d, mode, **kw):
    return g.raycast(_gpu(o), _gpu(d), mode=mode, bary=True, side=True, **kw)


@pytest.fixture(scope="module")
def soup():
    _, v, f, lo, hi = MR.indexed_soup()
    o, d = MR.soup_rays(v, f, lo, hi)
    return dict(v=v, f=f, o=o, d=d, ref=MR.brute_force(o, d, v, f))


@pytest.mark.parametrize("cells", list(CELLS))
def test_soup_equals_the_restatement_on_every_path(soup, cells):
    """700 triangles (all degenerate shapes, shared and unreferenced vertices) x 4096 rays: a third from outside the box, a third starting
    inside, a tenth that miss the box, the rest aimed at vertices and edge midpoints"""
    from sobfu_amd import ops

    cell, dims = CELLS[cells]
    g = ops.TriangleGrid(_gpu(soup["v"]), _gpu(soup["f"]), cell=cell)
    assert list(g.dims) == dims
    hits = int((soup["ref"][1] >= 0).sum())
    assert 0.3 * len(soup["o"]) < hits < 0.9 * len(soup["o"])
    for mode in MODES:
        _same(_cast(g, soup["o"], soup["d"], mode), soup["ref"], "%s %s" % (cells, mode))
    t, tri = g.raycast(_gpu(soup["o"]), _gpu(soup["d"]))  # without the optional outputs
    _same((t, tri), soup["ref"][:2], "t and tri only")
    limit = float(np.median(soup["ref"][0][np.isfinite(soup["ref"][0])]))
    want = MR.brute_force(soup["o"], soup["d"], soup["v"], soup["f"], 0.25 * limit, limit)
    assert (want[1] != soup["ref"][1]).sum() > 100
    for mode in MODES:
        _same(_cast(g, soup["o"], soup["d"], mode, t_min=0.25 * limit, t_max=limit), want, "%s %s limited" % (cells, mode))


def _small_triangle(c, s=0.02):
    """a triangle around c, perpendicular to (1, 1, 1), within s of c on every axis"""
    c = np.asarray(c, np.float64)
    return [c + s * np.array(e) for e in ((1, -0.5, -0.5), (-0.5, 1, -0.5), (-0.5, -0.5, 1))]


def _lattice_mesh():
    """Box [0, 1]^3 (two tiny anchor triangles at its corners), cell 0.25: the lattice planes k / 4 are exact in float32.  Triangles:
    2 just beyond the lattice corner (0.5, 0.5, 0.5) in cell (2, 2, 2) and only there, diagonally opposite for a ray along (1, 1, 1), 3
    likewise in cell (1, 1, 2) for a ray along (-1, -1, 1), 4 beyond the midpoint (0.5, 0.5, 0.625) of a lattice edge, in cell (2, 2, 2),
    5 and 6 in the planes x = 0.6 and x = 0.7 with
    an edge ON the lattice plane y = 0.5, from either side, then 120 that straddle the planes around random lattice corners."""
    rng = np.random.default_rng(12)
    tris = [[(0, 0, 0), (0.01, 0, 0), (0, 0.01, 0)], [(1, 1, 1), (0.99, 1, 1), (1, 0.99, 1)],
            _small_triangle((0.53, 0.53, 0.53)), _small_triangle((0.47, 0.47, 0.53)), _small_triangle((0.53, 0.53, 0.625)),
            [(0.6, 0.5, 0.55), (0.6, 0.5, 0.65), (0.6, 0.53, 0.6)], [(0.7, 0.5, 0.55), (0.7, 0.5, 0.65), (0.7, 0.47, 0.6)]]
    while len(tris) < 127:
        corner = rng.integers(1, 4, 3) / 4.0
        if corner[0] == corner[1] or corner[1] == 0.5:  # clear of the planes x = y and y = 0.5, where the rays aimed by hand run
            continue
        tris.append(_small_triangle(corner + 0.03 * rng.choice([-1.0, 1.0], 3), 0.05))
    tris = np.asarray(tris, np.float64)
    v = np.ones((3 * len(tris), 4), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    return v, np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def _lattice_rays():
    rays = []
    for o in ((0.25, 0.25, 0.25), (0.125, 0.125, 0.125), (0.375, 0.375, 0.375)):  # through the corner (0.5, 0.5, 0.5) exactly
        rays.append((o, (1, 1, 1)))
        rays.append((o, (0.5, 0.5, 0.5)))
    rays.append(((0.75, 0.75, 0.25), (-1, -1, 1)))
    rays.append(((1.0, 1.0, 0.0), (-2, -2, 2)))
    one = np.float32(1)
    for k in range(3):  # ... and a last bit to either side of it
        for nudged in (np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))):
            d = [1.0, 1.0, 1.0]
            d[k] = float(nudged)
            rays.append(((0.25, 0.25, 0.25), tuple(d)))
            rays.append(((0.75, 0.75, 0.25), (-d[0], -d[1], d[2])))
    for o, d in (((0.25, 0.25, 0.625), (1, 1, 0)), ((0.75, 0.75, 0.625), (-1, -1, 0)), ((-0.25, -0.25, 0.625), (2, 2, 0))):  # a lattice edge's midpoint
        rays.append((o, d))
    for o, d in (((0.1, 0.5, 0.6), (1, 0, 0)), ((0.9, 0.5, 0.6), (-1, 0, 0)), ((-1, 0.5, 0.6), (3, 0, 0)), ((0.35, 0.5, 0.35), (1, 0, 1)),
                 ((0.1, 0.5, 0.575), (1, 0, 0.05)), ((0.9, 0.5, 0.625), (-1, 0, -0.05)), ((0.6, 0.5, 0.1), (0, 0, 1)), ((0.5, 0.5, -1), (0, 0, 1)),
                 ((0.5, 0.5, 2), (0, 0, -1)), ((-1, 0.5, 0.5), (1, 0, 0)), ((0.5, 2, 0.5), (0, -1, 0))):  # along lattice planes and edges
        rays.append((o, d))
    for c in ((0.53, 0.53, 0.53), (0.47, 0.47, 0.47), (0.53, 0.53, 0.625)):  # parallel to each axis, both ways, through the triangles
        for k in range(3):
            for s in (1.0, -1.0):
                o, d = list(c), [0.0, 0.0, 0.0]
                o[k], d[k] = c[k] - 2 * s, s
                rays.append((tuple(o), tuple(d)))
    rng = np.random.default_rng(13)
    for _ in range(1500):  # from lattice point to lattice point, some outside the box: exact corner and edge crossings throughout
        o, tgt = rng.integers(-1, 6, 3) / 4.0, rng.integers(0, 5, 3) / 4.0
        if np.any(o != tgt):
            rays.append((tuple(o), tuple((tgt - o) * rng.choice([0.5, 1.0, 2.0]))))
    o, d = np.ones((len(rays), 4), np.float32), np.zeros((len(rays), 4), np.float32)
    o[:, :3], d[:, :3] = [r[0] for r in rays], [r[1] for r in rays]
    return o, d


def test_rays_through_the_lattice():
    """the smallest case at which a cell walk's stepping order can lose a cell: rays that meet two or three lattice planes at once"""
    from sobfu_amd import ops

    v, f = _lattice_mesh()
    o, d = _lattice_rays()
    g = ops.TriangleGrid(_gpu(v), _gpu(f), cell=0.25)
    assert list(g.dims) == [4, 4, 4] and np.array_equal(g.origin, [0, 0, 0]) and g.h == 0.25
    tri = v[f][:, :, :3]
    for k, cell in ((2, (2, 2, 2)), (3, (1, 1, 2)), (4, (2, 2, 2))):  # each of them lies in one cell only
        assert np.all(np.floor(tri[k] / 0.25) == cell)
    ref = MR.brute_force(o, d, v, f)
    assert list(ref[1][:8]) == [2, 2, 2, 2, 2, 2, 3, 3]  # through the corner: the triangle beyond it
    assert list(ref[1][8:20]) == [2, 3] * 6 and np.all(ref[1][20:23] == 4) and list(ref[1][23:27]) == [5, 6, 5, 5]
    hits = int((ref[1] >= 0).sum())
    print("lattice: %d rays, %d hit" % (len(o), hits))
    assert hits > 200
    for mode in MODES:
        _same(_cast(g, o, d, mode), ref, "lattice %s" % mode)
    fine = ops.TriangleGrid(_gpu(v), _gpu(f), cell=1.0 / 16)
    assert list(fine.dims) == [16, 16, 16]
    _same(_cast(fine, o, d, "grid"), ref, "lattice, 16 cells")


def test_early_stop_and_the_tie_rule():
    """two parallel sheets spanning a 32 x 32 x 13 grid, the nearer one with the HIGHER triangle indices: the walk may not stop at the
    first triangle it meets in a cell; then a coplanar duplicate of the nearer sheet with lower indices: the lowest index wins"""
    from sobfu_amd import ops

    def sheet(z):
        return [[(0, 0, z), (1, 0, z), (1, 1, z)], [(0, 0, z), (1, 1, z), (0, 1, z)]]

    rng = np.random.default_rng(21)
    n = 1200
    o, d = np.ones((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o[:, :3] = rng.uniform([-0.5, -0.5, -1.0], [1.5, 1.5, -0.2], (n, 3))
    d[:, :3] = rng.uniform([0.05, 0.05, 0.3], [0.95, 0.95, 0.3], (n, 3)) - o[:, :3]  # through the nearer sheet, z = 0.3, well inside it
    d[:, :3] *= rng.uniform(0.5, 2.0, (n, 1))
    o[n // 2:, :3] += d[n // 2:, :3] * rng.uniform(0.5, 1.5, (n - n // 2, 1))  # the second half starts around the nearer sheet, inside the box
    for tris, nearer in ((sheet(0.7) + sheet(0.3), (2, 3)), (sheet(0.7) + sheet(0.3) + sheet(0.3), (2, 3))):
        v = np.ones((3 * len(tris), 4), np.float32)
        v[:, :3] = np.asarray(tris, np.float64).reshape(-1, 3)
        f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
        ref = MR.brute_force(o, d, v, f)
        first = ref[1][:n // 2]
        assert np.all(np.isin(first, nearer)) and set(first) == set(nearer)
        g = ops.TriangleGrid(_gpu(v), _gpu(f), cell=1.0 / 32)
        assert list(g.dims) == [32, 32, 13] and g.references > 1000
        for mode in ("grid", "brute"):
            _same(_cast(g, o, d, mode), ref, "%d sheets %s" % (len(tris) // 2, mode))


def test_edges(soup):
    import torch

    from sobfu_amd import ops

    o, d = soup["o"][:600], soup["d"][:600]
    v, f = _gpu(soup["v"]), _gpu(soup["f"])
    miss = (np.full(600, np.inf, np.float32), np.full(600, -1, np.int32), np.zeros((600, 2), np.float32), np.zeros(600, np.int8))
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    for verts in (v, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):  # no triangles, with and without vertices
        for mode in MODES:
            _same(_cast(ops.TriangleGrid(verts, none), o, d, mode), miss, "no triangles %s" % mode)
    g = ops.TriangleGrid(v, f)
    empty = torch.zeros((0, 4), dtype=torch.float32, device="cuda")
    t, tri, bary, side = g.raycast(empty, empty, bary=True, side=True)  # no rays
    assert t.shape == (0,) and tri.shape == (0,) and bary.shape == (0, 2) and side.shape == (0,)
    # a repeated call and a rebuilt grid give the same bits and leave the inputs as they were
    go, gd = _gpu(o), _gpu(d)
    first = [_cpu(x).copy() for x in g.raycast(go, gd, mode="grid", bary=True, side=True)]
    again = [_cpu(x) for x in g.raycast(go, gd, mode="grid", bary=True, side=True)]
    rebuilt = [_cpu(x) for x in ops.TriangleGrid(v, f).raycast(go, gd, mode="grid", bary=True, side=True)]
    for a, b, c in zip(first, again, rebuilt):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert _cpu(go).tobytes() == o.tobytes() and _cpu(gd).tobytes() == d.tobytes() and _cpu(v).tobytes() == soup["v"].tobytes()
    # zero, NaN and Inf directions and origins are misses, between rays that hit
    bo, bd = o.copy(), d.copy()
    bd[0, :3], bd[1, 2], bd[2, 0], bd[3, 1], bo[4, 0], bo[5, 2] = 0, np.nan, np.inf, -np.inf, np.nan, np.inf
    want = MR.brute_force(bo, bd, soup["v"], soup["f"])
    assert np.all(want[1][:6] == -1) and (want[1][6:] >= 0).sum() > 100
    for mode in MODES:
        _same(_cast(g, bo, bd, mode), want, "bad rays %s" % mode)
    # t_min / t_max cut exactly at a hit: t == t_max is a hit, t == t_min is not
    one_v = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 2, 0, 1]], np.float32)
    one = ops.TriangleGrid(_gpu(one_v), _gpu(np.array([[0, 1, 2]], np.int32)))
    ro, rd = _gpu(np.array([[0.5, 0.25, 3, 1]], np.float32)), _gpu(np.array([[0, 0, -1, 0]], np.float32))
    below = float(np.nextafter(np.float32(3), np.float32(0)))
    for mode in MODES:
        for kw, hit in ((dict(), True), (dict(t_max=3.0), True), (dict(t_max=below), False), (dict(t_min=3.0), False), (dict(t_min=below), True),
                        (dict(t_max=0.0), True), (dict(t_max=-1.0), True), (dict(t_max=float("inf")), True)):
            t, tri, bary, side = (_cpu(x) for x in one.raycast(ro, rd, mode=mode, bary=True, side=True, **kw))
            assert (t[0], tri[0], tuple(bary[0]), side[0]) == ((3.0, 0, (0.25, 0.125), 1) if hit else (np.inf, -1, (0.0, 0.0), 0)), (mode, kw)
    # a workspace that is not marked as built answers "miss" for every ray
    g.workspace.zero_()
    for mode in MODES:
        _same(_cast(g, o, d, mode), miss, "unbuilt %s" % mode)
    with pytest.raises(ValueError):
        g.raycast(go, gd, mode="fast")


def test_watertight_on_a_closed_icosphere():
    """the rays of tests/test_mesh_ray_cpu.py through every vertex, every edge midpoint and 2000 random points on edges of a closed
    icosphere of 320 faces, from outside toward the centre: all hit, on the outside, in front of the centre (t = 1)"""
    from sobfu_amd import ops

    v, f = MR.icosphere(0.1, 2, (0.01, -0.02, 0.5))
    o, d = MR.watertight_rays(v, f)
    for cell in (None, 0.012):
        g = ops.TriangleGrid(_gpu(v), _gpu(f), cell=cell)
        for t_max in (None, 1.0):
            got = _cast(g, o, d, "grid", t_max=t_max)
            t, tri, side = _cpu(got[0]), _cpu(got[1]), _cpu(got[3])
            assert np.all(tri >= 0) and np.all(side == 1) and np.all(t < 1)
            _same(got, MR.brute_force(o, d, v, f, 0.0, t_max), "icosphere cell %s" % cell)
