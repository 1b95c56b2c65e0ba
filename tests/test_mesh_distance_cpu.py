"""Exact point-to-mesh distances, on the CPU: the C ABI's entry points (exported, ABI version unchanged, argument checks before any device
call), the grid plan against goldens, and the numpy restatement tests/mesh_distance_reference.py of the point-triangle rule
(sobfu_amd/csrc/sobfu_mesh_distance.hpp) against closed forms, against its float64 twin and against the header itself as a host compiler
takes it.

Measured here, restatement vs float64 twin, L = the largest absolute coordinate (seeds below):
  soup   3000 triangles (edge scale 0.1, 300 exact-midpoint slivers, every degenerate shape) x 1500 points: per pair 3.0e-7 L, per-point
         minimum 5.4e-8 L, no argmin differs
  shell  3000 triangles of 5 mm on a 0.3 m sphere x 1500 points within 3 mm: per pair 7.7e-8 L, per-point minimum 4.3e-8 L
The bounds asserted are the issue's: 1e-4 L per pair (the margin of the grid query's stop rule, kMeshMargin, must be at least this),
1e-6 L for the per-point minimum."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_distance_reference as MD

F3, F6, I3 = C.c_float * 3, C.c_float * 6, C.c_int * 3
A, B, D, E, G = (C.c_void_p(4096 * k) for k in range(1, 6))  # 16-byte aligned addresses that are never dereferenced
PAIR_BOUND, MIN_BOUND = 1e-4, 1e-6


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    L = _lib.lib()
    L.sobfu_hip_mesh_grid_workspace_bytes.restype = C.c_size_t
    return L


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_mesh_grid_plan", "sobfu_hip_mesh_grid_workspace_bytes", "sobfu_hip_mesh_grid_build", "sobfu_hip_mesh_distance",
              "sobfu_hip_mesh_distance_unresolved"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


# ---- argument checks: every case is refused (or n = 0) before any device call ---------------------------------------------------------
def _build(lib, **kw):
    a = dict(v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), ws=D, ws_bytes=1 << 20, max_refs=64, refs=C.byref(C.c_int(0)))
    a.update(kw)
    return lib.sobfu_hip_mesh_grid_build(a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"], a["ws"],
                                         C.c_size_t(a["ws_bytes"]), a["max_refs"], a["refs"], None)


def _distance(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), p=E, n=4, max_dist=0.0, mode=0, cap=0,
             dist=G, tri=C.c_void_p(G.value + 4096), closest=None, un=C.c_void_p(G.value + 8192))
    a.update(kw)
    return lib.sobfu_hip_mesh_distance(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                       a["p"], a["n"], C.c_float(a["max_dist"]), a["mode"], a["cap"], a["dist"], a["tri"], a["closest"], a["un"], None)


GRID_BAD = [dict(ws=None), dict(ws=C.c_void_p(4104)), dict(ws_bytes=16), dict(origin=None), dict(dims=None), dict(h=0.0), dict(h=-1.0),
            dict(h=float("nan")), dict(h=float("inf")), dict(origin=F3(0, float("nan"), 0)), dict(origin=F3(float("inf"), 0, 0)), dict(dims=I3(0, 2, 2)),
            dict(dims=I3(2, -1, 2)), dict(dims=I3(2, 2, 129)), dict(v=None), dict(f=None), dict(v=C.c_void_p(4100)), dict(f=C.c_void_p(8194)),
            dict(nv=-1), dict(nt=-1)]


@pytest.mark.parametrize("kw", GRID_BAD + [dict(refs=None), dict(max_refs=-1), dict(ws_bytes=4 * (16 + 2 * 9 + 2 + 64) - 1)])
def test_build_bad_arguments(lib, kw):
    assert _build(lib, **kw) == -1


@pytest.mark.parametrize("kw", GRID_BAD + [dict(p=None), dict(dist=None), dict(tri=None), dict(un=None), dict(n=-1), dict(p=C.c_void_p(E.value + 8)),
                                           dict(dist=C.c_void_p(G.value + 2)), dict(tri=C.c_void_p(G.value + 4097)), dict(closest=C.c_void_p(G.value + 8)),
                                           dict(un=C.c_void_p(G.value + 8193)), dict(max_dist=float("nan")), dict(mode=-1), dict(mode=3), dict(cap=-1)])
def test_distance_bad_arguments(lib, kw):
    assert _distance(lib, **kw) == -1


def test_no_points_is_a_success_without_a_device(lib):
    assert _distance(lib, n=0) == 0 and _distance(lib, n=0, closest=A, max_dist=float("inf"), mode=2, un=None) == 0
    assert _distance(lib, n=0, ws=None) == -1 and _distance(lib, n=0, dist=None) == -1  # the checks come first
    assert lib.sobfu_hip_mesh_distance_unresolved(None, C.byref(C.c_int(0)), None) == -1
    assert lib.sobfu_hip_mesh_distance_unresolved(D, None, None) == -1
    assert lib.sobfu_hip_mesh_grid_workspace_bytes(I3(2, 2, 2), 64) == 4 * (16 + 2 * 9 + 2 + 64)
    assert lib.sobfu_hip_mesh_grid_workspace_bytes(I3(0, 2, 2), 64) == 0 and lib.sobfu_hip_mesh_grid_workspace_bytes(I3(2, 2, 2), -1) == 0


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def _plan(lib, bbox, n, cell=0.0):
    origin, h, dims = F3(), C.c_float(0), I3()
    rc = lib.sobfu_hip_mesh_grid_plan(F6(*bbox), n, C.c_float(cell), origin, C.byref(h), dims)
    return rc, np.array(list(origin), np.float32), np.float32(h.value), list(dims)


@pytest.mark.parametrize("bbox, n, cell, h, dims", [
    ((0, 0, 0, 1, 0.5, 0.25), 1600, 0.0, 0.1, [10, 5, 3]),      # default: ceil(sqrt(1600) / 4) = 10 cells along x
    ((0, 0, 0, 1, 0.5, 0.25), 1600, 0.3, 0.3, [4, 2, 1]),       # a given cell
    ((-1, -1, 2, 1, 1, 2), 64, 0.0, 1.0, [2, 2, 1]),            # a flat box: one cell across
    ((3, 4, 5, 3, 4, 5), 100, 0.0, 1.0, [1, 1, 1]),             # a point: one cell of edge 1 ...
    ((3, 4, 5, 3, 4, 5), 100, 0.25, 0.25, [1, 1, 1]),           # ... or of the given edge
    ((0, 0, 0, 2, 2, 2), 0, 0.0, 2.0, [1, 1, 1]),               # n = 0
    ((0, 0, 0, 2, 2, 2), 1, 0.0, 2.0, [1, 1, 1]),               # n = 1
    ((0, 0, 0, 2, 2, 1), 1000000, 0.0, 2.0 / 128, [128, 128, 64]),  # n = 10^6: 250 cells, capped at 128
    ((0, 0, 0, 2, 2, 1), 10, 1e-6, 2.0 / 128, [128, 128, 64]),  # a cell that would need more than 128
])
def test_plan_goldens(lib, bbox, n, cell, h, dims):
    rc, origin, got_h, got_dims = _plan(lib, bbox, n, cell)
    assert rc == 0 and got_dims == dims and got_h == np.float32(h)
    assert np.array_equal(origin, np.array(bbox[:3], np.float32))
    o2, h2, d2 = MD.grid_plan(bbox, n, cell)
    assert h2 == got_h and list(d2) == dims


def test_plan_covers_the_box_and_stays_within_128(lib):
    rng = np.random.default_rng(5)
    for _ in range(300):
        lo = rng.uniform(-10, 10, 3).astype(np.float32)
        ext = (rng.uniform(0, 1, 3) ** 4 * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32) * (rng.uniform(size=3) > 0.15)
        bbox = np.concatenate([lo, (lo + ext).astype(np.float32)])
        n = int(rng.choice([0, 1, 7, 700, 175000, 10 ** 6, 2 ** 31 - 1]))
        cell = float(rng.choice([0.0, 0.0, 1e-4, 0.05, 3.0]))
        rc, origin, h, dims = _plan(lib, bbox, n, cell)
        assert rc == 0 and all(1 <= d <= 128 for d in dims)
        real = bbox[3:].astype(np.float64) - bbox[:3].astype(np.float64)
        assert np.all(np.array(dims) * float(h) >= real), (bbox, n, cell, h, dims)
        o2, h2, d2 = MD.grid_plan(bbox, n, cell)
        assert h2 == h and list(d2) == dims


@pytest.mark.parametrize("bbox, n, cell", [((0, 0, 0, 1, 1, float("nan")), 4, 0.0), ((0, 0, 0, float("inf"), 1, 1), 4, 0.0), ((1, 0, 0, 0, 1, 1), 4, 0.0),
                                           ((0, 0, 0, 1, 1, 1), -1, 0.0), ((0, 0, 0, 1, 1, 1), 4, -0.5), ((0, 0, 0, 1, 1, 1), 4, float("nan")),
                                           ((-3e38, 0, 0, 3e38, 1, 1), 4, 0.0)])
def test_plan_refusals(lib, bbox, n, cell):
    assert _plan(lib, bbox, n, cell)[0] == -1


# ---- the restatement against closed forms -------------------------------------------------------------------------------------------------
TA, TB, TC = (0, 0, 0), (2, 0, 0), (0, 2, 0)


@pytest.mark.parametrize("p, q, d2", [
    ((-1, -1, 1), (0, 0, 0), 3),          # vertex a
    ((3, -1, 0), (2, 0, 0), 2),           # vertex b
    ((-1, 3, 0), (0, 2, 0), 2),           # vertex c
    ((1, -1, 2), (1, 0, 0), 5),           # edge ab
    ((-1, 1, 2), (0, 1, 0), 5),           # edge ac
    ((2, 2, 1), (1, 1, 0), 3),            # edge bc
    ((0.5, 0.5, 3), (0.5, 0.5, 0), 9),    # interior
    ((2, 0, 0), (2, 0, 0), 0),            # on a vertex
    ((1, 0, 0), (1, 0, 0), 0),            # on an edge
    ((0.5, 0.75, 0), (0.5, 0.75, 0), 0),  # in the plane, inside
])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_case_per_region(p, q, d2, dtype):
    for a, b, c in ((TA, TB, TC), (TB, TC, TA), (TC, TA, TB), (TA, TC, TB)):  # every corner order: the answer is the triangle's
        gq, gd = MD.closest_on_triangle(p, a, b, c, dtype)
        assert np.array_equal(gq, np.array(q, dtype)) and gd == dtype(d2), (a, b, c, gq, gd)


@pytest.mark.parametrize("a, b, c, p, q, d2", [
    ((0, 0, 0), (0, 0, 0), (2, 0, 0), (1, 1, 0), (1, 0, 0), 1),     # a == b: the segment ac
    ((0, 0, 0), (2, 0, 0), (0, 0, 0), (3, 0, 4), (2, 0, 0), 17),    # a == c: the segment ab, beyond b
    ((0, 0, 0), (2, 0, 0), (2, 0, 0), (-1, 0, 1), (0, 0, 0), 2),    # b == c, before a
    ((1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 5), (1, 2, 3), 4),     # a point
    ((0, 0, 0), (2, 0, 0), (1, 0, 0), (1.5, 2, 0), (1.5, 0, 0), 4),  # collinear, c the midpoint of ab
    ((0, 0, 0), (1, 0, 0), (2, 0, 0), (1.5, 2, 0), (1.5, 0, 0), 4),  # collinear, c beyond b: the point lies over bc
    ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 4), (2, 0, 0), 17),
    ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0.5, 0, 0), (0.5, 0, 0), 0),  # on the segment
])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_degenerate_triangles_are_segments_and_points(a, b, c, p, q, d2, dtype):
    gq, gd = MD.closest_on_triangle(p, a, b, c, dtype)
    assert np.all(np.isfinite(gq)) and np.isfinite(gd)
    assert np.array_equal(gq, np.array(q, dtype)) and gd == dtype(d2)


def test_no_nan_or_inf_on_any_degenerate_shape():
    p, a, b, c = MD.soup(11, 240, 400, slivers=False)
    for k in range(0, 240, 24):  # ten copies of the six shapes
        MD.degenerate_shapes(a, b, c, k)
    q, d2 = MD.closest_on_triangle(p[:, None, :3], a[None], b[None], c[None])
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(d2))
    # a degenerate triangle is the segment between its extreme corners: compare with the float64 point-segment distance
    P = p[:, None, :3].astype(np.float64)
    best = np.full(d2.shape, np.inf)
    for u, v in ((a, b), (b, c), (a, c)):
        u, e = u[None].astype(np.float64), (v.astype(np.float64) - u.astype(np.float64))[None]
        l2 = (e * e).sum(-1)
        t = np.clip(np.where(l2 > 0, ((P - u) * e).sum(-1) / np.where(l2 > 0, l2, 1), 0), 0, 1)
        best = np.minimum(best, np.linalg.norm(P - (u + e * t[..., None]), axis=-1))
    err = np.abs(np.sqrt(d2.astype(np.float64)) - best).max()
    print("degenerate shapes: max |d32 - segment distance| = %.3g" % err)
    assert err <= PAIR_BOUND * float(np.abs(p[:, :3]).max())


# ---- the restatement against its float64 twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "shell"])
def test_float32_against_the_float64_twin(name):
    p, a, b, c = MD.soup(0, 3000, 1500) if name == "soup" else MD.shell(1, 3000, 1500)
    v, f = MD.as_mesh(a, b, c)
    L = float(max(np.abs(p[:, :3]).max(), np.abs(v[:, :3]).max()))
    worst, runner_up = 0.0, np.zeros(len(p))
    for (rows, _, d32), (_, _, d64) in zip(MD.pair_distances(p, v, f), MD.pair_distances(p, v, f, np.float64)):
        assert np.all(np.isfinite(d32))
        s64 = np.sqrt(d64)
        worst = max(worst, float(np.abs(np.sqrt(d32).astype(np.float64) - s64).max()))
        two = np.partition(s64, 1, axis=1)[:, :2]
        runner_up[rows] = two[:, 1] - two[:, 0]
    d32, t32, _ = MD.brute_force(p, v, f)
    d64, t64, _ = MD.brute_force(p, v, f, dtype=np.float64)
    mins = float(np.abs(d32.astype(np.float64) - d64).max())
    clear = runner_up > MIN_BOUND * L
    print("%s: L = %.4g, per pair |d32 - d64| <= %.3g L, per-point minimum <= %.3g L, argmin differs at %d of %d points with a clear runner-up"
          % (name, L, worst / L, mins / L, int((t32 != t64)[clear].sum()), int(clear.sum())))
    assert worst <= PAIR_BOUND * L
    assert mins <= MIN_BOUND * L
    assert clear.sum() > len(p) // 2 and np.array_equal(t32[clear], t64[clear])


def test_the_header_on_the_cpu_equals_the_restatement(tmp_path):
    """sobfu_mesh_distance.hpp through a host compiler (tests/cpp/mesh_eval_tool closest, -ffp-contract=off like the kernels): q and d2 bit
    for bit on soup pairs that hold every region and every degenerate shape"""
    from sobfu_amd import build, build_host

    build.build_hip()
    tool = build_host.build_mesh_eval_tool()
    p, a, b, c = MD.soup(3, 400, 200)
    rows = np.concatenate([np.broadcast_to(p[:, None, :3], (200, 400, 3)), *(np.broadcast_to(x[None], (200, 400, 3)) for x in (a, b, c))], -1)
    rows = np.ascontiguousarray(rows.reshape(-1, 12), np.float32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int32(len(rows)).tobytes() + rows.tobytes())
    subprocess.run([tool, "closest", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 4)
    q, d2 = MD.closest_on_triangle(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])
    assert np.array_equal(got[:, :3].view(np.uint32), q.view(np.uint32))
    assert np.array_equal(got[:, 3].view(np.uint32), d2.view(np.uint32))


# ---- two concentric icospheres ---------------------------------------------------------------------------------------------------------
def test_concentric_icospheres():
    """Inner mesh inscribed in the sphere r1, outer in r2 > r1, same subdivision.  A face is a planar triangle inscribed in its sphere; its
    plane lies r cos(alpha_f) from the centre, alpha_f its angular circumradius, so every surface point x of a mesh has
    r cos(alpha) <= |x| <= r with alpha = max alpha_f.  An outer vertex r2 u: no inner point is nearer than r2 - r1 (all lie within r1),
    and the inner surface point on the ray u is at most r2 - r1 cos(alpha) away.  An inner vertex r1 u: the outer surface point on the
    ray is at most r2 - r1 away, and no outer point is nearer than r2 cos(alpha) - r1.  Slack: the per-point fp32 bound, 1e-6 L."""
    from sobfu_amd.evaluate import distance_stats

    r1, r2 = 0.1, 0.12
    vi, fi = MD.icosphere(r1, 3)
    vo, fo = MD.icosphere(r2, 3)
    assert len(fi) == 1280 and np.array_equal(fi, fo)
    tri = vi[fi][:, :, :3].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    cos_alpha = float((np.abs((tri[:, 0] * n).sum(1)) / np.linalg.norm(n, axis=1) / r1).min())
    assert 0.98 < cos_alpha < 1
    slack = MIN_BOUND * r2
    d_oi = MD.brute_force(vo, vi, fi)[0]
    d_io = MD.brute_force(vi, vo, fo)[0]
    print("icospheres: cos(alpha) = %.6f, outer -> inner in [%.6g, %.6g] (bounds %.6g, %.6g), inner -> outer in [%.6g, %.6g] (bounds %.6g, %.6g)"
          % (cos_alpha, d_oi.min(), d_oi.max(), r2 - r1, r2 - r1 * cos_alpha, d_io.min(), d_io.max(), r2 * cos_alpha - r1, r2 - r1))
    assert d_oi.min() >= r2 - r1 - slack and d_oi.max() <= r2 - r1 * cos_alpha + slack
    assert d_io.min() >= r2 * cos_alpha - r1 - slack and d_io.max() <= r2 - r1 + slack
    s = distance_stats(d_oi)
    assert s["n"] == s["within"] == len(vo) and r2 - r1 - slack <= s["median"] <= s["max"] == float(d_oi.max())
    assert abs(s["mean"] - d_oi.astype(np.float64).mean()) <= 1e-15 and abs(s["rms"] - np.sqrt((d_oi.astype(np.float64) ** 2).mean())) <= 1e-15
    far = distance_stats(np.array([np.inf, 0.25, np.inf, 0.75], np.float32))
    assert far == dict(n=4, within=2, mean=0.5, rms=float(np.sqrt((0.0625 + 0.5625) / 2)), median=0.5, max=0.75)
    assert distance_stats(np.array([np.inf], np.float32)) == dict(n=1, within=0, mean=0.0, rms=0.0, median=0.0, max=0.0)
