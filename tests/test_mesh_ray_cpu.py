"""Rays against triangle meshes, on the CPU: the C ABI's entry points (exported, ABI version unchanged, argument checks before any device
call) and the numpy restatement tests/mesh_ray_reference.py of the ray-triangle rule (sobfu_amd/csrc/sobfu_mesh_ray.hpp) against closed
forms, against its float64 twin, against the header itself as a host compiler takes it, and on a closed icosphere (watertightness).

Measured here, restatement vs float64 twin on the soup (700 triangles with every degenerate shape x 4096 rays, 10865 pairs that hit in
both; L = the largest absolute coordinate of the mesh and the origins, 5.0): |d|_inf |t32 - t64| <= 9.6e-7 L; 302 pairs hit in one and
miss in the other, every one with a float64 edge function within 4.8e-10 (4 L)^2 of 0.  The grid walk's margin, kRayMargin = 1e-4
(sobfu_amd/csrc/mesh_ray_kernels.hip), has to be at least ten times the measured maximum: the bound asserted is 1e-5 L."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import mesh_ray_reference as MR

F3, I3, F9 = C.c_float * 3, C.c_int * 3, C.c_float * 9
A, B, D, E, G = (C.c_void_p(4096 * k) for k in range(1, 6))  # 16-byte aligned addresses that are never dereferenced
PAIR_BOUND = 1e-5  # a tenth of kRayMargin
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_ray_tool()


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_mesh_raycast", "sobfu_hip_mesh_render"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


def test_the_margin_is_ten_times_the_bound():
    import os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sobfu_amd", "csrc", "mesh_ray_kernels.hip")).read()
    margin = float(re.search(r"constexpr float kRayMargin\s*=\s*([0-9.e+-]+)f;", src).group(1))
    assert margin >= 10 * PAIR_BOUND


# ---- argument checks: every case is refused (or n = 0) before any device call ---------------------------------------------------------
def _raycast(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), o=E, d=C.c_void_p(E.value + 4096), n=4,
             t_min=0.0, t_max=0.0, mode=0, t=G, tri=C.c_void_p(G.value + 4096), bary=None, side=None)
    a.update(kw)
    return lib.sobfu_hip_mesh_raycast(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                      a["o"], a["d"], a["n"], C.c_float(a["t_min"]), C.c_float(a["t_max"]), a["mode"], a["t"], a["tri"], a["bary"],
                                      a["side"], None)


def _render(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), vn=None, vc=None, R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1),
             t=F3(0, 0, 0), fx=500.0, fy=500.0, cx=8.0, cy=6.0, rows=12, cols=16, z_min=0.0, z_max=0.0, depth=None, depth_step=0, points=None,
             points_step=0, normals=None, normals_step=0, colour=None, colour_step=0, tri=None, tri_step=0)
    a.update(kw)
    return lib.sobfu_hip_mesh_render(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                     a["vn"], a["vc"], a["R"], a["t"], C.c_float(a["fx"]), C.c_float(a["fy"]), C.c_float(a["cx"]), C.c_float(a["cy"]),
                                     a["rows"], a["cols"], C.c_float(a["z_min"]), C.c_float(a["z_max"]), a["depth"], a["depth_step"], a["points"],
                                     a["points_step"], a["normals"], a["normals_step"], a["colour"], a["colour_step"], a["tri"], a["tri_step"], None)


GRID_BAD = [dict(ws=None), dict(ws=C.c_void_p(4104)), dict(ws_bytes=16), dict(origin=None), dict(dims=None), dict(h=0.0), dict(h=-1.0),
            dict(h=float("nan")), dict(h=INF), dict(origin=F3(0, float("nan"), 0)), dict(origin=F3(INF, 0, 0)), dict(dims=I3(0, 2, 2)),
            dict(dims=I3(2, -1, 2)), dict(dims=I3(2, 2, 129)), dict(v=None), dict(f=None), dict(v=C.c_void_p(4100)), dict(f=C.c_void_p(8194)),
            dict(nv=-1), dict(nt=-1)]


@pytest.mark.parametrize("kw", GRID_BAD + [dict(o=None), dict(d=None), dict(t=None), dict(tri=None), dict(n=-1), dict(o=C.c_void_p(E.value + 8)),
                                           dict(d=C.c_void_p(E.value + 4100)), dict(t=C.c_void_p(G.value + 2)), dict(tri=C.c_void_p(G.value + 4097)),
                                           dict(bary=C.c_void_p(G.value + 4)), dict(t_min=float("nan")), dict(t_min=INF), dict(t_min=-INF),
                                           dict(t_max=float("nan")), dict(mode=-1), dict(mode=3)])
def test_raycast_bad_arguments(lib, kw):
    assert _raycast(lib, **kw) == -1


@pytest.mark.parametrize("kw", GRID_BAD + [dict(R=None), dict(t=None), dict(R=F9(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)), dict(t=F3(0, INF, 0)),
                                           dict(fx=0.0), dict(fy=float("nan")), dict(cx=INF), dict(rows=0), dict(cols=-3), dict(z_min=float("nan")),
                                           dict(z_max=float("nan")), dict(vn=C.c_void_p(A.value + 8)), dict(vc=C.c_void_p(A.value + 2)),
                                           dict(depth=G, depth_step=31), dict(depth=C.c_void_p(G.value + 1), depth_step=32), dict(depth=G, depth_step=33),
                                           dict(points=G, points_step=255), dict(points=G, points_step=264), dict(points=C.c_void_p(G.value + 8), points_step=256),
                                           dict(normals=G, normals_step=16), dict(normals=C.c_void_p(G.value + 4), normals_step=256),
                                           dict(colour=G, colour_step=64, vc=None), dict(colour=G, colour_step=60, vc=A),
                                           dict(colour=C.c_void_p(G.value + 2), colour_step=64, vc=A), dict(tri=G, tri_step=63),
                                           dict(tri=C.c_void_p(G.value + 2), tri_step=64)])
def test_render_bad_arguments(lib, kw):
    assert _render(lib, depth=kw.pop("depth", G), depth_step=kw.pop("depth_step", 32), **kw) == -1


def test_nothing_to_do_is_a_success_without_a_device(lib):
    assert _raycast(lib, n=0) == 0 and _raycast(lib, n=0, bary=A, side=C.c_void_p(A.value + 1), t_max=INF, mode=2) == 0
    assert _raycast(lib, n=0, ws=None) == -1 and _raycast(lib, n=0, t=None) == -1  # the checks come first
    assert _render(lib) == 0  # no output asked for
    assert _render(lib, ws=None) == -1 and _render(lib, fx=0.0) == -1


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
TV = np.array([[0, 0, 0, 1], [2, 0, 0, 1], [0, 2, 0, 1]], np.float32)


def _one(o, d, faces=((0, 1, 2),), t_min=0.0, t_max=None, dtype=np.float32):
    o4, d4 = np.array([list(o) + [1]], np.float32), np.array([list(d) + [0]], np.float32)
    t, tri, bary, side = MR.brute_force(o4, d4, TV, np.array(faces, np.int32), t_min, t_max, dtype)
    return float(t[0]), int(tri[0]), tuple(float(x) for x in bary[0]), int(side[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_triangle(dtype):
    assert _one((0.5, 0.25, 3), (0, 0, -1), dtype=dtype) == (3.0, 0, (0.25, 0.125), 1)  # counter-clockwise from the origin: the front
    assert _one((0.5, 0.25, -3), (0, 0, 1), dtype=dtype) == (3.0, 0, (0.25, 0.125), -1)
    assert _one((0.5, 0.25, 3), (0, 0, -2), dtype=dtype) == (1.5, 0, (0.25, 0.125), 1)  # t counts in units of d
    assert _one((0.5, 0.25, 3), (0, 0, -1), faces=((0, 2, 1),), dtype=dtype) == (3.0, 0, (0.125, 0.25), -1)  # the other winding
    for corner, bary in (((0, 0), (0, 0)), ((2, 0), (1, 0)), ((0, 2), (0, 1)), ((1, 0), (0.5, 0)), ((1, 1), (0.5, 0.5)), ((0, 1), (0, 0.5))):
        assert _one(corner + (1,), (0, 0, -1), dtype=dtype) == (1.0, 0, bary, 1), corner  # corners and edges belong to the triangle
    assert _one((2.5, 0.25, 3), (0, 0, -1), dtype=dtype)[1] == -1 and _one((0.5, 0.25, 3), (0, 0, 1), dtype=dtype) == (INF, -1, (0, 0), 0)
    assert _one((0.5, 0.25, 0), (1, 0, 0), dtype=dtype)[1] == -1  # in the triangle's plane: det = 0
    assert _one((0.5, 0.25, 3), (0, 0, -1), t_max=3.0, dtype=dtype)[1] == 0 and _one((0.5, 0.25, 3), (0, 0, -1), t_max=2.999, dtype=dtype)[1] == -1
    assert _one((0.5, 0.25, 3), (0, 0, -1), t_min=3.0, dtype=dtype)[1] == -1 and _one((0.5, 0.25, 3), (0, 0, -1), t_min=2.999, dtype=dtype)[1] == 0
    for t_max in (None, 0.0, -1.0, INF):
        assert _one((0.5, 0.25, 3), (0, 0, -1), t_max=t_max, dtype=dtype)[0] == 3.0
    assert _one((0.5, 0.25, 3), (0, 0, -1), faces=((0, 2, 1), (0, 1, 2)), dtype=dtype)[1] == 0  # coplanar duplicates: the lowest index
    for faces in (((0, 0, 1),), ((1, 1, 1),), ((0, 1, 0),)):  # degenerate triangles are misses
        assert _one((0.5, 0, 3), (0, 0, -1), faces=faces, dtype=dtype) == (INF, -1, (0, 0), 0)


def test_bad_rays_miss():
    for o, d in (((0.5, 0.25, 3), (0, 0, 0)), ((0.5, 0.25, 3), (0, 0, float("nan"))), ((0.5, 0.25, 3), (0, INF, -1)), ((0.5, 0.25, 3), (0, 0, -INF)),
                 ((float("nan"), 0.25, 3), (0, 0, -1)), ((0.5, INF, 3), (0, 0, -1)), ((0.5, 0.25, 3), (0, 0, -1e-45))):
        with np.errstate(all="ignore"):
            assert _one(o, d) == (INF, -1, (0, 0), 0), (o, d)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_every_major_axis(axis, sign):
    """the same triangle and ray with the coordinates rotated: every kz and both signs of d[kz] give the same answer"""
    perm = [(0 + axis) % 3, (1 + axis) % 3, (2 + axis) % 3]
    v = np.ones((3, 4), np.float32)
    v[:, perm] = TV[:, :3] * [1, 1, sign]
    o, d = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.float32)
    o[0, perm], d[0, perm] = [0.5, 0.25, 3 * sign], [0.125, 0.25, -sign]
    t, tri, bary, side = MR.brute_force(o, d, v, np.array([[0, 1, 2]], np.int32))
    assert (t[0], tri[0], side[0]) == (3.0, 0, sign) and tuple(bary[0]) == (0.4375, 0.5)


# ---- the header through a host compiler ------------------------------------------------------------------------------------------------
def _run_tool(tool, tmp_path, origins, dirs, vertices, faces, t_min=0.0, t_max=0.0):
    a, b, c = MR.corners(vertices, faces)
    rays = np.ascontiguousarray(np.concatenate([origins[:, :3], dirs[:, :3]], 1), np.float32)
    tris = np.ascontiguousarray(np.concatenate([a, b, c], 1), np.float32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([len(rays), len(tris)], np.int32).tobytes() + np.array([t_min, t_max], np.float32).tobytes() + rays.tobytes() + tris.tobytes())
    subprocess.run([tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    out = np.fromfile(tmp_path / "out.bin", np.dtype([("t", "<f4"), ("tri", "<i4"), ("u", "<f4"), ("v", "<f4"), ("side", "<i4")]))
    return out["t"], out["tri"], np.stack([out["u"], out["v"]], 1), out["side"].astype(np.int8)


def _same(got, want, what):
    for name, g, w in zip(("t", "tri", "bary", "side"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).reshape(len(w), -1).any(1))[0]
        assert bad.size == 0, "%s %s differs at %d rays, first %d: got %r want %r" % (what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.fixture(scope="module")
def soup():
    _, v, f, lo, hi = MR.indexed_soup()
    o, d = MR.soup_rays(v, f, lo, hi)
    return dict(v=v, f=f, lo=lo, hi=hi, o=o, d=d)


def test_the_header_on_the_cpu_equals_the_restatement(tool, tmp_path, soup):
    """sobfu_mesh_ray.hpp through a host compiler (tests/cpp/mesh_ray_tool, -ffp-contract=off like the kernels): t, tri, barycentrics and
    side bit for bit on the soup (every degenerate shape; rays through vertices and edge midpoints, where the fp64 recomputation runs)"""
    want = MR.brute_force(soup["o"], soup["d"], soup["v"], soup["f"])
    hits = int((want[1] >= 0).sum())
    print("soup: %d of %d rays hit, %d front, %d back" % (hits, len(want[1]), int((want[3] > 0).sum()), int((want[3] < 0).sum())))
    assert 0.3 * len(want[1]) < hits < 0.9 * len(want[1]) and (want[3] > 0).sum() > 100 and (want[3] < 0).sum() > 100
    _same(_run_tool(tool, tmp_path, soup["o"], soup["d"], soup["v"], soup["f"]), want, "soup")
    limit = float(np.median(want[0][np.isfinite(want[0])]))
    cut = MR.brute_force(soup["o"], soup["d"], soup["v"], soup["f"], 0.25 * limit, limit)
    assert (cut[1] != want[1]).sum() > 100
    _same(_run_tool(tool, tmp_path, soup["o"], soup["d"], soup["v"], soup["f"], 0.25 * limit, limit), cut, "soup, limited")


# ---- the restatement against its float64 twin ---------------------------------------------------------------------------------------------
def test_float32_against_the_float64_twin(soup):
    v, f, o, d = soup["v"], soup["f"], soup["o"], soup["d"]
    used = v[np.unique(f), :3]
    L = float(max(np.abs(used).max(), np.abs(o[:, :3]).max()))
    r32, r64 = MR.ray_setup(o, d), MR.ray_setup(o, d, np.float64)
    c32, c64 = MR.corners(v, f), MR.corners(v, f, np.float64)
    worst, both, differ, noise = 0.0, 0, 0, 0.0
    for i in range(0, len(o), 256):
        p32, p64 = ({k: x[i:i + 256] for k, x in r.items()} for r in (r32, r64))
        t32 = MR.ray_triangle(p32, *c32, 0.0, np.inf)[0]
        t64, _, _, _, (U, V, W) = MR.ray_triangle(p64, *c64, 0.0, np.inf, np.float64, parts=True)
        h32, h64 = np.isfinite(t32), np.isfinite(t64)
        scale = np.abs(d[i:i + 256, :3]).max(1)[:, None]  # t counts in units of d
        with np.errstate(invalid="ignore"):
            err = np.abs(t32.astype(np.float64) - t64) * scale
        m = h32 & h64
        if m.any():
            worst = max(worst, float(err[m].max()))
        both += int(m.sum())
        x = h32 != h64
        if x.any():
            differ += int(x.sum())
            noise = max(noise, float(np.minimum(np.minimum(np.abs(U), np.abs(V)), np.abs(W))[x].max()))
    edge_noise = PAIR_BOUND * (4 * L) ** 2  # a sheared coordinate is at most 4 L, an edge function a difference of two of their products
    print("soup: L = %.4g, |d| |t32 - t64| <= %.3g L over %d pairs that hit in both; %d pairs hit in one only, their smallest float64 edge function"
          " <= %.3g (4 L)^2" % (L, worst / L, both, differ, noise / (4 * L) ** 2))
    assert both > 5000
    assert worst <= PAIR_BOUND * L
    assert noise <= edge_noise


# ---- a closed mesh ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    v, f = MR.icosphere(0.1, 2, (0.01, -0.02, 0.5))
    o, d = MR.watertight_rays(v, f)
    return dict(v=v, f=f, o=o, d=d)


def test_watertight_on_a_closed_icosphere(tool, tmp_path, sphere):
    """rays from outside toward the centre, one through every vertex, one through every edge midpoint, 2000 through random points on
    edges: every one hits, in the restatement and in the header; t = 1 is the centre, so the first hit is in front of it, on the outside"""
    v, f, o, d = sphere["v"], sphere["f"], sphere["o"], sphere["d"]
    assert len(f) == 320 and len(o) == 162 + 480 + 2000
    for t_max in (0.0, 1.0):
        want = MR.brute_force(o, d, v, f, 0.0, t_max)
        assert np.all(want[1] >= 0) and np.all(want[3] == 1) and np.all(want[0] < 1)
        _same(_run_tool(tool, tmp_path, o, d, v, f, 0.0, t_max), want, "icosphere")


def test_a_missing_face_lets_rays_through(tool, tmp_path, sphere):
    """the same mesh without face 7: rays into that face's interior now reach the far side (unlimited) or nothing (t_max = 1, the centre)"""
    v, f = sphere["v"], sphere["f"]
    gone = 7
    keep = np.arange(len(f)) != gone
    tri = v[f[gone], :3].astype(np.float64)
    w = np.array([[1, 1, 1], [2, 1, 1], [1, 3, 1], [1, 1, 4], [5, 5, 1]], np.float64)
    inner = (w / w.sum(1, keepdims=True)) @ tri
    centre = v[np.unique(f), :3].astype(np.float64).mean(0)
    o, d = np.ones((len(inner), 4), np.float32), np.zeros((len(inner), 4), np.float32)
    o[:, :3] = centre + 3.0 * (inner - centre)
    d[:, :3] = centre - o[:, :3].astype(np.float64)
    full = MR.brute_force(o, d, v, f, 0.0, 1.0)
    assert np.all(full[1] == gone)
    for t_max, tri_ok, side in ((1.0, lambda t: t == -1, 0), (0.0, lambda t: t >= 0, -1)):
        want = MR.brute_force(o, d, v, f[keep], 0.0, t_max)
        assert np.all(tri_ok(want[1])) and np.all(want[3] == side) and np.all(want[0] > 1)
        _same(_run_tool(tool, tmp_path, o, d, v, f[keep], 0.0, t_max), want, "missing face")
    # the rays of the closed test: float32 origins put a ray aimed at an edge of face 7 a hair to one side of it.  Those that chose face 7
    # now miss, or hit a neighbour that shares the edge or corner the ray passes exactly, at the same t within twice the bound of
    # test_float32_against_the_float64_twin; the others are unmoved
    was = MR.brute_force(sphere["o"], sphere["d"], v, f, 0.0, 1.0)
    now = MR.brute_force(sphere["o"], sphere["d"], v, f[keep], 0.0, 1.0)
    chose = was[1] == gone
    assert np.array_equal(now[1][~chose], was[1][~chose] - (was[1][~chose] > gone)) and np.array_equal(now[0][~chose], was[0][~chose])
    lost = chose & (now[1] < 0)
    print("face %d removed: %d rays had chosen it, %d of them now miss" % (gone, int(chose.sum()), int(lost.sum())))
    kept = chose & ~lost
    L = float(max(np.abs(v[:, :3]).max(), np.abs(sphere["o"][:, :3]).max()))
    assert lost.sum() > 0 and np.all(np.abs(now[0][kept].astype(np.float64) - was[0][kept]) * np.abs(sphere["d"][kept, :3]).max(1) <= 2 * PAIR_BOUND * L)
