"""The inside / outside rule for closed meshes, on the CPU: the C ABI's entry points (exported, ABI version unchanged, argument checks
before any device call) and the numpy restatement tests/mesh_parity_reference.py of the row-crossing rule
(sobfu_amd/csrc/sobfu_mesh_parity.hpp) against the header itself as a host compiler takes it, on closed meshes (every row is crossed an
even number of times, also through vertices, along edges and in face planes), against analytic shapes and on an open mesh."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_parity_reference as MP

F3, I3 = C.c_float * 3, C.c_int * 3
A, B, D, E, G, H = (C.c_void_p(4096 * k) for k in range(1, 7))  # 16-byte aligned addresses that are never dereferenced
INF = float("inf")
CUBE_LO, CUBE_HI = (-0.25, -0.25, 0.75), (0.25, 0.25, 1.25)  # corners on multiples of 1 / 16


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_parity_tool()


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_mesh_voxelise_workspace_bytes", "sobfu_hip_mesh_voxelise", "sobfu_hip_mesh_inside"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


# ---- argument checks: every case is refused (or n = 0) before any device call ---------------------------------------------------------
def _voxelise(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), vol=E, X=40, Y=8, Z=4, vs=F3(0.01, 0.01, 0.01),
             trunc=0.03, eta=0.01, mode=0, bits=G, bits_bytes=1 << 12, open_rows=H)
    a.update(kw)
    return lib.sobfu_hip_mesh_voxelise(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                       a["vol"], a["X"], a["Y"], a["Z"], a["vs"], C.c_float(a["trunc"]), C.c_float(a["eta"]), a["mode"], a["bits"],
                                       C.c_size_t(a["bits_bytes"]), a["open_rows"], None)


def _inside(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), p=E, n=4, inside=G, open=H, mode=0)
    a.update(kw)
    return lib.sobfu_hip_mesh_inside(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                     a["p"], a["n"], a["inside"], a["open"], a["mode"], None)


GRID_BAD = [dict(ws=None), dict(ws=C.c_void_p(4104)), dict(ws_bytes=16), dict(origin=None), dict(dims=None), dict(h=0.0), dict(h=float("nan")),
            dict(origin=F3(0, float("nan"), 0)), dict(dims=I3(0, 2, 2)), dict(dims=I3(2, 2, 129)), dict(v=None), dict(f=None),
            dict(v=C.c_void_p(4100)), dict(f=C.c_void_p(8194)), dict(nv=-1), dict(nt=-1), dict(mode=-1), dict(mode=3)]


@pytest.mark.parametrize("kw", GRID_BAD + [dict(vol=None), dict(vol=C.c_void_p(E.value + 4)), dict(X=0), dict(Y=0), dict(Z=-1), dict(X=513), dict(vs=None),
                                           dict(vs=F3(0.01, 0, 0.01)), dict(vs=F3(0.01, 0.01, float("nan"))), dict(vs=F3(-0.01, 0.01, 0.01)),
                                           dict(trunc=0.0), dict(trunc=float("nan")), dict(trunc=INF), dict(eta=float("nan")), dict(eta=INF),
                                           dict(bits=None), dict(bits=C.c_void_p(G.value + 4)), dict(bits_bytes=8 * 4 * 2 * 4 - 1), dict(open_rows=None),
                                           dict(open_rows=C.c_void_p(H.value + 2))])
def test_voxelise_bad_arguments(lib, kw):
    assert _voxelise(lib, **kw) == -1


@pytest.mark.parametrize("kw", GRID_BAD + [dict(p=None), dict(p=C.c_void_p(E.value + 8)), dict(inside=None), dict(open=None), dict(n=-1)])
def test_inside_bad_arguments(lib, kw):
    assert _inside(lib, **kw) == -1


def test_workspace_bytes_and_nothing_to_do(lib):
    wb = lib.sobfu_hip_mesh_voxelise_workspace_bytes
    assert wb(512, 3, 5) == 16 * 4 * 15 and wb(70, 9, 5) == 3 * 4 * 45 + 4 and wb(32, 1, 1) == 16 and wb(33, 1, 1) == 16
    assert wb(513, 3, 5) == 0 and wb(0, 3, 5) == 0 and wb(8, 0, 5) == 0 and wb(8, 3, -1) == 0 and wb(8, 1 << 16, 1 << 16) == 0
    assert _inside(lib, n=0) == 0
    assert _inside(lib, n=0, ws=None) == -1 and _inside(lib, n=0, inside=None) == -1  # the checks come first


# ---- the header through a host compiler ------------------------------------------------------------------------------------------------
def _run_tool(tool, tmp_path, rows, vertices, faces):
    a, b, c = MP.corners(vertices, faces)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 2)
    tris = np.ascontiguousarray(np.concatenate([a, b, c], 1), np.float32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([len(rows), len(tris)], np.int32).tobytes() + rows.tobytes() + tris.tobytes())
    subprocess.run([tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = len(rows) * len(tris)
    return raw[:n].reshape(len(rows), len(tris)).astype(bool), raw[n:].view(np.float64).reshape(len(rows), len(tris))


def _same(tool, tmp_path, rows, vertices, faces, what):
    hit, X = _run_tool(tool, tmp_path, rows, vertices, faces)
    want_hit, want_X = MP.crossings(rows, vertices, faces)
    assert np.array_equal(hit, want_hit), "%s: the crossing flag differs at %d pairs" % (what, int((hit != want_hit).sum()))
    assert np.array_equal(X.view(np.uint64), want_X.view(np.uint64)), "%s: X differs at %d pairs" % (what, int((X.view(np.uint64) != want_X.view(np.uint64)).sum()))
    return hit, X


@pytest.fixture(scope="module")
def sphere():
    centre, radius = (0.01, -0.02, 0.5), 0.1
    v, f = MP.icosphere(radius, 3, centre)
    a, b, c = (x.astype(np.float64) for x in MP.corners(v, f))
    n = np.cross(b - a, c - a)
    plane = np.abs(((a - centre) * n).sum(1)) / np.linalg.norm(n, axis=1)  # the distance of each face's plane from the centre
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    mid = ((v[edges[:, 0], :3] + v[edges[:, 1], :3]) / np.float32(2)).astype(np.float32)
    return dict(v=v, f=f, centre=np.array(centre), radius=radius, sagitta=radius - float(plane.min()), mid=mid)


def _lattice(lo, hi, n):
    y, z = np.meshgrid(np.linspace(lo[1], hi[1], n), np.linspace(lo[2], hi[2], n), indexing="ij")
    return np.stack([y.ravel(), z.ravel()], 1).astype(np.float32)


def test_the_header_on_the_cpu_equals_the_restatement_and_closed_meshes_have_even_rows(tool, tmp_path, sphere):
    """the crossing flag and X (as float64 bits), header against restatement; rows through the exact (y, z) of every vertex and of every
    edge midpoint of the icosphere, and a lattice of rows over it: every total is even"""
    v, f = sphere["v"], sphere["f"]
    assert len(f) == 1280 and len(v) == 642 and len(sphere["mid"]) == 1920
    lat = _lattice(sphere["centre"] - 0.13, sphere["centre"] + 0.13, 27)
    for rows, what in ((v[:, 1:3], "vertex rows"), (sphere["mid"][:, 1:3], "edge rows"), (lat, "lattice rows")):
        hit, _ = _same(tool, tmp_path, rows, v, f, "icosphere, " + what)
        total = hit.sum(1)
        print("icosphere, %s: %d rows, %d crossed, %d odd totals" % (what, len(rows), int((total > 0).sum()), int((total & 1).sum())))
        assert (total > 0).sum() > len(rows) // 3 and not (total & 1).any()


def test_the_cube_on_exact_lattice_values(tool, tmp_path):
    """a 13 x 13 lattice of rows hits the cube's face planes, edges and corners exactly: even totals, header = restatement; the 13^3
    lattice points off the surface are inside iff the analytic box says so"""
    v, f = MP.cube(CUBE_LO, CUBE_HI)
    rows = _lattice((0, -0.375, 0.625), (0, 0.375, 1.375), 13)
    assert (np.abs(rows[:, 0]) == 0.25).sum() == 26 and (rows[:, 1] == 0.75).sum() == 13
    hit, _ = _same(tool, tmp_path, rows, v, f, "cube")
    total = hit.sum(1)
    print("cube: %d rows cross twice, %d not at all" % (int((total == 2).sum()), int((total == 0).sum())))
    inner = (np.abs(rows[:, 0]) < 0.25) & (np.abs(rows[:, 1] - 1) < 0.25)  # strictly inside the outline: one crossing per x face
    assert not (total & 1).any() and inner.sum() == 49 and np.all(total[inner] == 2) and set(total.tolist()) == {0, 2}
    x = np.linspace(-0.375, 0.375, 13).astype(np.float32)
    p = np.ones((13 * 13 * 13, 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = np.repeat(x, 169), np.tile(rows[:, 0], 13), np.tile(rows[:, 1], 13)
    ins, opn = MP.inside(p, v, f)
    sdf = MP.box_sdf(p[:, :3], CUBE_LO, CUBE_HI)
    off = sdf != 0
    print("cube: %d lattice points, %d off the surface, %d inside" % (len(p), int(off.sum()), int(ins.sum())))
    assert not opn.any() and off.sum() == 13 ** 3 - (9 ** 3 - 7 ** 3) and np.array_equal(ins[off] == 1, sdf[off] < 0)


def test_the_degenerate_soup(tool, tmp_path):
    """700 triangles with every degenerate shape: rows through vertices (ties) and random rows, header = restatement; a triangle without
    area is never a crossing"""
    _, v, f, lo, hi = MP.indexed_soup()
    rng = np.random.default_rng(11)
    rows = np.concatenate([v[f[::3, 0], 1:3], v[f[:24].ravel(), 1:3], rng.uniform(lo[1:], hi[1:], (600, 2)).astype(np.float32)])
    hit, X = _same(tool, tmp_path, rows, v, f, "soup")
    print("soup: %d rows x %d triangles, %d crossings" % (len(rows), len(f), int(hit.sum())))
    assert hit.sum() > 1000 and np.isfinite(X).all()
    a, b, c = (x.astype(np.float64) for x in MP.corners(v, f))
    flat = np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0
    assert flat.sum() >= 12 and not hit[:, flat].any()


def test_known_answers_on_the_sphere(sphere):
    """lattice points against the analytic sphere wherever |r - R| exceeds the sagitta (the mesh lies between the two radii)"""
    v, f, c, R = sphere["v"], sphere["f"], sphere["centre"], sphere["radius"]
    yz = _lattice(c - 0.13, c + 0.13, 27)
    x = np.linspace(c[0] - 0.13, c[0] + 0.13, 41).astype(np.float32)
    p = np.ones((len(yz) * len(x), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = np.tile(x, len(yz)), np.repeat(yz[:, 0], len(x)), np.repeat(yz[:, 1], len(x))
    ins, opn = MP.inside(p, v, f)
    r = np.linalg.norm(p[:, :3].astype(np.float64) - c, axis=1)
    decided = np.abs(r - R) > sphere["sagitta"] + 1e-6 * R  # 1e-6 R: the vertices are rounded to float32
    wrong = int(((ins[decided] == 1) != (r[decided] < R)).sum())
    print("sphere: sagitta %.3g, %d of %d points decided, %d inside, %d wrong" % (sphere["sagitta"], int(decided.sum()), len(p), int(ins.sum()), wrong))
    assert not opn.any() and decided.sum() > 0.9 * len(p) and ins.sum() > 1000 and wrong == 0


def test_an_open_cube_has_odd_rows(tool, tmp_path):
    """without one triangle of its +x face the rows through that triangle cross once: the header counts the restatement's number of odd
    rows, > 0; a z-facing triangle is parallel to the rows, never crossed, and not missed"""
    rows = _lattice((0, -0.375, 0.625), (0, 0.375, 1.375), 25)
    v, f = MP.cube(CUBE_LO, CUBE_HI, drop=[2])
    hit, _ = _same(tool, tmp_path, rows, v, f, "open cube")
    odd = int((hit.sum(1) & 1).sum())
    want = int((MP.crossings(rows, v, f)[0].sum(1) & 1).sum())
    print("open cube: %d of %d rows are odd" % (odd, len(rows)))
    assert odd == want and 100 < odd < 200  # half of the 17 x 17 rows of the outline, the diagonal to one side
    p = np.ones((len(rows), 4), np.float32)
    p[:, 1:3] = rows
    ins, opn = MP.inside(p, v, f)
    assert int(opn.sum()) == odd
    v, f = MP.cube(CUBE_LO, CUBE_HI, drop=[9])
    assert not (_same(tool, tmp_path, rows, v, f, "cube without a z triangle")[0].sum(1) & 1).any()
