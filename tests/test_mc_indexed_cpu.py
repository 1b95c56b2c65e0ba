"""Indexed (welded) marching cubes on the CPU: the float32 restatement (tests/mc_indexed_reference.py) against the oracle's triangle soup,
the C ABI's argument checks (no GPU needed) and the two binary PLY writers (sobfu_amd.mesh_io.write_ply, sobfu_amd::write_ply)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mc_indexed_reference as MI


@pytest.mark.parametrize("case", MI.CASES)
def test_restatement_welds_the_oracle_soup(oracle, case):
    vol = MI.case_volume(oracle, case)
    soup_v, soup_n = oracle.marching_cubes(vol, MI.SIZE, MI.POSE_R, MI.POSE_T)
    m = MI.marching_cubes_indexed(vol, MI.SIZE, MI.POSE_R, MI.POSE_T)
    V, Fc = len(m["vertices"]), len(m["faces"])
    assert 3 * Fc == len(soup_v)
    if case == "empty":
        assert V == 0 and Fc == 0
        return
    occ, count = oracle.mc_occupied_voxels(vol, 2_000_000)
    assert m["active"] == count
    faces = m["faces"]
    assert faces.min() >= 0 and faces.max() < V
    assert np.array_equal(np.unique(faces), np.arange(V))  # every vertex is used: no orphans
    assert np.all((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]))
    got = m["vertices"][faces]                               # (F, 3, 4)
    want = soup_v.reshape(-1, 3, 4)[:, [0, 2, 1]]            # soup triangle k, corners 1 and 2 swapped
    canon = np.isin(m["edges"], MI.CANONICAL_EDGES)
    assert canon.any() and (~canon).any()
    assert np.array_equal(got[canon].view(np.uint32), want[canon].view(np.uint32))
    other = ~canon
    mag = np.abs(want[other][:, :3]).max(1)
    tol = 8 * np.spacing(mag)
    assert np.all(np.abs(got[other][:, :3] - want[other][:, :3]) <= tol[:, None])
    assert np.all(got[other][:, 3] == 1)
    # normals: unit, and on the spheres within a few degrees of the soup's face normals (those are not rotated by R, marching_cubes.cu:258)
    n = m["normals"]
    assert np.all(n[:, 3] == 1)
    if case != "random":
        assert np.allclose(np.sqrt((n[:, :3].astype(np.float64) ** 2).sum(1)), 1, atol=1e-5)
        Rm = MI.POSE_R.astype(np.float64)
        flip = np.array([1, -1, -1])
        face_n = (soup_n.reshape(-1, 3, 4)[:, 0, :3] * flip) @ Rm.T * flip  # into the vertices' frame
        vert_n = n[faces][:, :, :3].astype(np.float64).mean(1)
        cosang = (face_n * vert_n).sum(1) / np.linalg.norm(vert_n, axis=1)
        assert cosang.min() > 0.9  # vertex normals agree with the soup's outward face normals
        # faces wind counter-clockwise seen from outside: their geometric normal points along the vertex normals
        p = got[:, :, :3].astype(np.float64)
        cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert np.all((cr * vert_n).sum(1) > 0)


def test_restatement_edge_rule_and_order():
    """one inside voxel: 6 cut edges around it, each shared by active cells; vertex order = owner index, then axis"""
    vol = np.zeros((5, 5, 5, 2), np.float32)
    vol[..., 0], vol[..., 1] = 1.0, 1.0
    vol[2, 2, 2, 0] = -1.0
    m = MI.marching_cubes_indexed(vol, (1, 1, 1))
    assert len(m["vertices"]) == 6 and len(m["faces"]) == 8
    mask = m["mask"]
    owners = sorted((z, y, x) for z, y, x in zip(*np.nonzero(mask)))
    assert owners == [(1, 2, 2), (2, 1, 2), (2, 2, 1), (2, 2, 2)] and mask[2, 2, 2] == 7
    p = m["vertices"][:, :3] * np.array([1, -1, -1], np.float32)
    c = np.float32(2.5 / 5)
    assert np.allclose(np.abs(p - c).max(1), 0.1) and np.allclose(np.sort(np.abs(p - c).sum(1)), 0.1)
    n = m["normals"][:, :3] * np.array([1, -1, -1], np.float32)
    assert np.all(((p - c) * n).sum(1) > 0)  # toward positive TSDF: outwards
    vol[2, 2, 3, 1] = 0.0  # an unobserved corner silences the 4 cells that touch it; their edges keep a vertex only if another cell uses it
    m2 = MI.marching_cubes_indexed(vol, (1, 1, 1))
    assert len(m2["faces"]) == 4 and len(m2["vertices"]) == 5


# ---- C ABI argument checks (every check precedes any device call) ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import _lib, build

    build.build_hip()
    return _lib.lib()


def test_abi_argument_checks(lib):
    lib.sobfu_hip_mc_indexed_workspace_bytes.restype = C.c_size_t
    ws = lib.sobfu_hip_mc_indexed_workspace_bytes(64, 64, 64)
    assert ws >= 6 * 64 ** 3 and ws <= 8 * 64 ** 3
    assert lib.sobfu_hip_mc_indexed_workspace_bytes(0, 4, 4) == 0
    assert lib.sobfu_hip_mc_indexed_workspace_bytes(512, 512, 512) <= 1.1e9
    p = C.c_void_p(256)  # never dereferenced: the checks fail first
    a, v, t = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    W = C.c_size_t(ws)
    cnt = lib.sobfu_hip_mc_indexed_count
    assert cnt(None, None, 64, 64, 64, p, W, C.byref(a), C.byref(v), C.byref(t)) == -1       # no volume
    assert cnt(None, p, 64, 64, 64, None, W, C.byref(a), C.byref(v), C.byref(t)) == -1       # no workspace
    assert cnt(None, p, 64, 64, 64, p, C.c_size_t(ws - 1), C.byref(a), C.byref(v), C.byref(t)) == -1  # workspace too small
    assert cnt(None, p, 0, 64, 64, p, W, C.byref(a), C.byref(v), C.byref(t)) == -1           # dims
    assert cnt(None, p, 64, 64, 64, p, W, None, C.byref(v), C.byref(t)) == -1
    assert cnt(None, p, 2048, 2048, 1024, p, W, C.byref(a), C.byref(v), C.byref(t)) == -3    # > INT32_MAX voxels
    assert (a.value, v.value, t.value) == (-7, -7, -7)
    R, tv = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)()
    gen = lib.sobfu_hip_mc_indexed_generate
    args = lambda **k: [k.get("st"), k.get("vol", p), 64, 64, 64, C.c_float(1), C.c_float(1), C.c_float(1), k.get("R", R), k.get("t", tv),
                        k.get("ws", p), k.get("W", W), k.get("v", p), k.get("n", p), k.get("maxv", 10), k.get("f", p), k.get("maxf", 10)]
    for bad in (dict(vol=None), dict(R=None), dict(t=None), dict(ws=None), dict(W=C.c_size_t(16)), dict(v=None), dict(n=None), dict(f=None),
                dict(maxv=-1), dict(maxf=-1)):
        assert gen(*args(**bad)) == -1, bad
    big = args()
    big[2:5] = [2048, 2048, 1024]
    assert gen(*big) == -3


# ---- binary PLY: the Python and C++ writers give the same bytes --------------------------------------------------------------------
def _mesh(n_vertices, n_faces, coloured):
    """the test mesh ply_write_tool writes (see tests/cpp/ply_write_tool.cpp)"""
    i = np.arange(n_vertices, dtype=np.float32)
    v = np.stack([i * 0.5, -i, i * 0.25 + 1, np.ones_like(i)], -1).astype(np.float32)
    one = np.float32(1)
    n = np.stack([i / (i + one), -one / (i + one), np.full_like(i, 0.5), np.ones_like(i)], -1).astype(np.float32)
    k = np.arange(n_faces, dtype=np.int64)
    f = np.stack([k % n_vertices, (k + 1) % n_vertices, (k + 2) % n_vertices], -1).astype(np.int32)
    j = np.arange(n_vertices, dtype=np.int64)
    c = np.stack([(7 * j) & 255, (13 * j + 1) & 255, (29 * j + 2) & 255, np.full_like(j, 255)], -1).astype(np.uint8) if coloured else None
    return v, n, f, c


@pytest.fixture(scope="module")
def ply_tool():
    from sobfu_amd import build, build_host

    build.build_hip()
    return build_host.build_ply_tool()


@pytest.mark.parametrize("coloured", [False, True])
def test_write_ply_python_and_cpp_agree(ply_tool, tmp_path, coloured):
    from sobfu_amd import mesh_io

    v, n, f, c = _mesh(37, 50, coloured)
    py, cpp = tmp_path / "py.ply", tmp_path / "cpp.ply"
    mesh_io.write_ply(str(py), v, n, f, c)
    assert subprocess.run([ply_tool, str(cpp), "37", "50", "1" if coloured else "0"], timeout=60).returncode == 0
    assert py.read_bytes() == cpp.read_bytes()
    header, verts, faces = MI.read_ply(str(py))
    assert ("property uchar red" in header) == coloured
    assert np.array_equal(verts["x"], v[:, 0]) and np.array_equal(verts["y"], v[:, 1]) and np.array_equal(verts["z"], v[:, 2])
    assert np.array_equal(verts["nx"], n[:, 0]) and np.array_equal(verts["nz"], n[:, 2])
    assert np.array_equal(faces, f)
    if coloured:  # BGRA in, r g b out
        assert np.array_equal(verts["red"], c[:, 2]) and np.array_equal(verts["green"], c[:, 1]) and np.array_equal(verts["blue"], c[:, 0])


def test_write_ply_empty_mesh(ply_tool, tmp_path):
    from sobfu_amd import mesh_io

    e4, e3 = np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32)
    py, cpp = tmp_path / "py.ply", tmp_path / "cpp.ply"
    mesh_io.write_ply(str(py), e4, e4, e3)
    assert subprocess.run([ply_tool, str(cpp), "0", "0", "0"], timeout=60).returncode == 0
    assert py.read_bytes() == cpp.read_bytes()
    _, verts, faces = MI.read_ply(str(py))
    assert len(verts) == 0 and len(faces) == 0
