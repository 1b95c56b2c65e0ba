"""Indexed (welded) marching cubes on the GPU (sobfu_hip_mc_indexed_*, ops.marching_cubes_indexed): bit for bit against the numpy
restatement tests/mc_indexed_reference.py, the never-truncate contract, the topology of a closed 256^3 sphere, per-vertex colour and the
headless app's --mesh-format ply."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import colour_reference as CR
import mc_indexed_reference as MI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")


def _bits(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", MI.CASES)
def test_hip_matches_restatement(oracle, case):
    import torch

    from sobfu_amd import _lib, ops

    vol = MI.case_volume(oracle, case)
    ref = MI.marching_cubes_indexed(vol, MI.SIZE, MI.POSE_R, MI.POSE_T)
    d = torch.from_numpy(vol).cuda()
    ws = ops.mc_indexed_workspace(d)
    v, n, f = ops.marching_cubes_indexed(d, MI.SIZE, MI.POSE_R, MI.POSE_T, workspace=ws)
    assert v.shape == (len(ref["vertices"]), 4) and f.shape == (len(ref["faces"]), 3) and f.dtype == torch.int32
    assert np.array_equal(_bits(v), ref["vertices"].view(np.uint32))
    assert np.array_equal(f.cpu().numpy(), ref["faces"])
    assert np.abs(n.cpu().numpy() - ref["normals"]).max(initial=0) <= 2e-6
    # counts of the count call
    L = _lib.lib()
    a, nv, nt = C.c_int(0), C.c_int(0), C.c_int(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.sobfu_hip_mc_indexed_count(stream, C.c_void_p(d.data_ptr()), *ops._xyz(d), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()),
                                        C.byref(a), C.byref(nv), C.byref(nt)) == 0
    assert (a.value, nv.value, nt.value) == (ref["active"], len(ref["vertices"]), len(ref["faces"]))
    # the reused workspace gives the same bits again
    for _ in range(2):
        v2, n2, f2 = ops.marching_cubes_indexed(d, MI.SIZE, MI.POSE_R, MI.POSE_T, workspace=ws)
        assert np.array_equal(_bits(v2), _bits(v)) and np.array_equal(_bits(n2), _bits(n)) and torch.equal(f2, f)
    # the soup from the same volume is the oracle's, bit for bit
    sv, sn = ops.marching_cubes(d, MI.SIZE, MI.POSE_R, MI.POSE_T)
    ov, on = oracle.marching_cubes(vol, MI.SIZE, MI.POSE_R, MI.POSE_T)
    assert np.array_equal(_bits(sv), ov.view(np.uint32)) and np.array_equal(sn.cpu().numpy(), on, equal_nan=True)
    # never truncate: a buffer one short of the counts is refused before any kernel writes
    if nt.value == 0:
        return
    assert L.sobfu_hip_mc_indexed_count(stream, C.c_void_p(d.data_ptr()), *ops._xyz(d), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()),
                                        C.byref(a), C.byref(nv), C.byref(nt)) == 0
    R9, t3 = (C.c_float * 9)(*MI.POSE_R.reshape(9).tolist()), (C.c_float * 3)(*MI.POSE_T.tolist())
    bv = torch.full((nv.value, 4), 7.0, dtype=torch.float32, device="cuda")
    bn = torch.full_like(bv, 7.0)
    bf = torch.full((nt.value, 3), -5, dtype=torch.int32, device="cuda")
    for mv, mt in ((nv.value - 1, nt.value), (nv.value, nt.value - 1)):
        rc = L.sobfu_hip_mc_indexed_generate(stream, C.c_void_p(d.data_ptr()), *ops._xyz(d), *[C.c_float(s) for s in MI.SIZE], R9, t3,
                                             C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), C.c_void_p(bv.data_ptr()),
                                             C.c_void_p(bn.data_ptr()), C.c_int(mv), C.c_void_p(bf.data_ptr()), C.c_int(mt))
        assert rc == -1, (mv, mt, rc)
    torch.cuda.synchronize()
    assert bool((bv == 7).all()) and bool((bn == 7).all()) and bool((bf == -5).all())


def test_256_cubed_sphere_is_a_closed_manifold():
    """the sphere of test_marching_cubes.py::test_hip_256_cubed_mesh_is_closed: what the soup cannot show, checked on the indices"""
    import torch

    from sobfu_amd import ops

    n, r, c = 256, 0.2, (0.375, 0.37, 0.38)
    vs = 0.75 / n
    vol = ops.new_volume((n, n, n))
    ops.init_sphere(vol, (vs,) * 3, 48 * vs, 3 * vs, c, r)
    v, nr, f = ops.marching_cubes_indexed(vol, (0.75,) * 3)
    soup_v, _ = ops.marching_cubes(vol, (0.75,) * 3)
    torch.cuda.synchronize()
    V, F = v.shape[0], f.shape[0]
    assert 3 * F == soup_v.shape[0] and F > 100_000
    f = f.cpu().numpy().astype(np.int64)
    assert f.min() >= 0 and f.max() < V
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    dkey = directed[:, 0] * V + directed[:, 1]
    assert np.unique(dkey).size == dkey.size  # every directed edge once: consistently oriented
    ukey = np.minimum(directed[:, 0], directed[:, 1]) * V + np.maximum(directed[:, 0], directed[:, 1])
    _, cnt = np.unique(ukey, return_counts=True)
    assert np.all(cnt == 2)  # every undirected edge twice: closed, no boundary
    E = cnt.size
    assert V - E + F == 2  # a sphere
    assert abs(V - F / 2) <= 2
    flip = np.array([1, -1, -1], np.float32)
    p = v.cpu().numpy()[:, :3] * flip
    d = p.astype(np.float64) - np.array(c)
    rad = np.sqrt((d ** 2).sum(1))
    assert rad.min() > r - 0.05 * vs and rad.max() < r + 0.05 * vs
    nn = nr.cpu().numpy()[:, :3].astype(np.float64) * flip
    cosang = (nn * d).sum(1) / (np.linalg.norm(nn, axis=1) * rad)
    assert cosang.min() > np.cos(np.radians(5.0))


def test_colours_are_sampled_at_the_welded_vertices(oracle):
    import torch

    from sobfu_amd import ops

    vol = MI.case_volume(oracle, "sphere32")
    X = vol.shape[2]
    rng = np.random.default_rng(5)
    colour = rng.integers(0, 256, vol.shape[:3] + (4,), dtype=np.uint8)
    colour[..., 3] = rng.choice(np.uint8([0, 1, 9, 255]), vol.shape[:3])
    d, cd = torch.from_numpy(vol).cuda(), torch.from_numpy(colour).cuda()
    v, n, f, col = ops.marching_cubes_indexed(d, MI.SIZE, MI.POSE_R, MI.POSE_T, colour=cd)
    vs = [float(np.float32(MI.SIZE[i]) / np.float32(X)) for i in range(3)]
    want = CR.sample_colour(colour, vs, MI.POSE_R, MI.POSE_T, v.cpu().numpy(), mc_vertices=True)
    col = col.cpu().numpy()
    assert col.shape == (v.shape[0], 4) and np.array_equal(col, want)
    assert (col[:, 3] > 0).sum() > 100
    # on the edges the soup walks from the lower corner up, the welded vertex is the soup's own: so is its colour
    sv, sn, scol = ops.marching_cubes(d, MI.SIZE, MI.POSE_R, MI.POSE_T, colour=cd)
    ref = MI.marching_cubes_indexed(vol, MI.SIZE, MI.POSE_R, MI.POSE_T)
    canon = np.isin(ref["edges"], MI.CANONICAL_EDGES)
    soup_c = scol.cpu().numpy().reshape(-1, 3, 4)[:, [0, 2, 1]]
    assert np.array_equal(col[f.cpu().numpy()][canon], soup_c[canon])


def _app(*args):
    from sobfu_amd import build, build_host

    build.build_hip()
    exe = build_host.build_app()
    r = subprocess.run([exe, CONFIG1, "--no-stats", *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def test_app_mesh_format_ply(tmp_path):
    ply, vtk = tmp_path / "ply", tmp_path / "vtk"
    ply.mkdir()
    vtk.mkdir()
    _app("--synthetic", "3", "--textured", "--mesh", str(ply), "--mesh-format", "ply")
    _app("--synthetic", "3", "--textured", "--mesh", str(vtk), "--mesh-format", "vtk")
    names = sorted(p.name[:-4] for p in vtk.glob("*.vtk"))
    assert sorted(p.name[:-4] for p in ply.glob("*.ply")) == names and len(names) >= 8
    assert not list(ply.glob("*.vtk")) and not list(vtk.glob("*.ply"))
    coloured = 0
    for name in names:
        text = (vtk / (name + ".vtk")).read_text()
        polygons = int(text.split("POLYGONS ")[1].split()[0])
        header, verts, faces = MI.read_ply(str(ply / (name + ".ply")))
        assert len(faces) == polygons, name
        assert faces.min() >= 0 and faces.max() < len(verts)
        has_colour = "property uchar red" in header
        assert has_colour == ("COLOR_SCALARS" in text), name
        coloured += has_colour
        assert len(verts) < len(faces)  # welded: F/2 plus half the boundary (one view's surface is open), not the soup's 3F
        ln = np.linalg.norm(np.stack([verts["nx"], verts["ny"], verts["nz"]], -1), axis=1)
        assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0)) and (ln > 0).mean() > 0.99  # unit, or (0, 0, 0) for a zero gradient
    assert coloured >= 2
    assert "--mesh-format" in subprocess.run([os.path.join(ROOT, "build", "sobfu_headless")], capture_output=True, text=True, timeout=60).stdout
