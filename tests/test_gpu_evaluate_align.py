"""Automatic alignment of the ground truth in evaluation, on the GPU: SobFusion.evaluate(align=True) on config 1's translating sphere (set
up as tests/test_gpu_evaluate.py does) against an icosphere displaced by 3 mm, the solve and evaluate(align=False) left exactly as they
are, and the headless app's --evaluate-align / --evaluate-pose-out against the Python front end on the files the app wrote.

The pose cannot be pinned more finely than the reconstruction's own error: the recovered displacement is held to a_to_b.rms of the
undisplaced, unaligned evaluation -- of the float64 twin's displacement on the mesh the GPU produced, because the twin does not return
the applied displacement within that bound either (the model carries a systematic offset of its own; figures in the test and in
profiles/mesh_align.md)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_align_reference as MA

pytestmark = pytest.mark.gpu
MD = MA.MD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
SHIFT, FRAMES, MOVED = 0.005, 3, 0.003
STATE = ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi", "psi", "psi_inv")


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gt():
    """the analytic sphere of frame 0 in the frame of the meshes the app writes, (x, -y, -z): an icosphere of 5120 faces"""
    return MD.icosphere(0.1, 4, (0.0, 0.0, -0.75))


@pytest.fixture(scope="module")
def fused():
    """config 1 after three frames, and the same run with nothing evaluated in between"""
    from sobfu_amd import synthetic as S
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    runs = []
    for _ in range(2):
        f = SobFusion(P)
        for n in range(FRAMES):
            f(_gpu(S.render_sphere_depth((SHIFT * n, 0.0, 0.75), 0.1, P["intr"])))
        runs.append(f)
    yield P, runs[0], {k: _cpu(getattr(runs[1], k)).copy() for k in STATE}
    for f in runs:
        f.close()


def test_align_false_is_todays_result_and_the_state_is_untouched(fused):
    from sobfu_amd import ops
    from sobfu_amd.evaluate import compare_meshes

    P, f, untouched = fused
    gv, gf = _gt()
    v, _, faces = ops.marching_cubes_indexed(f.phi_global, P["size"], P["R"], P["t"])
    today = compare_meshes(v, faces, gv, gf)
    plain, off = f.evaluate(gv, gf), f.evaluate(gv, gf, align=False)
    assert plain == today and off == today and sorted(off) == ["a_to_b", "b_to_a", "chamfer", "hausdorff"]
    moved = np.eye(4, dtype=np.float32)
    moved[0, 3] = 0.25
    assert f.evaluate(gv, gf, pose=moved, align=False, max_dist=0.3) == f.evaluate(gv, gf, pose=moved, max_dist=0.3)
    aligned = f.evaluate(gv, gf, align=True, align_dof=3)
    assert sorted(aligned) == ["a_to_b", "align", "b_to_a", "chamfer", "hausdorff", "pose"]
    with pytest.raises(ValueError):
        f.evaluate(gv, gf, which="live", align=True)
    for k in STATE:  # psi, phi_global and the rest keep their bits: evaluation reads the volumes only
        assert np.array_equal(_bits(_cpu(getattr(f, k))), _bits(untouched[k])), k


def test_a_displaced_ground_truth_is_brought_back(fused):
    from sobfu_amd import ops

    P, f, _ = fused
    gv, gf = _gt()
    base = f.evaluate(gv, gf)
    displaced = gv.copy()
    displaced[:, 0] += np.float32(MOVED)
    unaligned = f.evaluate(displaced, gf)
    r, mv, mf, posed = f.evaluate(displaced, gf, align=True, align_dof=3, return_meshes=True)
    pose, info = r["pose"], r["align"]
    bound = base["a_to_b"]["rms"]
    back = pose[:3, 3].astype(np.float64)
    miss = float(np.linalg.norm(back - np.array([-MOVED, 0.0, 0.0])))
    # the float64 twin on the mesh the GPU produced, its correspondences from the same grid
    grid = ops.TriangleGrid(_gpu(displaced), _gpu(gf))
    correspond = lambda s: tuple(_cpu(x) for x in grid.query(_gpu(s), closest=True)[1:])
    twin = MA.rigid_inverse(MA.align(_cpu(mv), displaced, gf, iters=30, dof=3, correspond=correspond)[0])
    twin_miss = float(np.linalg.norm(twin[:3, 3].astype(np.float64) - np.array([-MOVED, 0.0, 0.0])))
    print("undisplaced a_to_b: mean %.6g rms %.6g; displaced, unaligned rms %.6g; aligned rms %.6g" %
          (base["a_to_b"]["mean"], bound, unaligned["a_to_b"]["rms"], r["a_to_b"]["rms"]))
    print("recovered %s: off the applied displacement by %.6g m (bound %.6g); the twin: %s, off by %.6g m; GPU - twin %.3g m" %
          (back, miss, bound, twin[:3, 3], twin_miss, float(np.abs(back - twin[:3, 3]).max())))
    print("status %#x, last trace row %s" % (info["status"], info["trace"][-1]))
    assert info["status"] == 0 and info["iterations"] == 30 and not info["failed"]
    assert np.array_equal(_bits(pose[:3, :3]), _bits(np.eye(3, dtype=np.float32))) and np.array_equal(_bits(pose[3]), _bits(np.array([0, 0, 0, 1], np.float32)))
    # Held against the float64 twin's displacement, not the applied one: the canonical model of this run is itself off the analytic
    # sphere by more than its rms error (the sphere moves 5 mm per frame and the model fuses three warped frames: the best-fitting
    # translation is (3.6, -0.9, -2.5) mm from the true one, where the rms falls from 2.8 to 1.2 mm), so the applied displacement is
    # not what a correct alignment returns here.  Measured: GPU and twin agree to the bit; both miss the applied one by 4.42 mm.
    assert float(np.linalg.norm(back - twin[:3, 3].astype(np.float64))) <= bound
    assert r["a_to_b"]["rms"] < unaligned["a_to_b"]["rms"]
    from sobfu_amd.fusion import transform_points

    assert np.array_equal(_bits(_cpu(posed)), _bits(transform_points(displaced, pose)))  # the refined pose is what the comparison used


EVAL = re.compile(r"^evaluate canonical (\d+): (.*)$", re.M)
ALIGN = re.compile(r"^align: (.*)$", re.M)


def test_app_evaluate_align(tmp_path):
    from sobfu_amd import build_host, mesh_io
    from sobfu_amd.evaluate import align_meshes, format_alignment

    exe = build_host.build_app()  # over the library the package has loaded: nothing of it is built here
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    gv, gf = _gt()
    gv[:, 0] += np.float32(MOVED)
    mesh_io.write_ply(tmp_path / "gt.ply", gv, gv, gf)
    common = [exe, CONFIG1, "--no-stats", "--synthetic", str(FRAMES), "--evaluate", str(tmp_path / "gt.ply")]
    out = tmp_path / "refined.txt"
    r = subprocess.run(common + ["--mesh", str(meshes), "--mesh-format", "ply", "--evaluate-align", "--evaluate-align-dof", "3", "--evaluate-pose-out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    (line,), ((n, evaluated),) = ALIGN.findall(r.stdout), EVAL.findall(r.stdout)
    print("align: " + line)
    assert int(n) == FRAMES - 1
    from sobfu_amd.params import read_ini

    limit = float(np.float32(5) * np.float32(read_ini(CONFIG1)["trunc"]))
    mv = mesh_io.read_ply(meshes / ("phi_global_%d.ply" % (FRAMES - 1)))[0]
    pv, _, pf, _ = mesh_io.read_ply(tmp_path / "gt.ply")
    pose, info = align_meshes(mv, pv, pf, iters=30, max_dist=limit, dof=3)
    assert line == format_alignment(info, pose)  # number for number at %.9g
    assert np.array_equal(_bits(np.loadtxt(out, dtype=np.float32).reshape(4, 4)), _bits(pose))
    # the written pose, read back by --evaluate-pose, gives the same evaluation line
    r2 = subprocess.run(common + ["--evaluate-pose", str(out)], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-2000:]
    assert EVAL.findall(r2.stdout) == [(n, evaluated)] and not ALIGN.findall(r2.stdout)
    # a given count of iterations; the live evaluation is never aligned
    r3 = subprocess.run(common + ["--evaluate-align", "2", "--evaluate-align-dof", "3"], capture_output=True, text=True, timeout=600)
    assert r3.returncode == 0 and "iterations=2 " in ALIGN.findall(r3.stdout)[0]
    for bad in (["--evaluate-align-dof", "4", "--evaluate-align"], ["--evaluate-pose-out", str(out)]):
        rb = subprocess.run(common + bad, capture_output=True, text=True, timeout=60)
        assert rb.returncode == 2 and "--evaluate-align" in rb.stdout
