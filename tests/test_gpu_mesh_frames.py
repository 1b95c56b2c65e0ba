"""Ground-truth meshes in, depth frames out, fusion, error back against the same meshes: config 1's 64^3 run of two frames driven from
sobfu_amd.mesh_render.render_mesh_depth of a translating icosphere, beside the same run driven from the analytic sphere
(synthetic.render_sphere_depth), both scored by SobFusion.evaluate against the icosphere of the last frame; and the headless app's
--render-mesh PATTERN --evaluate-live PATTERN on written .ply files.

Measured on the MI355X (two frames, 5 mm per frame, icosphere of 5120 faces, live model against the last frame's icosphere, a_to_b rms):
see DESIGN.md 4.11."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_ray_reference as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
SHIFT, FRAMES, RADIUS = 0.005, 2, 0.1


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gt(frame):
    """the sphere of frame n -- centre (shift n, 0, 0.75) in the camera frame, as the app's --synthetic --shift moves it -- as an icosphere
    of 5120 faces in the frame of the meshes the app writes, (x, -y, -z)"""
    return MR.icosphere(RADIUS, 4, (SHIFT * frame, 0.0, -0.75))


def test_fusion_driven_from_meshes_scores_like_the_analytic_run():
    from sobfu_amd import mesh_render, synthetic as S
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    gv, gf = _gt(FRAMES - 1)
    tri = gv[gf][:, :, :3].astype(np.float64)
    centre = np.array([SHIFT * (FRAMES - 1), 0.0, -0.75])
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float((np.abs(((tri[:, 0] - centre) * n).sum(1)) / np.linalg.norm(n, axis=1)).min())  # the nearest face plane
    sagitta = RADIUS - r_in
    assert 0 < sagitta < 2e-4
    rms, frames = {}, {}
    for source in ("analytic", "mesh"):
        f = SobFusion(P)
        for k in range(FRAMES):
            if source == "analytic":
                depth = S.render_sphere_depth((SHIFT * k, 0.0, 0.75), RADIUS, P["intr"])
            else:
                depth = mesh_render.render_mesh_depth(*_gt(k), P["intr"], pose=mesh_render.MESH_FRAME)
            assert depth.dtype == np.uint16 and depth.shape == (480, 640)
            frames[source, k] = depth
            f(_gpu(depth))
        r = f.evaluate(gv, gf, which="live")
        assert r["a_to_b"]["within"] == r["a_to_b"]["n"] > 100
        rms[source] = r["a_to_b"]["rms"]
        f.close()
    for k in range(FRAMES):  # the frames themselves: the mesh lies inside the sphere, so it covers no pixel the sphere does not, and none nearer
        a, m = frames["analytic", k].astype(np.int64), frames["mesh", k].astype(np.int64)
        both = (a > 0) & (m > 0)
        assert both.sum() > 0.95 * (a > 0).sum() and not np.any((m > 0) & (a == 0)) and np.all(m[both] >= a[both] - 1)
    print("live model against the last frame's icosphere, a_to_b rms: analytic-driven %.6g m, mesh-driven %.6g m; sagitta %.3g m"
          % (rms["analytic"], rms["mesh"], sagitta))
    # the mesh-driven frames see a surface at most r - r_in inside the analytic one, then round to millimetres
    assert rms["mesh"] <= rms["analytic"] + sagitta + 1e-3
    assert 0 < rms["mesh"] < float(P["trunc"])


LINE = re.compile(r"^evaluate live (\d+): (.*)$", re.M)


def test_app_render_mesh_and_evaluate_live_share_a_pattern(tmp_path):
    """sobfu_headless --render-mesh PATTERN --evaluate-live PATTERN on written .ply files: the frames are rendered from the meshes and
    every solved frame is scored against the mesh it was rendered from, through the one grid built for it.  The app scores solved frames
    only and frame 0 is never solved, so three files give the two "evaluate live" lines.  The same run with the ground truth under
    another name (its own grid per evaluation) prints the same numbers."""
    from sobfu_amd import build, build_host, mesh_io
    from sobfu_amd.params import read_ini

    build.build_hip()
    exe = build_host.build_app()
    for n in range(3):
        gv, gf = _gt(n)
        nrm = gv.copy()
        nrm[:, :3] = (gv[:, :3] - np.array([SHIFT * n, 0, -0.75], np.float32)) / np.float32(RADIUS)
        for name in ("gt_%06d.ply", "copy_%06d.ply"):
            mesh_io.write_ply(tmp_path / (name % n), gv, nrm, gf)
    runs = []
    for scored in ("gt_%06d.ply", "copy_%06d.ply"):
        r = subprocess.run([exe, CONFIG1, "--no-stats", "--render-mesh", str(tmp_path / "gt_%06d.ply"), "--evaluate-live", str(tmp_path / scored)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        runs.append(LINE.findall(r.stdout))
        print("\n".join("evaluate live %s: %s" % l for l in runs[-1]))
    assert [int(n) for n, _ in runs[0]] == [1, 2] and runs[0] == runs[1]
    P = read_ini(CONFIG1)
    for _, text in runs[0]:
        got = dict(kv.split("=") for kv in text.split())
        assert int(got["a_to_b.within"]) == int(got["a_to_b.n"]) > 100 and int(got["b_to_a.n"]) == len(_gt(0)[0])
        assert 0 < float(got["a_to_b.mean"]) <= float(got["a_to_b.rms"]) < float(P["trunc"])
    bad = subprocess.run([exe, CONFIG1, "--render-mesh", str(tmp_path / "gt_%06d.ply"), "--synthetic", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--render-mesh excludes" in bad.stdout
    none = subprocess.run([exe, CONFIG1, "--render-mesh", str(tmp_path / "nowhere_%06d.ply")], capture_output=True, text=True, timeout=60)
    assert none.returncode == 2 and "no frame 0" in none.stdout
