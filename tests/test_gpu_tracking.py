"""The frame pipeline with camera tracking on the MI355X: a moving-camera sequence of the analytic scene (config 1 at 64^3, 5 frames,
1 degree and 5 mm per frame) through fusion.SobFusion and through apps/sobfu_headless --data ... --track --poses: every pose within
4 mm and 0.5 degrees of the truth, the two trajectories equal to 1e-6; and --poses without --track writes identity poses."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import icp_reference as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "params", "config1_sphere_64.ini")


def _png16(path, img):
    raw = b"".join(b"\x00" + img[r].astype(">u2").tobytes() for r in range(img.shape[0]))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 16, 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _truth(k):
    return IR.pose(IR.rot((0.2, 1.0, 0.1), 1.0 * k), np.array([0.6, -0.5, 0.62]) * 0.005 * k / np.linalg.norm([0.6, -0.5, 0.62]))


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _read_tum(path):
    out = []
    for line in open(path):
        v = [float(x) for x in line.split()]
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = _quat_to_R(v[4:8]), v[1:4]
        out.append(P)
    return out


def _check(poses, n):
    assert len(poses) == n
    for k, P in enumerate(poses):
        T = _truth(k)
        assert np.abs(P[:3, 3] - T[:3, 3]).max() < 4e-3, (k, P[:3, 3], T[:3, 3])
        assert IR.rot_angle_deg(np.asarray(P[:3, :3], np.float64).T @ T[:3, :3]) < 0.5, k


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    from sobfu_amd import params

    P = params.read_ini(CFG)
    d = tmp_path_factory.mktemp("moving")
    os.makedirs(d / "depth")
    for k in range(5):
        _png16(str(d / "depth" / f"{k:06d}.png"), IR.render_depth(_truth(k), P["intr"]))
    return d


def test_moving_camera_is_tracked_by_python_and_the_app(sequence):
    from sobfu_amd import build, build_host, fusion, params

    build.build_hip()
    app = build_host.build_app()
    P = params.read_ini(CFG)
    P["track_camera"] = True
    F = fusion.SobFusion(P)
    try:
        for k in range(5):
            img = IR.render_depth(_truth(k), P["intr"])
            F(torch.from_numpy(img.view(np.int16)).cuda())
        torch.cuda.synchronize()
        py = [p.astype(np.float64) for p in F.poses]
        img = F.render("phi_global")
        assert (img[..., 3] != 0).sum() > 1000  # rendered from the tracked pose: the model is in view
    finally:
        F.close()
    _check(py, 5)
    poses = str(sequence / "poses.txt")
    r = subprocess.run([app, CFG, "--data", str(sequence), "--track", "--poses", poses, "--no-stats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tracking failed" not in r.stdout
    cpp = _read_tum(poses)
    _check(cpp, 5)
    for a, b in zip(py, cpp):
        assert np.abs(a - b).max() < 1e-6, (a, b)


def test_poses_without_tracking_are_identity(tmp_path):
    from sobfu_amd import build, build_host

    build.build_hip()
    app = build_host.build_app()
    poses = str(tmp_path / "poses.txt")
    r = subprocess.run([app, CFG, "--synthetic", "3", "--poses", poses, "--no-stats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = open(poses).read().split("\n")[:-1]
    assert lines == [f"{k} 0 0 0 0 0 0 1" for k in range(3)]
