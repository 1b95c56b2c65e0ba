"""Camera tracking on the CPU: the C ABI's tracking entry points (exported, argument checks before any device call, ABI version unchanged),
closed forms of the numpy restatement tests/icp_reference.py, the tracking keys of both .ini readers, and the C++ driver over
ProjectiveICP / Frame / the imgproc shells compiling with g++."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import icp_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(4096)  # a 16-byte aligned address that is never dereferenced: every case below is refused before any device call
INTR = (570.342, 570.342, 320.0, 240.0)


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


NAMES = ("sobfu_hip_depth_pyramid", "sobfu_hip_compute_point_normals", "sobfu_hip_compute_normals_mask_depth", "sobfu_hip_resize_depth_normals",
         "sobfu_hip_resize_points_normals", "sobfu_hip_icp_workspace_bytes", "sobfu_hip_icp_step", "sobfu_hip_icp_estimate")


def test_icp_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in NAMES:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3
    assert lib.sobfu_hip_icp_workspace_bytes() > 0


def _level(**kw):
    from sobfu_amd.ops import IcpLevel

    a = dict(curr=A, curr_step=64 * 16, ncurr=A, ncurr_step=64 * 16, prev=A, prev_step=64 * 16, nprev=A, nprev_step=64 * 16, rows=48, cols=64)
    a.update(kw)
    return IcpLevel(a["curr"], a["curr_step"], a["ncurr"], a["ncurr_step"], a["prev"], a["prev_step"], a["nprev"], a["nprev_step"], a["rows"], a["cols"])


def _estimate(lib, levels=None, n=1, iters=(3, 0, 0, 0), depth=0, ws=A, wsb=1 << 20, pose=A, status=A, dist=0.1, angle=0.3, fx=500.0):
    from sobfu_amd.ops import IcpLevel

    levels = [_level()] * max(n, 1) if levels is None else levels
    arr = (IcpLevel * len(levels))(*levels)
    f = C.c_float
    return lib.sobfu_hip_icp_estimate(arr, n, (C.c_int * 4)(*iters), depth, f(fx), f(500.0), f(32.0), f(24.0), f(dist), f(angle), ws, C.c_size_t(wsb),
                                      pose, status, None, None)


def _step(lib, level=None, idx=0, depth=0, aff=A, ws=A, wsb=1 << 20, sums=A, codes=None, codes_step=0, dist=0.1, angle=0.3):
    f = C.c_float
    lv = _level() if level is None else level
    return lib.sobfu_hip_icp_step(C.byref(lv), idx, depth, f(500.0), f(500.0), f(32.0), f(24.0), f(dist), f(angle), aff, ws, C.c_size_t(wsb), sums,
                                  codes, codes_step, None)


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=5), dict(ws=None), dict(pose=None), dict(status=None), dict(wsb=16), dict(depth=2), dict(dist=0.0), dict(dist=float("nan")),
    dict(angle=-1.0), dict(fx=0.0), dict(iters=(-1, 0, 0, 0)),
])
def test_icp_estimate_refuses_bad_arguments(lib, kw):
    assert _estimate(lib, **kw) == -1


@pytest.mark.parametrize("lk", [dict(curr=None), dict(ncurr=None), dict(prev=None), dict(nprev=None), dict(rows=0), dict(cols=0),
                                dict(curr_step=16), dict(nprev_step=64 * 16 - 16), dict(ncurr=C.c_void_p(4100))])
def test_icp_levels_are_checked(lib, lk):
    assert _estimate(lib, levels=[_level(**lk)]) == -1
    assert _estimate(lib, levels=[_level(), _level(**lk)], n=2, iters=(1, 1, 0, 0)) == -1
    assert _step(lib, level=_level(**lk)) == -1


def test_icp_depth_mode_steps(lib):
    # a depth level needs 2 bytes per pixel on the depth images, 16 on the normals
    assert _step(lib, level=_level(curr_step=63 * 2, prev_step=64 * 2), depth=1) == -1
    assert _step(lib, level=_level(curr_step=64 * 2, prev_step=64 * 2, ncurr_step=64 * 2), depth=1) == -1


@pytest.mark.parametrize("kw", [dict(aff=None), dict(ws=None), dict(sums=None), dict(wsb=8), dict(idx=-1), dict(idx=4), dict(depth=3),
                                dict(codes=A, codes_step=63), dict(angle=float("inf"))])
def test_icp_step_refuses_bad_arguments(lib, kw):
    assert _step(lib, **kw) == -1


def test_image_entry_points_refuse_bad_arguments(lib):
    f = C.c_float
    i = (f(500.0), f(500.0), f(32.0), f(24.0))
    assert lib.sobfu_hip_depth_pyramid(None, 128, 48, 64, A, 64, f(0.04), None) == -1
    assert lib.sobfu_hip_depth_pyramid(A, 126, 48, 64, A, 64, f(0.04), None) == -1
    assert lib.sobfu_hip_depth_pyramid(A, 128, 1, 64, A, 64, f(0.04), None) == -1
    assert lib.sobfu_hip_depth_pyramid(A, 128, 48, 64, A, 62, f(0.04), None) == -1
    assert lib.sobfu_hip_compute_point_normals(A, 128, 48, 64, *i, None, 1024, A, 1024, None) == -1
    assert lib.sobfu_hip_compute_point_normals(A, 128, 48, 64, *i, A, 1008, A, 1024, None) == -1
    assert lib.sobfu_hip_compute_point_normals(A, 128, 48, 64, f(0.0), *i[1:], A, 1024, A, 1024, None) == -1
    assert lib.sobfu_hip_compute_normals_mask_depth(A, 128, 48, 64, *i, C.c_void_p(4104), 1024, None) == -1
    assert lib.sobfu_hip_compute_normals_mask_depth(A, 128, 0, 64, *i, A, 1024, None) == -1
    assert lib.sobfu_hip_resize_depth_normals(A, 128, A, 1024, 48, 64, A, 64, A, 504, None) == -1
    assert lib.sobfu_hip_resize_depth_normals(A, 128, None, 1024, 48, 64, A, 64, A, 512, None) == -1
    assert lib.sobfu_hip_resize_points_normals(A, 1024, A, 1024, 48, 64, A, 512, A, 496, None) == -1
    assert lib.sobfu_hip_resize_points_normals(A, 1024, A, 1024, 1, 64, A, 512, A, 512, None) == -1


# ---- closed forms of the restatement ----------------------------------------------------------------------------------------------
def test_fronto_parallel_plane_normals_face_the_camera():
    d = np.full((12, 16), 800, np.uint16)
    p, n = IR.point_normals(d, INTR)
    inner = n[:-1, :-1]
    assert np.array_equal(inner[..., :3], np.broadcast_to(np.array([0, 0, -1], np.float32), inner[..., :3].shape))
    assert np.isnan(n[-1]).all() and np.isnan(n[:, -1]).all() and np.isnan(p[-1]).all()
    assert np.allclose(p[:-1, :-1, 2], 0.8)
    dm, nm = IR.normals_mask_depth(d, INTR)
    assert (dm[-1] == 0).all() and (dm[:, -1] == 0).all() and (dm[:-1, :-1] == 800).all()
    assert (nm[-1, :, 3] == 0).all()


def test_constant_depth_pyramids_to_itself():
    d = np.full((20, 30), 1234, np.uint16)
    assert np.array_equal(IR.depth_pyramid(d, 0.04), np.full((10, 15), 1234, np.uint16))


def test_pyramid_border_windows():
    # the reference's clipped upper bounds drop the last row and column of the image from every window
    rows, cols = 10, 12
    d = np.full((rows, cols), 1000, np.uint16)
    d[-1, :] = 1010
    d[:, -1] = 1010
    pyr = IR.depth_pyramid(d, 0.04)
    assert (pyr == 1000).all()
    d = np.arange(rows * cols, dtype=np.uint16).reshape(rows, cols) + 1000
    pyr = IR.depth_pyramid(d, 1.0)  # every sample qualifies: the plain window mean, truncated
    for y in range(rows // 2):
        for x in range(cols // 2):
            win = d[max(0, 2 * y - 2):min(2 * y + 3, rows - 1), max(0, 2 * x - 2):min(2 * x + 3, cols - 1)].astype(np.int64)
            assert pyr[y, x] == win.sum() // win.size
    d = np.full((rows, cols), 1000, np.uint16)
    d[1, 1] = 0  # a hole farther than 3 sigma from the centre is left out of the mean
    assert IR.depth_pyramid(d, 0.001)[0, 0] == 1000
    d[0, 0] = 0  # a hole as the centre averages only the holes
    assert IR.depth_pyramid(d, 0.001)[0, 0] == 0


def test_resize_validity_rule():
    p = np.ones((4, 4, 4), np.float32)
    n = np.zeros((4, 4, 4), np.float32)
    n[..., 2] = -1
    p[0, 0] = 0  # a raycaster miss: zeros with normal.w == 0
    n[0, 0] = 0
    pr, nr = IR.resize_points_normals(p, n)
    assert np.isnan(pr[0, 0]).all() and np.isnan(nr[0, 0]).all()
    assert np.array_equal(nr[1, 1], np.array([0, 0, -1, 0], np.float32))


def test_identical_frames_give_zero_residuals_and_identity():
    intr = (570.342 / 4, 570.342 / 4, 80.0, 60.0)
    d = IR.render_depth(np.eye(4), intr, 120, 160)
    p, n = IR.point_normals(d, intr)
    codes, row, _ = IR.correspond(0, intr, p, n, p, n, np.eye(4), 0.1, np.deg2rad(20))
    s, _ = IR.sums(row, codes)
    A_, b = IR.unpack(s)
    assert s[27] > 1000 and (b == 0).all() and s[28] == 0
    ok, x = IR.solve(A_, b)
    assert ok and (x == 0).all()
    assert np.array_equal(IR.compose(x, np.eye(4)), np.eye(4, dtype=np.float32))


def test_restatement_recovers_a_small_motion():
    # the whole coarse-to-fine estimate in numpy (points, 3 levels, {10, 5, 4}) on the analytic scene: a check of the restatement itself
    truth = IR.pose(IR.rot((0.3, 1, 0.2), 2.0), (0.012, -0.012, 0.0106))
    d = [[IR.render_depth(np.eye(4), INTR)], [IR.render_depth(truth, INTR)]]
    for k in range(2):
        for _ in range(2):
            d[k].append(IR.depth_pyramid(d[k][-1], 0.04))
    aff = np.eye(4, dtype=np.float32)
    for level, iters in ((2, 4), (1, 5), (0, 10)):
        li = tuple(float(np.float32(np.float32(v) / np.float32(1 << level))) for v in INTR)
        p0, n0 = IR.point_normals(d[0][level], li)
        p1, n1 = IR.point_normals(d[1][level], li)
        for _ in range(iters):
            codes, row, _ = IR.correspond(level, INTR, p1, n1, p0, n0, aff, 0.1, np.deg2rad(20))
            ok, x = IR.solve(*IR.unpack(IR.sums(row, codes)[0]))
            assert ok
            aff = IR.compose(x, aff)
    assert np.abs(aff[:3, 3] - truth[:3, 3]).max() < 1e-3
    assert IR.rot_angle_deg(aff[:3, :3].astype(np.float64).T @ truth[:3, :3]) < 0.1


# ---- settings ---------------------------------------------------------------------------------------------------------------------
INI_EXTRA = "TRACK_CAMERA=1\nICP_DIST_THRES=0.05\nICP_ANGLE_THRES=25\nICP_ITERS=7,3\n"


def _cpp_read(path):
    from sobfu_amd import build_host

    exe = os.path.join(ROOT, "build", "params_probe")
    src = os.path.join(ROOT, "build", "params_probe.cpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    with open(src, "w") as f:
        f.write('#include <sobfu_amd/sobfu.hpp>\nint main(int, char** argv) { Params p; if (!sobfu_amd::read_params_ini(argv[1], p)) return 1;\n'
                'std::printf("%d %.9g %.9g %d %d %d %d\\n", (int) p.track_camera, p.icp_dist_thres, p.icp_angle_thres, p.icp_iter_num[0], '
                'p.icp_iter_num[1], p.icp_iter_num[2], p.icp_iter_num[3]); return 0; }\n')
    subprocess.run(["g++", "-std=c++14", "-D__HIP_PLATFORM_AMD__", f"-I{build_host.ROCM}/include", f"-I{os.path.join(ROOT, 'include')}", src, "-o", exe,
                    f"-L{build_host.ROCM}/lib", "-lamdhip64", f"-L{os.path.join(ROOT, 'sobfu_amd')}", "-lsobfu_hip", f"-Wl,-rpath,{build_host.ROCM}/lib",
                    f"-Wl,-rpath,{os.path.join(ROOT, 'sobfu_amd')}"], check=True)
    out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.split()
    return bool(int(out[0])), float(out[1]), float(out[2]), [int(v) for v in out[3:]]


@pytest.mark.parametrize("cfg", sorted(os.listdir(os.path.join(ROOT, "params"))))
def test_shipped_configs_do_not_track(lib, cfg):
    from sobfu_amd import params

    path = os.path.join(ROOT, "params", cfg)
    P = params.read_ini(path)
    assert P["track_camera"] is False and P["icp_iter_num"] == [10, 5, 4, 0]
    track, dist, angle, iters = _cpp_read(path)
    assert track is False and iters == [10, 5, 4, 0]
    assert np.float32(dist) == np.float32(P["icp_dist_thres"]) and np.float32(angle) == np.float32(P["icp_angle_thres"])


def test_tracking_keys_parse_identically(lib, tmp_path):
    from sobfu_amd import params

    src = open(os.path.join(ROOT, "params", "config1_sphere_64.ini")).read()
    path = tmp_path / "track.ini"
    path.write_text(src + INI_EXTRA)
    P = params.read_ini(str(path))
    assert P["track_camera"] is True and P["icp_iter_num"] == [7, 3, 0, 0]
    track, dist, angle, iters = _cpp_read(str(path))
    assert track is True and iters == [7, 3, 0, 0]
    assert np.float32(dist) == np.float32(P["icp_dist_thres"]) == np.float32(0.05)
    assert np.float32(angle) == np.float32(P["icp_angle_thres"])
    assert abs(angle - np.deg2rad(25)) < 1e-6
    base = params.read_ini(os.path.join(ROOT, "params", "config1_sphere_64.ini"))
    for k, v in base.items():  # the new keys change no existing entry
        if k not in ("TRACK_CAMERA", "ICP_DIST_THRES", "ICP_ANGLE_THRES", "track_camera", "icp_dist_thres", "icp_angle_thres", "icp_iter_num"):
            assert np.array_equal(np.asarray(P[k]), np.asarray(v)), k


def test_cpp_icp_driver_compiles(lib):
    from sobfu_amd import build_host

    exe = build_host.build_icp_tool(force=True)
    assert os.path.exists(exe)
