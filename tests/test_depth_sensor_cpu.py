"""The depth sensor model and trajectories, on the CPU: the Philox known answers and the variates' statistics in the numpy restatement
(tests/depth_sensor_reference.py), the C ABI's entry points (exported, ABI version unchanged, every argument refused before any device
call), and sobfu_amd/trajectory.py with its C++ twin include/sobfu_amd/trajectory.hpp (TUM round trip, ATE and RPE against closed forms).

Measured here: the normal variate over 256 x 256 draws of stream 2, seed 12345, frame 0: mean -0.0014, variance 0.9933, max |g| 3.85."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import depth_sensor_reference as DS

A, B, D, E = (C.c_void_p(4096 * k) for k in range(1, 5))  # 16-byte aligned addresses that are never dereferenced
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_depth_sensor", "sobfu_hip_philox4x32_10"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


# ---- the generator and the variates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", DS.PHILOX_KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(x) for x in DS.philox4x32_10([counter], key)[0]) == want


def test_the_draw_is_the_pixel_frame_stream_counter_under_the_seed():
    seed = 0x0123456789ABCDEF
    d = DS.draws(seed, 7, 3, 5, 2)
    assert tuple(d[2, 4]) == tuple(DS.philox4x32_10([(4, 2, 7, 2)], (0x89ABCDEF, 0x01234567))[0])
    assert np.array_equal(DS.draws(seed, 7, 2, 3, 2, u0=2, v0=1), d[1:, 2:])  # the image size and the offset enter through (u, v) alone


def test_normal_variate_statistics():
    n = 256 * 256
    g = DS.normal_variate(DS.draws(12345, 0, 256, 256, 2)).astype(np.float64).ravel()
    assert DS.NORMAL_SCALE == np.float32(1.0 / np.sqrt(8.0 * (65536.0 ** 2 - 1.0) / 12.0))
    print("mean %.4f variance %.4f max |g| %.4f" % (g.mean(), g.var(), np.abs(g).max()))
    assert abs(g.mean()) < 4 / np.sqrt(n)  # four standard errors of a unit-variance mean
    assert abs(g.var() - 1) < 4 * np.sqrt(2 / n)  # conservative: the variate's kurtosis is below 3
    assert np.abs(g).max() < 4.9


def test_uniform_variate_range():
    w = np.array([0, 255, 256, 0xFFFFFFFF], np.uint32)
    u = DS.uniform_variate(w)
    assert u.dtype == np.float32 and u[0] == 0 and u[1] == 0 and u[2] == np.float32(2.0 ** -24) and u[3] == np.float32(1 - 2.0 ** -24) < 1


def test_reference_identity_and_branches():
    """on the analytic scene: ideal() is rint(1000 z) of every hit; the test setting reaches every flag but RANGE, z_max = 0.85 that too"""
    P, N = DS.scene(23, 37)
    hit = N[..., 3] == 1
    d, f = DS.depth_sensor(P, N, DS.ideal())
    assert np.array_equal(d[hit], np.rint(np.float32(1000) * P[..., 2][hit]).astype(np.uint16)) and not d[~hit].any()
    assert np.array_equal(f, np.where(hit, DS.VALID, DS.MISS))
    counts = DS.flag_counts(DS.depth_sensor(P, N, DS.parity_setting())[1])
    assert counts == dict(valid=572, miss=181, range=0, grazing=21, edge=62, dropout=15), counts
    counts = DS.flag_counts(DS.depth_sensor(P, N, DS.parity_setting(z_max=0.85))[1])
    assert all(v > 0 for v in counts.values()), counts


# ---- argument checks: every case is refused before any device call ------------------------------------------------------------------------
def _params(**kw):
    from sobfu_amd import _lib

    m = DS.kinect()
    m.__dict__.update({k: v for k, v in kw.items() if k in DS.FIELDS})
    return _lib.SensorParams(kw.get("seed", 1), kw.get("frame", 0), *[getattr(m, k) for k in DS.FIELDS])


def _sensor(lib, **kw):
    a = dict(points=A, points_step=16 * 16, normals=B, normals_step=16 * 16, rows=12, cols=16, depth=D, depth_step=32, flags=E, flags_step=16)
    a.update({k: v for k, v in kw.items() if k in a})
    p = None if kw.get("params", 0) is None else C.byref(_params(**kw))
    return lib.sobfu_hip_depth_sensor(a["points"], a["points_step"], a["normals"], a["normals_step"], a["rows"], a["cols"], p, a["depth"], a["depth_step"],
                                      a["flags"], a["flags_step"], None)


SENSOR_BAD = [dict(points=None), dict(normals=None), dict(depth=None), dict(params=None), dict(rows=-1), dict(cols=-1),
              dict(points_step=255), dict(points_step=264), dict(points=C.c_void_p(A.value + 8)), dict(points_step=-256),
              dict(normals_step=16), dict(normals_step=260), dict(normals=C.c_void_p(B.value + 4)),
              dict(depth_step=31), dict(depth_step=33), dict(depth=C.c_void_p(D.value + 1)), dict(flags_step=15), dict(flags_step=-16),
              dict(lateral=-0.1), dict(lateral=NAN), dict(lateral=INF), dict(z_min=NAN), dict(z_min=INF), dict(z_min=-INF), dict(z_max=NAN),
              dict(cos_min=-0.1), dict(cos_min=1.1), dict(cos_min=NAN), dict(edge_radius=-1), dict(edge_radius=4), dict(edge_jump=-0.01),
              dict(edge_jump=NAN), dict(edge_drop=-0.1), dict(edge_drop=1.5), dict(edge_drop=NAN), dict(drop=-0.1), dict(drop=1.01), dict(drop=NAN),
              dict(a0=NAN), dict(a0=INF), dict(a1=NAN), dict(a1=-INF), dict(z0=NAN), dict(z0=INF), dict(a2=NAN), dict(a2=INF),
              dict(disparity=NAN), dict(disparity=INF), dict(disparity=-1.0)]


@pytest.mark.parametrize("kw", SENSOR_BAD)
def test_depth_sensor_bad_arguments(lib, kw):
    assert _sensor(lib, **kw) == -1
    if "rows" not in kw:
        assert _sensor(lib, rows=0, **kw) == -1  # the checks come before "nothing to do"


def test_philox_bad_arguments(lib):
    K = (C.c_uint32 * 2)(1, 2)
    for args in ((None, K, 4, B), (A, None, 4, B), (A, K, 4, None), (A, K, -1, B), (C.c_void_p(A.value + 2), K, 4, B), (A, K, 4, C.c_void_p(B.value + 1)),
                 (None, K, 0, B), (A, None, 0, B)):
        assert lib.sobfu_hip_philox4x32_10(*args, None) == -1, args


def test_nothing_to_do_is_a_success_without_a_device(lib):
    assert _sensor(lib, rows=0) == 0 and _sensor(lib, cols=0, points_step=0, normals_step=0, depth_step=0, flags_step=0) == 0
    assert _sensor(lib, rows=0, flags=None, flags_step=0, z_max=INF, edge_radius=3, cos_min=1.0, drop=1.0) == 0
    assert lib.sobfu_hip_philox4x32_10(A, (C.c_uint32 * 2)(0, 0), 0, B, None) == 0


def test_the_ctypes_struct_matches_the_header():
    """the fields of sobfu_hip_sensor_params in include/sobfu_hip.h, in order, are those of _lib.SensorParams and of ops.SensorModel"""
    import dataclasses
    import re

    from sobfu_amd import _lib, ops

    txt = open(_lib.HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct sobfu_hip_sensor_params \{(.*?)\} sobfu_hip_sensor_params;", txt, re.S).group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.SensorParams._fields_] == ["seed", "frame"] + list(DS.FIELDS)
    assert [f.name for f in dataclasses.fields(ops.SensorModel)] == list(DS.FIELDS)
    for ours, theirs in ((ops.SensorModel.kinect(), DS.kinect()), (ops.SensorModel.ideal(), DS.ideal())):
        assert dataclasses.asdict(ours) == theirs.__dict__


# ---- trajectories ----------------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _trajectory(n=9, seed=3):
    """n poses of unit scale as (n, 4, 4) float64: random positions in a unit cube, rotations of up to a radian"""
    rng = np.random.default_rng(seed)
    m = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        m[i, :3, :3] = _rotation(rng.normal(size=3), rng.uniform(-1, 1))
        m[i, :3, 3] = rng.uniform(-0.5, 0.5, 3)
    return m


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_trajectory_tool()


def _tool(tool, *args):
    out = subprocess.run([tool, *map(str, args)], check=True, capture_output=True, text=True).stdout
    return {k: float(v) for k, v in (w.split("=") for w in out.split())}


def test_tum_round_trip(tmp_path, tool):
    from sobfu_amd import trajectory as T

    rows = T.from_matrices(_trajectory()).astype(np.float32)  # what tracking gives: float32 numbers
    frames = np.arange(len(rows)) * 3 + 1
    T.write_tum(tmp_path / "a.txt", rows, frames)
    got_frames, got = T.read_tum(tmp_path / "a.txt")
    assert np.array_equal(got_frames, frames) and got.dtype == np.float64
    assert np.array_equal(got.astype(np.float32).view(np.uint32), rows.view(np.uint32))  # %.9g keeps every float32
    T.write_tum(tmp_path / "b.txt", got, got_frames)
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()
    # matrices go through the quaternion the app writes; the C++ twin reads and writes the same bytes
    T.write_tum(tmp_path / "m.txt", T.to_matrices(rows.astype(np.float64)))
    assert np.allclose(np.abs((T.read_tum(tmp_path / "m.txt")[1][:, 3:] * rows[:, 3:]).sum(1)), 1, atol=1e-6)
    _tool(tool, tmp_path / "a.txt", tmp_path / "a.txt", 1, tmp_path / "c.txt")
    assert (tmp_path / "c.txt").read_bytes() == (tmp_path / "a.txt").read_bytes()
    (tmp_path / "bad.txt").write_text("# a comment\n\n0 1 2 3 0 0 0\n")
    with pytest.raises(ValueError):
        T.read_tum(tmp_path / "bad.txt")
    assert subprocess.run([tool, str(tmp_path / "bad.txt"), str(tmp_path / "a.txt")], capture_output=True).returncode == 2


def test_ate_of_a_rigidly_moved_copy_is_zero(tmp_path, tool):
    from sobfu_amd import trajectory as T

    gt = _trajectory()
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = _rotation((1, -2, 0.5), 0.9), (0.3, -0.2, 0.7)
    est = M @ gt
    assert T.ate(est, gt) < 1e-12 and T.ate(gt, gt) < 1e-12
    R, t = T.align(est, gt)
    assert np.allclose(R, M[:3, :3].T, atol=1e-12) and np.allclose(t, -M[:3, :3].T @ M[:3, 3], atol=1e-12)
    # the relative motions of a trajectory moved on the left are its own
    assert max(T.rpe(est, gt)) < 1e-12
    T.write_tum(tmp_path / "est.txt", T.from_matrices(est).astype(np.float32))
    T.write_tum(tmp_path / "gt.txt", T.from_matrices(gt).astype(np.float32))
    got = _tool(tool, tmp_path / "est.txt", tmp_path / "gt.txt")
    want = T.ate(T.read_tum(tmp_path / "est.txt")[1], T.read_tum(tmp_path / "gt.txt")[1])
    assert got["ate"] < 1e-6 and abs(got["ate"] - want) < 1e-12  # float32 files: 1e-7 of unit scale


def test_ate_of_one_displaced_pose_against_the_closed_form(tmp_path, tool):
    """n poses whose positions are symmetric about pose k's, pose k displaced by d: the centroid moves by d / n, and the cross-covariance
    of the centred positions stays sum g g^T -- the term g_k d^T vanishes with g_k = 0 -- which is symmetric and positive definite, so the
    best rotation is the identity: the alignment absorbs d / n and nothing else.  The residuals are d (1 - 1 / n) once and -d / n for the
    other n - 1 poses: ate = |d| sqrt(n - 1) / n."""
    from sobfu_amd import trajectory as T

    half = np.random.default_rng(11).uniform(-0.5, 0.5, (4, 3))
    pos = np.concatenate([half, [[0, 0, 0]], -half]) + (0.2, 0.1, -0.3)
    n, k, d = len(pos), 4, np.array([0.03, -0.04, 0.12])
    gt = _trajectory(n)
    gt[:, :3, 3] = pos
    est = gt.copy()
    est[k, :3, 3] += d
    want = np.linalg.norm(d) * np.sqrt(n - 1) / n
    assert abs(T.ate(est, gt) - want) < 1e-12
    T.write_tum(tmp_path / "est.txt", est)
    T.write_tum(tmp_path / "gt.txt", gt)
    assert abs(_tool(tool, tmp_path / "est.txt", tmp_path / "gt.txt")["ate"] - want) < 1e-8  # the files keep nine digits


def test_rpe(tmp_path, tool):
    from sobfu_amd import trajectory as T

    gt = _trajectory()
    assert T.rpe(gt, gt) == (0.0, 0.0) and T.rpe(gt, gt, delta=3) == (0.0, 0.0)
    assert T.rpe(T.from_matrices(gt), T.from_matrices(gt)) == (0.0, 0.0)
    T.write_tum(tmp_path / "gt.txt", gt)
    got = _tool(tool, tmp_path / "gt.txt", tmp_path / "gt.txt")
    assert got["rpe_trans"] == 0.0 and got["rpe_rot"] == 0.0 and got["ate"] < 1e-12
    # every second pose moved by M in its own frame: a step into a moved pose has E = B^-1 A = M, a step out of one E = B^-1 M^-1 B.
    # M a translation of length d: |trans(E)| = d and no rotation either way.  M a rotation by w: the angle of E is w either way
    # (a conjugate turns by the same angle)
    d, w = 0.01, 0.02
    M = np.eye(4)
    M[:3, 3] = np.array([2.0, -1.0, 2.0]) * d / 3
    est = gt.copy()
    est[1::2] = est[1::2] @ M
    trans, rot = T.rpe(est, gt)
    assert abs(trans - d) < 1e-12 and rot < 1e-12
    M = np.eye(4)
    M[:3, :3] = _rotation((0.3, -1, 2), w)
    est = gt.copy()
    est[1::2] = est[1::2] @ M
    trans, rot = T.rpe(est, gt)
    assert abs(rot - w) < 1e-12 and trans > 0
    T.write_tum(tmp_path / "est.txt", est)
    got = _tool(tool, tmp_path / "est.txt", tmp_path / "gt.txt")
    assert abs(got["rpe_trans"] - trans) < 1e-8 and abs(got["rpe_rot"] - rot) < 1e-8
    with pytest.raises(ValueError):
        T.rpe(gt, gt[:-1])
    with pytest.raises(ValueError):
        T.rpe(gt, gt, delta=len(gt))
