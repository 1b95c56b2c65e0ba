"""Rigid alignment of a point list to a mesh, on the CPU: the shared solve header sobfu_amd/csrc/sobfu_rigid.hpp through a host compiler
against its restatement tests/mesh_align_reference.py bit for bit, the C ABI's new entry points (exported, ABI version unchanged, every
argument check before any device call) and the reference twin alone on exact data.

Measured here (the twin, float32 closest points of mesh_distance_reference.brute_force, float64 normal equations): the 642 vertices of the
ellipsoid target moved by 3 degrees / 5 mm return to within 1e-6 of the known pose in 4 iterations; every point ends within 3.1e-8 m of
its known position."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_align_reference as MA

F3, I3 = C.c_float * 3, C.c_int * 3
A, B, D, E, G, H = (C.c_void_p(65536 * k) for k in range(1, 7))  # 16-byte aligned addresses that are never dereferenced
BADARG = -1


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_rigid_tool()


def _run(tool, tmp_path, mode, records, out_dtype, out_cols):
    records = np.ascontiguousarray(records, np.float64)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int32(len(records)).tobytes() + records.tobytes())
    subprocess.run([tool, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    return np.fromfile(tmp_path / "out.bin", out_dtype).reshape(len(records), out_cols)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def _spd(rng, n, count):
    out = []
    for _ in range(count):
        M = rng.normal(size=(n + 3, n)) * 10.0 ** rng.uniform(-3, 2, n)
        out.append((M.T @ M, rng.normal(size=n)))
    return out


# ---- the header against the restatement, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 3])
def test_ldlt_bit_for_bit(tool, tmp_path, n):
    systems = _spd(np.random.default_rng(n), n, 200)
    got = _run(tool, tmp_path, "ldlt%d" % n, [np.concatenate([a.ravel(), b]) for a, b in systems], np.float64, 2 * n + 2)
    for (a, b), g in zip(systems, got):
        x, d, det, ok = MA.ldlt(a, b)
        assert ok and g[-1] == 1.0
        assert _same(g[:n], x) and _same(g[n:2 * n], d) and _same(g[2 * n:2 * n + 1], np.array([det]))
        assert np.abs(a @ x - b).max() <= 1e-6 * np.abs(b).max() * np.linalg.cond(a)  # and it is a solution


@pytest.mark.parametrize("n", [6, 3])
def test_ldlt_failures(tool, tmp_path, n):
    """an exactly zero pivot (a plane's normal equations: no curvature along z), a negative pivot, a NaN and an infinite pivot"""
    rng = np.random.default_rng(7)
    good, b = _spd(rng, n, 1)[0]
    zero = good.copy()
    zero[n - 1, :] = zero[:, n - 1] = 0.0
    negative = good.copy()
    negative[0, 0] = -negative[0, 0]
    nan = good.copy()
    nan[1, 1] = np.nan
    inf = good.copy()
    inf[n - 1, n - 1] = np.inf
    empty = np.zeros((n, n))
    cases = [zero, negative, nan, inf, empty]
    got = _run(tool, tmp_path, "ldlt%d" % n, [np.concatenate([a.ravel(), b]) for a in cases + [good]], np.float64, 2 * n + 2)
    assert list(got[:, -1]) == [0.0] * len(cases) + [1.0]
    assert got[0, 2 * n - 1] == 0.0 and got[1, n] < 0 and np.isnan(got[2, n + 1]) and np.isinf(got[3, 2 * n - 1])
    for a in cases:
        assert not MA.ldlt(a, b)[3]
    assert MA.ldlt(good, b)[3]


def test_rodrigues_bit_for_bit(tool, tmp_path):
    rng = np.random.default_rng(2)
    w = np.concatenate([np.zeros((1, 3)), rng.normal(size=(100, 3)) * 10.0 ** rng.uniform(-12, 0.5, (100, 1)), [[1e-200, 0, 0], [0, np.pi, 0]]])
    got = _run(tool, tmp_path, "rodrigues", w, np.float64, 10)
    for v, g in zip(w, got):
        R, th = MA.rodrigues(v)
        assert _same(g[:9], R) and g[9] == th
        assert np.abs(R.reshape(3, 3) @ R.reshape(3, 3).T - np.eye(3)).max() < 1e-14
    assert _same(got[0, :9], np.eye(3).ravel()) and got[0, 9] == 0.0  # theta == 0: I exactly (no -0, no 1 - eps)


def _poses(rng, count):
    out = []
    for _ in range(count):
        P = np.eye(4, dtype=np.float32)
        P[:3, :3] = MA.rodrigues(rng.normal(size=3))[0].reshape(3, 3).astype(np.float32)
        P[:3, 3] = rng.normal(size=3)
        out.append(P)
    return out


def test_compose_and_inverse_bit_for_bit(tool, tmp_path):
    rng = np.random.default_rng(3)
    poses = _poses(rng, 100)
    incs = [(MA.rodrigues(rng.normal(size=3) * 0.1)[0], rng.normal(size=3) * 0.01) for _ in poses]
    got = _run(tool, tmp_path, "compose", [np.concatenate([R, t, P.ravel().astype(np.float64)]) for (R, t), P in zip(incs, poses)], np.float32, 16)
    for (R, t), P, g in zip(incs, poses, got):
        assert _same(g, MA.pose_compose(R, t, P).ravel())
    inv = _run(tool, tmp_path, "inverse", [P.ravel().astype(np.float64) for P in poses], np.float32, 16)
    from sobfu_amd.evaluate import rigid_inverse

    for P, g in zip(poses, inv):
        assert _same(g, MA.rigid_inverse(P).ravel()) and _same(g, rigid_inverse(P).ravel())
        assert np.abs(g.reshape(4, 4).astype(np.float64) @ P.astype(np.float64) - np.eye(4)).max() < 1e-6
    assert _same(MA.rigid_inverse(np.eye(4)).ravel() + 0.0, np.eye(4, dtype=np.float32).ravel())


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NAMES = ("sobfu_hip_mesh_align_workspace_bytes", "sobfu_hip_mesh_align_step", "sobfu_hip_mesh_align_estimate")


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in NAMES:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3
    assert lib.sobfu_hip_mesh_align_workspace_bytes(0) == 256 * 32 * 8
    assert lib.sobfu_hip_mesh_align_workspace_bytes(5) == 256 * 32 * 8 + 32 * 5 + 12 * 8
    assert lib.sobfu_hip_mesh_align_workspace_bytes(-1) == 0


def _args(kw):
    a = dict(grid=D, grid_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), p=E, n=4, max_dist=0.0, mode=0, cap=0,
             iters=3, dof=6, eps_rot=0.0, eps_trans=0.0, ws=G, ws_bytes=1 << 20, pose=H, status=C.c_void_p(H.value + 256),
             trace=C.c_void_p(H.value + 512), sums=C.c_void_p(H.value + 1024))
    a.update(kw)
    return a


def _target(a):
    return (a["grid"], C.c_size_t(a["grid_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"], a["p"], a["n"],
            C.c_float(a["max_dist"]), a["mode"], a["cap"])


def _step(lib, **kw):
    a = _args(kw)
    return lib.sobfu_hip_mesh_align_step(*_target(a), a["pose"], a["ws"], C.c_size_t(a["ws_bytes"]), a["sums"], None)


def _estimate(lib, **kw):
    a = _args(kw)
    return lib.sobfu_hip_mesh_align_estimate(*_target(a), a["iters"], a["dof"], C.c_float(a["eps_rot"]), C.c_float(a["eps_trans"]), a["ws"],
                                             C.c_size_t(a["ws_bytes"]), a["pose"], a["status"], a["trace"], None)


SMALL = 256 * 32 * 8 + 32 * 4 + 12 * 4 - 1  # one byte less than 4 points need
COMMON_BAD = [dict(pose=None), dict(ws=None), dict(ws=C.c_void_p(G.value + 8)), dict(ws_bytes=SMALL), dict(ws_bytes=0), dict(p=None),
              dict(p=C.c_void_p(E.value + 8)), dict(p=C.c_void_p(E.value + 4)), dict(n=-1), dict(grid=None), dict(grid_bytes=16), dict(v=None),
              dict(f=None), dict(v=C.c_void_p(A.value + 4)), dict(origin=None), dict(dims=None), dict(dims=I3(0, 2, 2)), dict(h=0.0),
              dict(h=float("nan")), dict(max_dist=float("nan")), dict(mode=3), dict(mode=-1), dict(cap=-1), dict(nv=-1), dict(nt=-1)]
ESTIMATE_BAD = [dict(dof=0), dict(dof=4), dict(dof=5), dict(dof=-3), dict(iters=-1), dict(iters=1001), dict(eps_rot=-1e-9), dict(eps_trans=-1.0),
                dict(eps_rot=float("nan")), dict(eps_trans=float("inf")), dict(status=None), dict(status=C.c_void_p(H.value + 257)),
                dict(trace=C.c_void_p(H.value + 514))]


@pytest.mark.parametrize("kw", COMMON_BAD + [dict(sums=None), dict(sums=C.c_void_p(H.value + 1028))])
def test_step_bad_arguments(lib, kw):
    assert _step(lib, **kw) == BADARG


@pytest.mark.parametrize("kw", COMMON_BAD + ESTIMATE_BAD)
def test_estimate_bad_arguments(lib, kw):
    assert _estimate(lib, **kw) == BADARG
    if "n" not in kw and kw.get("ws_bytes") != SMALL:  # the checks come before n = 0 (SMALL is enough for no points)
        assert _estimate(lib, n=0, **kw) == BADARG


def test_no_points_is_a_success_without_a_device(lib):
    assert _step(lib, n=0) == 0 and _estimate(lib, n=0) == 0
    assert _estimate(lib, n=0, trace=None, dof=3, iters=0, ws_bytes=256 * 32 * 8) == 0
    assert _estimate(lib, n=0, ws_bytes=256 * 32 * 8 - 1) == BADARG


# ---- the twin alone, on exact data -----------------------------------------------------------------------------------------------------
def test_twin_recovers_a_known_motion():
    gv, gf = MA.ellipsoid()
    assert gv.shape == (642, 4) and gf.shape == (1280, 3)
    T = MA.motion(3.0, 5.0)
    src = MA.moved(gv, np.linalg.inv(T))  # pose T carries them back onto the target's own vertices
    pose, status, trace = MA.align(src, gv, gf, iters=8, eps_rot=1e-6, eps_trans=1e-6)
    print("status %#x, trace:\n%s" % (status, trace))
    assert status & 0x20000 and 3 <= (status & 0xFFFF) <= 6 and len(trace) == (status & 0xFFFF)
    assert np.abs(pose.astype(np.float64) - T).max() <= 1e-6
    err = np.linalg.norm(MA.transform(src, pose)[:, :3].astype(np.float64) - gv[:, :3], axis=1).max()
    print("largest distance to the known position: %.3g m" % err)
    assert err <= 1e-4 * float(np.abs(gv[:, :3]).max())  # kMeshMargin L, the bound on one fp32 point-triangle answer
    assert trace[0, 0] == 642 and trace[-1, 1] < 1e-7


def test_twin_translation_only_and_failure():
    sv, sf = MA.MD.icosphere(0.1, 2, (0.0, 0.0, -0.75))
    src = sv.copy()
    src[:, 0] -= np.float32(0.004)
    pose, status, trace = MA.align(src, sv, sf, iters=3, dof=3)
    assert status == 0 and _same(pose[:3, :3], np.eye(3, dtype=np.float32))
    assert np.abs(pose[:3, 3] - np.array([0.004, 0, 0])).max() <= 1e-4 * 0.85
    # a plane: no translation in x, y and no rotation about z is fixed -- an exactly zero pivot
    qv = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [1, 1, 0, 1], [0, 1, 0, 1]], np.float32)
    qf = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    pts = np.array([[0.25, 0.5, 0.125, 1], [0.75, 0.25, 0.25, 1], [0.5, 0.75, 0.5, 1]], np.float32)
    start = np.eye(4, dtype=np.float32)
    start[0, 3] = 0.0625
    for dof in (6, 3):
        pose, status, trace = MA.align(pts, qv, qf, pose=start, iters=4, dof=dof)
        assert status == 0x10000 and _same(pose, start) and len(trace) == 1 and trace[0, 0] == 3
