"""The canonical mesh carried to live, on the CPU: the C ABI's two entry points (exported, argument checks before any device call, ABI version
unchanged) and the numpy restatement tests/mesh_warp_reference.py against closed forms (identity, an affine psi) and on the oracle's solved
scenes (the warped vertices fit phi_n better than the unwarped ones; transformed normals beat copied ones)."""
import ctypes as C

import numpy as np
import pytest

import mc_indexed_reference as MI
import mesh_warp_reference as MW
import render_reference as RR

F9, F3 = C.c_float * 9, C.c_float * 3
A = C.c_void_p(4096)  # a 16-byte aligned address that is never dereferenced: every case below is refused (or n = 0) before any device call
B = C.c_void_p(8192)
ULP64 = float(np.spacing(np.float32(64)))  # ulp32(max(X, Y, Z)) of the 64^3 cases: 7.6e-6


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_warp_points", "sobfu_hip_sample_tsdf"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


def _warp(lib, **kw):
    a = dict(psi=A, X=8, Y=8, Z=8, vs=F3(0.01, 0.01, 0.01), R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1), t=F3(0, 0, 0), mc=1, points=A, normals=None, n=4,
             points_out=B, normals_out=None)
    a.update(kw)
    return lib.sobfu_hip_warp_points(a["psi"], a["X"], a["Y"], a["Z"], a["vs"], a["R"], a["t"], a["mc"], a["points"], a["normals"], a["n"],
                                     a["points_out"], a["normals_out"], None)


def _sample(lib, **kw):
    a = dict(vol=A, X=8, Y=8, Z=8, vs=F3(0.01, 0.01, 0.01), R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1), t=F3(0, 0, 0), mc=0, points=A, n=4, out=B)
    a.update(kw)
    return lib.sobfu_hip_sample_tsdf(a["vol"], a["X"], a["Y"], a["Z"], a["vs"], a["R"], a["t"], a["mc"], a["points"], a["n"], a["out"], None)


@pytest.mark.parametrize("kw", [
    dict(psi=None), dict(vs=None), dict(R=None), dict(t=None), dict(points=None), dict(points_out=None), dict(X=0), dict(Y=-1), dict(Z=0),
    dict(n=-1), dict(normals=A), dict(normals_out=B), dict(normals=A, normals_out=None), dict(vs=F3(0, 0.01, 0.01)), dict(vs=F3(0.01, -1, 0.01)),
    dict(vs=F3(0.01, 0.01, float("nan"))), dict(vs=F3(float("inf"), 0.01, 0.01)), dict(psi=C.c_void_p(4104)), dict(points=C.c_void_p(4100)),
    dict(points_out=C.c_void_p(8200)), dict(normals=C.c_void_p(4104), normals_out=B), dict(normals=A, normals_out=C.c_void_p(8196)),
])
def test_warp_points_bad_arguments(lib, kw):
    assert _warp(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(vol=None), dict(vs=None), dict(R=None), dict(t=None), dict(points=None), dict(out=None), dict(X=0), dict(Y=0), dict(Z=-3), dict(n=-1),
    dict(vs=F3(0.01, 0, 0.01)), dict(vs=F3(0.01, 0.01, float("nan"))), dict(vol=C.c_void_p(4100)), dict(points=C.c_void_p(4104)),
    dict(out=C.c_void_p(8194)),
])
def test_sample_tsdf_bad_arguments(lib, kw):
    assert _sample(lib, **kw) == -1


def test_no_points_is_a_success_without_a_device(lib):
    assert _warp(lib, n=0) == 0 and _warp(lib, n=0, normals=A, normals_out=B) == 0 and _sample(lib, n=0) == 0
    assert _warp(lib, n=0, psi=None) == -1 and _sample(lib, n=0, out=None) == -1  # the checks come first


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
def _identity(dims):
    X, Y, Z = dims
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in (Z, Y, X)), indexing="ij")
    return np.stack([xx, yy, zz, np.zeros_like(xx)], -1)


def _rotation(deg_y=25.0, deg_z=-40.0):
    a, b = np.radians(deg_y), np.radians(deg_z)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return Ry @ Rz


def _unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([v, np.ones((n, 1))], -1).astype(np.float32)


@pytest.mark.parametrize("mc", [False, True])
def test_identity_psi_returns_the_input(mc):
    """psi = identity: every displacement is exactly 0, so the points come back value for value whatever the pose; the normals (identity pose:
    R^T and R are exact) come back within 1 ulp of a unit component, 2^-23 -- the rounding of 1 / sqrt(|n|^2) and of the product."""
    rng = np.random.default_rng(1)
    dims, vs = (20, 18, 16), (0.01, 0.012, 0.009)
    psi = _identity(dims)
    pts = np.concatenate([rng.uniform(-0.05, 0.25, (5000, 3)), np.ones((5000, 1))], -1).astype(np.float32)
    nrm = _unit_normals(rng, 5000)
    nrm[::97, :3] = 0
    R, t = _rotation().astype(np.float32), np.array([0.02, -0.01, 0.03], np.float32)
    out = MW.warp_points(psi, vs, R, t, pts, mc_vertices=mc)
    assert np.array_equal(out, pts)
    out, n = MW.warp_points(psi, vs, np.eye(3), (0, 0, 0), pts, nrm, mc_vertices=mc)
    assert np.array_equal(out, pts)
    err = np.abs(n[:, :3] - nrm[:, :3]).max()
    print("identity psi: max |normal out - normal in| = %.3g (1 ulp = %.3g)" % (err, np.spacing(np.float32(1))))
    assert err <= np.spacing(np.float32(1))
    assert np.all(n[:, 3] == 1) and np.array_equal(n[::97, :3], np.zeros_like(n[::97, :3]))


@pytest.mark.parametrize("mc", [False, True])
def test_affine_psi_against_float64(mc):
    """psi(x) = A x + b: the trilinear interpolant of an affine map is the map, and its Jacobian is A in every cell, so the only errors are
    psi's float32 storage and the float32 lerp chain.  Positions within 8 ulp32(64) max(vs), unit normals within 16 ulp32(64) per component."""
    rng = np.random.default_rng(2)
    dims = (64, 64, 64)
    vs = np.array([0.008, 0.0075, 0.0085], np.float32).astype(np.float64)  # the float32 values the restatement works with
    Am = np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3))
    b = rng.uniform(-0.5, 0.5, 3)
    idn = _identity(dims).astype(np.float64)
    psi = np.zeros(idn.shape, np.float32)
    psi[..., :3] = (idn[..., :3] @ Am.T + b).astype(np.float32)
    R64, t64 = _rotation(), np.array([0.05, -0.1, 0.2])
    R, t = R64.astype(np.float32), t64.astype(np.float32)
    n = 20000
    g = rng.uniform(1.0, 62.0, (n, 3))  # interior cells: no clamp
    flip = np.array([1.0, -1.0, -1.0]) if mc else np.ones(3)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = ((((g + 0.5) * vs) @ R.astype(np.float64).T + t.astype(np.float64)) * flip).astype(np.float32)
    nrm = _unit_normals(rng, n)
    out, nout = MW.warp_points(psi, vs, R, t, pts, nrm, mc_vertices=mc)
    # float64 from the float32 points actually handed over
    R64, t64 = R.astype(np.float64), t.astype(np.float64)
    w = pts[:, :3].astype(np.float64) * flip
    g64 = ((w - t64) @ R64) / vs - 0.5
    want = (((g64 @ Am.T + b + 0.5) * vs) @ R64.T + t64) * flip
    perr = np.abs(out[:, :3] - want).max()
    Ametric = R64 @ np.diag(vs) @ Am @ np.diag(1 / vs) @ R64.T
    wn = (nrm[:, :3].astype(np.float64) * flip) @ np.linalg.inv(Ametric)  # rows: (A^-T n)^T = n^T A^-1
    wn = wn / np.linalg.norm(wn, axis=1, keepdims=True) * flip
    nerr = np.abs(nout[:, :3] - wn).max()
    print("affine psi (mc_vertices=%d): max position error %.3g m (bound %.3g), max normal error %.3g (bound %.3g)"
          % (mc, perr, 8 * ULP64 * vs.max(), nerr, 16 * ULP64))
    assert perr <= 8 * ULP64 * vs.max()
    assert nerr <= 16 * ULP64
    assert np.all(out[:, 3] == 1) and np.all(nout[:, 3] == 1)


def test_clamped_axis_has_no_derivative():
    """a point beyond the box: tri_setup collapses the axis (h == g), the displacement is the face's and the derivative along it is 0"""
    dims, vs = (8, 8, 8), (0.01,) * 3
    psi = _identity(dims)
    psi[..., 0] += 0.25 * psi[..., 0]  # u.x = 0.25 x: du.x/dx = 0.25 inside
    pts = np.array([[0.035, 0.04, 0.04, 1], [0.2, 0.04, 0.04, 1]], np.float32)  # g.x = 3: inside; g.x = 19.5: clamped to 7
    nrm = np.array([[0.6, 0.8, 0, 1], [0.6, 0.8, 0, 1]], np.float32)
    out, n = MW.warp_points(psi, vs, np.eye(3), (0, 0, 0), pts, nrm)
    assert abs(out[0, 0] - (0.035 + 0.25 * 3.0 * 0.01)) < 1e-7 and abs(out[1, 0] - (0.2 + 0.25 * 7 * 0.01)) < 1e-7
    want0 = np.array([0.6 / 1.25, 0.8]) / np.hypot(0.6 / 1.25, 0.8)
    assert np.abs(n[0, :2] - want0).max() < 1e-6 and np.abs(n[1, :2] - [0.6, 0.8]).max() < 1e-6


def test_sample_tsdf_restatement():
    rng = np.random.default_rng(3)
    dims = (12, 10, 9)
    X, Y, Z = dims
    vol = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.choice([0.0, 1.0, 1.0, 1.0, 3.0], (Z, Y, X))], -1).astype(np.float32)
    vs = (0.01, 0.011, 0.012)
    R, t = _rotation().astype(np.float32), np.array([0.02, -0.01, 0.03], np.float32)
    pts = np.concatenate([rng.uniform(-0.05, 0.2, (4000, 3)), np.ones((4000, 1))], -1).astype(np.float32)
    for mc in (False, True):
        got = MW.sample_tsdf(vol, vs, R, t, pts, mc_vertices=mc)
        _, g = MW.grid_position(vs, R, t, pts, mc)
        f, _ = RR.sample(vol.reshape(-1, 2), dims, *g)
        # a corner weight of 0, found independently of the sampler: the eight corners of the clamped cell
        bad = np.zeros(len(pts), bool)
        lo = [np.floor(np.clip(g[i], 0, dims[i] - 1)).astype(int) for i in range(3)]
        hi = [np.minimum(lo[i] + ((np.clip(g[i], 0, dims[i] - 1) != 0) & (np.clip(g[i], 0, dims[i] - 1) != dims[i] - 1)), dims[i] - 1) for i in range(3)]
        for xs in (lo[0], hi[0]):
            for ys in (lo[1], hi[1]):
                for zs in (lo[2], hi[2]):
                    bad |= vol[zs, ys, xs, 1] == 0
        assert bad.any() and (~bad).any()
        assert np.array_equal(np.isnan(got), bad)
        assert np.array_equal(got[~bad].view(np.uint32), f[~bad].view(np.uint32))


# ---- the oracle's solved scenes ---------------------------------------------------------------------------------------------------------
N, VS = 64, np.float32(0.5 / 64)
TRUNC, ETA = np.float32(5) * VS, np.float32(2) * VS


def _solve(oracle, pg, pn, iters):
    psi = oracle.new_field((N, N, N))
    oracle.init_identity(psi)
    oracle.estimate_psi(pg, pn, psi, max_iter=iters, alpha=0.1, w_reg=0.2)  # config 1's solver settings
    return psi


def test_warped_vertices_fit_phi_n_on_the_shifted_sphere(oracle):
    """sphere shifted 0.64 voxel in x, 100 iterations: rms |phi_n| at the welded vertices through psi is at most half the unwarped one"""
    pg, pn = oracle.new_volume((N, N, N)), oracle.new_volume((N, N, N))
    oracle.init_sphere(pg, (VS,) * 3, TRUNC, ETA, (0.25, 0.25, 0.25), 0.1)
    oracle.init_sphere(pn, (VS,) * 3, TRUNC, ETA, (0.255, 0.25, 0.25), 0.1)
    psi = _solve(oracle, pg, pn, 100)
    v = MI.marching_cubes_indexed(pg, (0.5,) * 3)["vertices"]
    assert len(v) > 3000
    rms = []
    for pts in (v, MW.warp_points(psi, (VS,) * 3, np.eye(3), (0, 0, 0), v, mc_vertices=True)):
        d = MW.sample_tsdf(pn, (VS,) * 3, np.eye(3), (0, 0, 0), pts, mc_vertices=True).astype(np.float64) * 5.0  # voxels: trunc = 5 voxels
        assert np.isfinite(d).mean() > 0.99
        rms.append(float(np.sqrt(np.nanmean(d * d))))
    print("shifted sphere, 100 iterations: rms |phi_n| at %d welded vertices %.4f voxel unwarped, %.4f through psi (x %.3f)"
          % (len(v), rms[0], rms[1], rms[1] / rms[0]))
    assert rms[1] <= 0.5 * rms[0]


def test_transformed_normals_beat_copied_normals_on_the_ellipsoid(oracle):
    """sphere r = 0.1 -> ellipsoid (0.108, 0.1, 0.092), 100 iterations: the normals pushed through psi's Jacobian make a smaller mean angle
    with grad phi_n at the warped vertex than the normals merely copied"""
    pg, pn = oracle.new_volume((N, N, N)), oracle.new_volume((N, N, N))
    oracle.init_sphere(pg, (VS,) * 3, TRUNC, ETA, (0.25, 0.25, 0.25), 0.1)
    oracle.init_ellipsoid(pn, (VS,) * 3, TRUNC, (0.108, 0.1, 0.092))
    psi = _solve(oracle, pg, pn, 100)
    m = MI.marching_cubes_indexed(pg, (0.5,) * 3)
    v, n = m["vertices"], m["normals"]
    wv, wn = MW.warp_points(psi, (VS,) * 3, np.eye(3), (0, 0, 0), v, n, mc_vertices=True)
    _, g = MW.grid_position((VS,) * 3, np.eye(3), (0, 0, 0), wv, True)
    flat = pn.reshape(-1, 2)
    one = np.float32(1)
    grad = np.stack([RR.sample_tsdf(flat, (N, N, N), *[g[i] + (one if i == a else 0) for i in range(3)]).astype(np.float64) -
                     RR.sample_tsdf(flat, (N, N, N), *[g[i] - (one if i == a else 0) for i in range(3)]).astype(np.float64) for a in range(3)], -1)
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    flip = np.array([1.0, -1.0, -1.0])

    def angle(nn):
        c = ((nn[:, :3].astype(np.float64) * flip) * grad).sum(1) / np.linalg.norm(nn[:, :3].astype(np.float64), axis=1)
        return np.degrees(np.arccos(np.clip(c, -1, 1)))

    a_t, a_c = angle(wn), angle(n)
    print("ellipsoid, 100 iterations, %d vertices: angle to grad phi_n transformed mean %.2f max %.2f deg, copied mean %.2f max %.2f deg"
          % (len(v), a_t.mean(), a_t.max(), a_c.mean(), a_c.max()))
    assert a_t.mean() < a_c.mean()
