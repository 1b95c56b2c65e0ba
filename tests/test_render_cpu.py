"""The numpy restatement of the raycaster (tests/render_reference.py) against closed forms, on the CPU: a truncated sphere SDF built in
numpy, seen by a pinhole camera outside the volume and by one rotated about y.  Off the silhouette, the hit depth is within 0.05 voxel
of the float64 ray / sphere intersection and the normal within 1 degree of the radial direction; the shaders follow their formulas."""
import numpy as np
import pytest

import render_reference as RR

N, SIZE, R_SPHERE = 64, 0.5, 0.1
VS = np.float32(SIZE / N)
TRUNC = np.float32(5) * VS
INTR = (570.342 / 8, 570.342 / 8, 40.0, 30.0)
ROWS, COLS = 60, 80
CENTRE_VOL = np.array([0.25, 0.25, 0.25])


def sphere_volume(centre=CENTRE_VOL, r=R_SPHERE):
    c = (np.arange(N) + 0.5) * float(VS)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    sdf = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r
    vol = np.zeros((N, N, N, 2), np.float32)
    vol[..., 0] = np.clip(sdf / float(TRUNC), -1, 1)
    vol[..., 1] = 1
    return vol


def rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)


def analytic(R, t, centre_vol, r, intr, rows, cols):
    """float64 ray / sphere intersection in the camera frame -> depth z (0 = miss), unit normals, ray-to-centre distance"""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    C = R @ np.asarray(centre_vol, np.float64) + t
    fx, fy, cx, cy = intr
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ C), C @ C - r * r
    disc = b * b - 4 * a * cc
    z = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    n = (z[..., None] * d - C) / r
    dist = np.linalg.norm(np.cross(d, C), axis=-1) / np.linalg.norm(d, axis=-1)
    return z, n, dist


@pytest.mark.parametrize("deg", [0.0, 30.0])
def test_restatement_matches_closed_form_sphere(deg):
    R = rot_y(deg)
    cam_centre = CENTRE_VOL - R.T.astype(np.float64) @ np.array([0, 0, 0.5])  # the sphere centre sits 0.5 m in front of the camera
    t = (-(R.astype(np.float64) @ cam_centre)).astype(np.float32)
    vol = sphere_volume()
    pts, nrm = RR.raycast(vol, (VS, VS, VS), TRUNC, R, t, INTR, ROWS, COLS)
    z, n, dist = analytic(R, t, CENTRE_VOL, R_SPHERE, INTR, ROWS, COLS)
    hit = nrm[..., 3] != 0
    inner, outer = dist < R_SPHERE - 2 * float(VS), dist > R_SPHERE + float(VS)
    assert inner.sum() > 150
    assert hit[inner].all() and not hit[outer].any()
    assert np.abs(pts[..., 2] - z)[inner].max() < 0.05 * float(VS)
    cosang = np.clip((nrm[..., :3].astype(np.float64) * n).sum(-1), -1, 1)
    assert np.degrees(np.arccos(cosang[inner])).max() < 1.0
    # points lie on their pixel's ray: (x, y) = z * ((u - cx) / fx, (v - cy) / fy)
    fx, fy, cx, cy = INTR
    u, v = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    assert np.allclose(pts[..., 0][hit], (pts[..., 2] * ((u - cx) / fx))[hit], atol=1e-6)
    assert np.allclose(pts[..., 1][hit], (pts[..., 2] * ((v - cy) / fy))[hit], atol=1e-6)
    assert (pts[~hit] == 0).all() and (nrm[~hit] == 0).all()


def test_invalid_corners_never_make_a_surface():
    """A sphere whose voxels behind the surface are unobserved (weight 0): the crossing sample is invalid, so nothing is hit; an
    all-cleared volume gives all misses."""
    vol = sphere_volume()
    vol[..., 1] = (vol[..., 0] > 0).astype(np.float32)
    t = np.array([-0.25, -0.25, 0.5], np.float32)
    _, nrm = RR.raycast(vol, (VS, VS, VS), TRUNC, np.eye(3), t, INTR, ROWS, COLS)
    assert not (nrm[..., 3] != 0).any()
    _, nrm = RR.raycast(np.zeros_like(vol), (VS, VS, VS), TRUNC, np.eye(3), t, INTR, ROWS, COLS)
    assert not (nrm[..., 3] != 0).any()


def test_shaders_follow_their_formulas():
    pts = np.zeros((2, 3, 4), np.float32)
    nrm = np.zeros((2, 3, 4), np.float32)
    pts[0, 0] = (0, 0, 1, 0)
    nrm[0, 0] = (0, 0, -1, 1)  # facing the headlight: I = 1
    pts[0, 1] = (0, 0, 1, 0)
    nrm[0, 1] = (1, 0, 0, 1)  # perpendicular: I = 0.2
    pts[0, 2] = (0, 0, 1, 0)
    nrm[0, 2] = (0, 0, 1, 1)  # facing away: I = 0.2
    pts[1, 0] = (0, 0, 2, 0)
    nrm[1, 0] = (0, -0.6, -0.8, 1)  # n . l = 0.8: I = 0.84
    img = RR.render_image(pts, nrm)
    assert img[0, 0].tolist() == [255, 255, 255, 255]
    assert img[0, 1].tolist() == [51, 51, 51, 255] and img[0, 2].tolist() == [51, 51, 51, 255]
    assert img[1, 0].tolist() == [214, 214, 214, 255]  # floor(255 * 0.84 + 0.5)
    assert img[1, 1].tolist() == [0, 0, 0, 0] and img[1, 2].tolist() == [0, 0, 0, 0]
    col = RR.render_normals(nrm)
    assert col[0, 0].tolist() == [0, 128, 128, 255]  # B = z, G = y, R = x
    assert col[0, 1].tolist() == [128, 128, 255, 255]
    assert col[1, 0].tolist() == [25, 51, 128, 255]  # (-0.8 * 0.5 + 0.5) * 255 is 25.4999... in float32
    assert col[1, 1].tolist() == [0, 0, 0, 0]


def _libm_fmaf(a, b, c):
    import ctypes
    import ctypes.util

    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([m.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def planted_ties():
    """a = 1 + k 2^-23, b = 1 + 2^-12, c = +-2^-60: a b has 36 significant bits, so for many k the float64 sum rounds c away and lands
    on a float32 tie, which the second rounding then breaks to even whatever the sign of c"""
    k = np.arange(50000, dtype=np.float64)
    a = np.repeat((1 + k * 2.0 ** -23).astype(np.float32), 2)
    b = np.full_like(a, 1 + 2.0 ** -12)
    c = np.tile(np.array([2.0 ** -60, -2.0 ** -60], np.float32), k.size)
    return a, b, c


def test_fma_is_libm_fmaf():
    """RR.fma against libm's fmaf, bit for bit: random triples across 60 binades, heavy cancellation, float32 ties (where the formula it
    replaced, float32(float64 sum), is shown to differ), and the special values."""
    rng = np.random.default_rng(20)
    n = 100000

    def spread():
        return (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)

    a, b = spread(), spread()
    ab = a.astype(np.float64) * b.astype(np.float64)
    near = (1 + rng.integers(-4, 5, n) * 2.0 ** -24)
    with np.errstate(over="ignore"):
        sets = {"random": (a, b, spread()), "half": (a, b, (-ab / 2 * near).astype(np.float32)), "cancel": (a, b, (-ab * near).astype(np.float32)),
                "ties": planted_ties()}
    for name, (a, b, c) in sets.items():
        want = _libm_fmaf(a, b, c)
        got = RR.fma(a, b, c)
        assert got.dtype == np.float32 and got.shape == a.shape
        assert np.isfinite(want).all(), name
        assert np.array_equal(_bits(got), _bits(want)), name
    a, b, c = sets["ties"]
    old = RR.fma_double_rounded(a, b, c)
    differs = _bits(old) != _bits(_libm_fmaf(a, b, c))
    print("double-rounded formula differs on", int(differs.sum()), "of", a.size, "planted ties")
    assert differs.sum() >= 1
    # zeros, infinities, NaN: the same class of result, and the sign of a zero
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -2.0 ** -149, 3.4e38, -3.4e38, 2.0 ** -126], np.float32)
    a, b, c = (g.ravel() for g in np.meshgrid(sp, sp, sp, indexing="ij"))
    want, got = _libm_fmaf(a, b, c), RR.fma(a, b, c)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got)[ok], _bits(want)[ok])  # bits: +-0 and +-inf keep their signs
    assert (want[ok] == 0).sum() > 50 and np.isinf(want[ok]).sum() > 50 and (~ok).sum() > 50
    # scalars and broadcasting keep working
    assert RR.fma(np.float32(2), np.float32(3), np.float32(1)) == 7 and RR.fma(np.float32(2), np.ones(3, np.float32), 1).shape == (3,)
