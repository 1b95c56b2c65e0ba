"""The cases of tests/test_gpu_render_edges.py and the facts about them that tests/test_render_cases_cpu.py proves on the CPU: small
volumes, cameras and image sizes that drive the TSDF raycaster (sobfu_amd/csrc/render_kernels.hip) to the places where it can go wrong
-- partial 16 x 16 and 64 x 4 tiles, 2-voxel-thin volumes, a surface within a voxel of each face (the gradient's clamps), a camera centre
exactly on a face (tri_setup's cf == 0 / cf == top rule), rays with exact D == 0 components inside and outside their slabs, cameras
inside, far from and looking away from the volume, unobserved, NaN-weight and non-finite voxels, a crossing whose gradient is exactly
zero -- with the restatement's result for each (tests/render_reference.py).  Numpy only: nothing here needs a GPU.  Everything a
function returns is cached and shared; treat it as read-only."""
from __future__ import annotations

import functools

import numpy as np

import render_reference as RR

F = np.float32
FIELD_DIMS, FIELD_VS, TRUNC = (24, 20, 18), (0.010, 0.012, 0.009), 0.04
DYADIC_DIMS, DYADIC_VS = (16, 12, 10), (2.0 ** -6,) * 3
PLANE_DIMS, PLANE_VS = (12, 10, 8), (0.010, 0.012, 0.009)
FLAT_DIMS = (10, 10, 9)  # `zero_gradient`
FACES = ("x0", "x1", "y0", "y1", "z0", "z1")
MINUS_X = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F)  # the camera looks along -x of the volume (90 degrees about y)
PLUS_Y = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F)   # along +y (90 degrees about x)
TURNED = np.diag([1.0, -1.0, -1.0]).astype(F)              # along -z (180 degrees about x)


def _grid(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def _volume(f, w=None):
    w = np.ones_like(f) if w is None else w
    return np.ascontiguousarray(np.stack([f, w], -1).astype(F))


def dims_of(vol):
    Z, Y, X = vol.shape[:3]
    return X, Y, Z


def extent(dims, vs):
    return np.asarray(dims, np.float64) * np.asarray(vs, F).astype(np.float64)


def field(dims, seed, zeros=0.03):
    """a smooth pseudo-random TSDF clipped to [-1, 1] -- positive toward z = 0, where the outside cameras are, with waves large enough to
    fold the surface -- and weights in {0, ..., 4}, about `zeros` of them 0"""
    rng = np.random.default_rng(seed)
    x, y, z = _grid(dims)
    c = [(d - 1) / 2 for d in dims]
    f = 0.9 * (c[2] - z) / max(c[2], 1.0)
    for _ in range(4):
        k, ph = rng.uniform(0.25, 0.9, 3), rng.uniform(0, 2 * np.pi)
        f = f + 0.45 * np.sin(k[0] * x + k[1] * y + k[2] * z + ph)
    w = np.where(rng.uniform(0, 1, f.shape) < zeros, 0, rng.integers(1, 5, f.shape))
    return _volume(np.clip(f, -1, 1), w)


def look(forward, up=(0.0, -1.0, 0.0)):
    """vol2cam rotation (float32) of a camera whose optical axis is `forward` (volume frame) and whose image y axis points away from `up`"""
    fw = np.asarray(forward, np.float64)
    fw = fw / np.linalg.norm(fw)
    x = np.cross(-np.asarray(up, np.float64), fw)
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(fw, x), fw]).astype(F)


def pose_at(R, centre):
    """t of vol2cam = (R, t) for a camera centre at `centre` (volume metres)"""
    return (-(np.asarray(R, F).astype(np.float64) @ np.asarray(centre, np.float64))).astype(F)


def _case(vol, vs, R, centre, intr, rows, cols, trunc=TRUNC, step_factor=0.75):
    return dict(vol=vol, vs=np.asarray(vs, F), trunc=F(trunc), R=np.asarray(R, F), t=pose_at(R, centre), intr=tuple(float(v) for v in intr),
                rows=rows, cols=cols, step_factor=step_factor)


def _aimed(vol, vs, eye_dir, dist, rows, cols, fill=0.8, aspect=1.0, **kw):
    """a camera `dist` from the volume's centre in direction `eye_dir`, looking at it; the focal length makes the box's bounding sphere
    fill about `fill` of the smaller image side (fx = aspect * fy)"""
    size = extent(dims_of(vol), vs)
    e = np.asarray(eye_dir, np.float64)
    e = e / np.linalg.norm(e)
    R = look(-e, up=(0.0, -1.0, 0.0) if abs(e[1]) < 0.9 else (0.0, 0.0, 1.0))
    f = fill * min(rows, cols) / 2 * dist / (np.linalg.norm(size) / 2)
    return _case(vol, vs, R, size / 2 + dist * e, (aspect * f, f, (cols - 1) / 2 + 0.25, (rows - 1) / 2 - 0.125), rows, cols, **kw)


@functools.lru_cache(None)
def field_volume():
    return field(FIELD_DIMS, 7)


@functools.lru_cache(None)
def dyadic_volume():
    return field(DYADIC_DIMS, 11)


def face_plane(face):
    """a tilted plane whose zero crossing lies 0.35 .. 0.9 voxel inside `face`, positive outside it"""
    axis, top = "xyz".index(face[0]), face[1] == "1"
    g = _grid(PLANE_DIMS)
    a, b = g[(axis + 1) % 3], g[(axis + 2) % 3]
    depth = (PLANE_DIMS[axis] - 1 - g[axis]) if top else g[axis]  # voxels inside the face
    return _volume(np.clip(0.6 * (0.35 + 0.03 * a + 0.025 * b - depth), -1, 1))


def zero_gradient_volume():
    """layers alternating +0.5 / -0.5 along z, observed from layer 4 up: the first crossing a ray can take is in cell z = 4 .. 5, where
    the tsdf one grid unit ahead and one behind are the same numbers weighted by the same fractions (g + 1 and g - 1 are exact for g
    in [4, 6]), so all three central differences cancel exactly for a ray that crosses with gx and gy in [4, 6]"""
    x, y, z = _grid(FLAT_DIMS)
    return _volume(np.where(z % 2 == 0, 0.5, -0.5), (z >= 4).astype(np.float64))


SIZES = ((1, 1), (7, 9), (17, 65), (33, 70), (16, 16))
NONFINITE = {"nan_tsdf": np.nan, "pinf_tsdf": np.inf, "ninf_tsdf": -np.inf}


def _outside(rows=33, cols=70, **kw):
    return _aimed(field_volume(), FIELD_VS, (0.0, 0.0, -1.0), 0.45, rows, cols, **kw)


def _planted(what):
    """the field volume with a few voxels around three of `outside`'s hit points replaced: their tsdf by NaN / +Inf / -Inf, or their weight by NaN"""
    c = _outside()
    ref = reference("outside")
    hits = np.argwhere(ref["normals"][..., 3] != 0)
    vol = c["vol"].copy()
    X, Y, Z = FIELD_DIMS
    for r, col in hits[[len(hits) // 5, len(hits) // 2, 4 * len(hits) // 5]]:
        g = [int(np.floor(RR.fma(ref["points"][r, col, 2], ref["trace"]["D"][i][r, col], ref["trace"]["O"][i]))) for i in range(3)]
        if what == "nan_weight":
            vol[min(g[2] + 1, Z - 1), g[1], g[0], 1] = np.nan  # the far corner of the crossing's cell
        else:
            vol[g[2], g[1], min(g[0] + 1, X - 1), 0] = NONFINITE[what]
    return vol


def _build(name):
    fv, dv = field_volume, dyadic_volume
    if name.startswith("size_"):
        rows, cols = (int(v) for v in name[5:].split("x"))
        return _outside(rows, cols, fill=1.5)
    if name == "outside":
        return _outside()
    if name == "rotated":  # about two axes
        return _aimed(fv(), FIELD_VS, (0.5, -0.35, -1.0), 0.5, 37, 53)
    if name == "inside":
        size = extent(FIELD_DIMS, FIELD_VS)
        return _case(fv(), FIELD_VS, look((0.1, 0.05, 1.0)), size * (0.45, 0.55, 0.12), (22.0, 22.0, 26.25, 18.5), 37, 53)
    if name in ("on_face_z0", "on_face_z1", "on_face_x0"):
        # dyadic voxel size and translation: O = o / vs - 0.5 is exactly 0 or dim - 1 on the axis
        vs, (X, Y, Z) = DYADIC_VS[0], DYADIC_DIMS
        if name == "on_face_z0":
            R, centre = np.eye(3, dtype=F), (8.5 * vs, 6.5 * vs, 0.5 * vs)
        elif name == "on_face_z1":
            R, centre = TURNED, (8.5 * vs, 6.5 * vs, (Z - 0.5) * vs)
        else:
            R, centre = look((1.0, 0.0, 0.0)), (0.5 * vs, 6.5 * vs, 3.5 * vs)
        return _case(dv(), DYADIC_VS, R, centre, (14.0, 14.0, 20.0, 15.0), 31, 41)
    if name in ("minus_x_in", "minus_x_out", "plus_y_in", "plus_y_out"):
        # integer cx, cy: the principal ray has dx == dy == 0, and R's exact zeros make two components of D exactly 0
        size = extent(FIELD_DIMS, FIELD_VS)
        if name.startswith("minus_x"):
            R, centre = MINUS_X, (size[0] + 0.3, 0.12 if name.endswith("_in") else -0.02, 0.08)
        else:
            R, centre = PLUS_Y, (0.12 if name.endswith("_in") else size[0] + 0.02, -0.3, 0.08)
        # the slab the principal ray is outside of, or inside all: the field is positive toward z = 0, so these cameras see it edge on
        return _case(fv(), FIELD_VS, R, centre, (60.0, 60.0, 13.0, 10.0), 21, 27)
    if name == "away":
        c = _outside(17, 23)
        return dict(c, R=TURNED @ c["R"], t=(TURNED @ c["t"]).astype(F))  # the same centre, turned round
    if name == "far":
        return _aimed(fv(), FIELD_VS, (0.2, 0.1, -1.0), 6.0, 9, 11, fill=0.35)
    if name.startswith("step_"):
        return _outside(step_factor=float(name[5:]))
    if name == "trunc_wide":
        return _outside(trunc=0.11)
    if name == "vol_2x2x2":
        vol = _volume(np.array([[[0.5, 0.8], [0.3, 0.6]], [[-0.4, -0.7], [-0.2, -0.9]]]))  # one sign change, between the z layers
        return _aimed(vol, (0.02, 0.02, 0.02), (0.7, 0.4, -1.0), 0.09, 29, 31, fill=0.95, trunc=0.03)
    if name == "vol_3x40x2":
        return _aimed(field((3, 40, 2), 3, zeros=0.01), (0.011, 0.006, 0.013), (0.6, 0.2, -1.0), 0.3, 40, 24, fill=1.5, aspect=4.0)
    if name == "vol_17x9x5":
        return _aimed(field((17, 9, 5), 5), (0.010, 0.012, 0.009), (-0.3, 0.4, -1.0), 0.3, 23, 39, fill=0.95)
    if name.startswith("plane_"):
        axis, top = "xyz".index(name[6]), name[7] == "1"
        e = np.roll([1.0, 0.7, 0.25], axis) * np.where(np.arange(3) == axis, 1.0 if top else -1.0, 1.0)
        return _aimed(face_plane(name[6:]), PLANE_VS, e, 0.25, 27, 35)
    if name in NONFINITE or name == "nan_weight":
        return dict(_outside(), vol=_planted(name))
    if name == "cleared":
        return dict(_outside(19, 21), vol=np.zeros_like(fv()))
    if name == "zero_gradient":
        return _aimed(zero_gradient_volume(), (0.01, 0.01, 0.01), (0.0, 0.0, -1.0), 0.3, 24, 28, step_factor=0.25)
    raise KeyError(name)


SIZE_CASES = tuple(f"size_{r}x{c}" for r, c in SIZES)
PLANE_CASES = tuple(f"plane_{f}" for f in FACES)
ON_FACE_CASES = ("on_face_z0", "on_face_z1", "on_face_x0")
AXIS_CASES = ("minus_x_in", "minus_x_out", "plus_y_in", "plus_y_out")
ALL_MISS_CASES = ("away", "cleared")
COUNT_EXEMPT = ("size_1x1", "far", "zero_gradient") + ALL_MISS_CASES  # zero_gradient is judged by its own condition
CASES = SIZE_CASES + ("outside", "rotated", "inside") + ON_FACE_CASES + AXIS_CASES + ("away", "far", "step_0.25", "step_0.75", "step_2.0",
        "trunc_wide", "vol_2x2x2", "vol_3x40x2", "vol_17x9x5") + PLANE_CASES + tuple(NONFINITE) + ("nan_weight", "cleared", "zero_gradient")


@functools.lru_cache(None)
def case(name):
    """-> dict(vol (Z, Y, X, 2), vs, trunc, R, t, intr, rows, cols, step_factor)"""
    c = _build(name)
    c["vol"].setflags(write=False)
    return c


def args(c):
    return (c["vs"], c["trunc"], c["R"], c["t"], c["intr"], c["rows"], c["cols"])


@functools.lru_cache(None)
def reference(name):
    """the restatement on the case -> dict(points, normals, image, colours, trace)"""
    c = case(name)
    trace = {}
    p, n = RR.raycast(c["vol"], *args(c), step_factor=c["step_factor"], trace=trace)
    out = dict(points=p, normals=n, image=RR.render_image(p, n), colours=RR.render_normals(n), trace=trace)
    for v in (p, n, out["image"], out["colours"]):
        v.setflags(write=False)
    return out


def hit_grid(name):
    """grid position of every pixel's point along its ray (meaningful on hits): three (rows, cols) float32 arrays"""
    r = reference(name)
    return [RR.fma(r["points"][..., 2], r["trace"]["D"][i], r["trace"]["O"][i]) for i in range(3)]
