"""The cases of tests/test_gpu_mc_edges.py and the facts about them that tests/test_mc_cases_cpu.py proves on the CPU: volumes that drive
marching cubes (sobfu_amd/csrc/mc_kernels.hip) and its three-pass scan (sobfu_amd/csrc/sobfu_scan.hpp) to the places where they change
regime -- the carry between slabs of scan_blocks, chunk seams, thin and tiny volumes, degenerate TSDF values, a closed form, the caps and
synthetic mc_offsets inputs -- with the references of each (the oracle's soup, the restatement's indexed mesh) and the bounds measured on
those references.  Numpy and the oracle only: nothing here needs a GPU.  Everything a function returns is cached and shared; treat it as
read-only."""
from __future__ import annotations

import functools

import numpy as np

import mc_indexed_reference as MI

F = np.float32
BLOCK, ITEMS = 256, 8
CHUNK = BLOCK * ITEMS  # cells per workgroup (sobfu_scan.hpp: kChunk)
SLAB = 1024            # per-chunk sums one pass of scan_blocks' loop takes
FLIP = np.array([1.0, -1.0, -1.0])
IDENTITY = (np.eye(3, dtype=F), np.zeros(3, F))

SEAM_DIMS = ((64, 4, 8), (41, 10, 5), (17, 16, 8), (255, 3, 3), (257, 3, 3), (30, 9, 10), (2050, 2, 2))
SEAM_CELLS = ((30, 9, 10), (2050, 2, 2))  # the seam volumes in which voxels 2047 and 2048 are cells themselves (the others have them on the top layer)
TINY_DIMS = ((2, 2, 2), (3, 2, 2), (2, 2, 9), (70, 2, 2))
FLAT_DIMS = ((1, 5, 5), (5, 1, 5), (5, 5, 1))
DEGENERATE_DIMS = (11, 7, 9)
DEGENERATE_VALUES = (0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-30, -1e-30, 1e-40, -1e-40)
PLANE_DIMS, PLANE_N, PLANE_D = (37, 21, 13), (0.31, 1.0, -0.42), 9.7

# ---- measured on the references by tests/test_mc_cases_cpu.py (it prints them and checks them against what is written here) -------------
# `plane`, float64, after undoing the flip and the pose and dividing by the float32 cell sizes.  Rounding only (a linear TSDF is exact
# under linear interpolation: there is no model error), hence a margin of 4 on each.
PLANE_MARGIN = 4.0
PLANE_RESIDUAL_MEASURED = 2.03e-6     # largest distance of a soup or welded vertex from the plane, grid units
PLANE_NORMAL_MEASURED = 4.6e-8        # largest component error of an indexed normal against R normalize(n / cs), flipped
PLANE_SOUP_NORMAL_MEASURED = 1.2e-5   # largest component error of a finite soup normal against normalize(n / cs), flipped (not rotated)
PLANE_RESIDUAL_BOUND = PLANE_MARGIN * PLANE_RESIDUAL_MEASURED
PLANE_NORMAL_BOUND = PLANE_MARGIN * PLANE_NORMAL_MEASURED
PLANE_SOUP_NORMAL_BOUND = PLANE_MARGIN * PLANE_SOUP_NORMAL_MEASURED
# vertices[faces[:, [0, 2, 1]]] against the soup, corner for corner: the two paths interpolate a shared edge from different ends.  The
# largest difference over every case of VOLUME_CASES (weld_keep() says which vertices it speaks about), in ulps of the case's largest
# coordinate; margin 2.
WELD_MARGIN = 2.0
WELD_ULPS_MEASURED = 1.0
WELD_ULPS_BOUND = WELD_MARGIN * WELD_ULPS_MEASURED


def _grid(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def _volume(f, w=None):
    w = np.ones_like(f) if w is None else w
    return np.ascontiguousarray(np.stack([f, w], -1).astype(F))


def _random(dims, seed, unobserved=0.02):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    return _volume(rng.uniform(-1, 1, (Z, Y, X)), rng.uniform(0, 1, (Z, Y, X)) > unobserved)


def coords(i, dims):
    X, Y, _ = dims
    return int(i % X), int((i // X) % Y), int(i // (X * Y))


def dims_of(vol):
    Z, Y, X = vol.shape[:3]
    return X, Y, Z


def chunk_of(index):
    return np.asarray(index, np.int64) // CHUNK


# ---- volume cases: name -> (vol, size, R, t) ----------------------------------------------------------------------------------------
def _carry():
    """1120 chunks: two slabs of scan_blocks.  A clipped tilted plane that crosses every z layer, so the chunks past 1024 hold cells"""
    dims = (64, 64, 560)
    x, y, z = _grid(dims)
    f = np.clip((0.31 * x + y + 0.017 * z - (dims[1] / 2 + 5.3)) / 4, -1, 1)
    return _volume(f), MI.SIZE, MI.POSE_R, MI.POSE_T


def _plane():
    x, y, z = _grid(PLANE_DIMS)
    f = np.clip((PLANE_N[0] * x + PLANE_N[1] * y + PLANE_N[2] * z - PLANE_D) / 4, -1, 1)
    return _volume(f), MI.SIZE, MI.POSE_R, MI.POSE_T


def seam_owner_cell(i, dims):
    """a cell that shares the +x edge of voxel i (the voxel itself unless it lies on the top y or z layer), as a flat index"""
    X, Y, Z = dims
    x, y, z = coords(i, dims)
    assert x + 1 < X
    cy, cz = (y - 1 if y == Y - 1 else y), (z - 1 if z == Z - 1 else z)
    return (cz * Y + cy) * X + x


def _seam(dims, kind):
    """Random TSDF, about 2 % unobserved.  Where the volume has a voxel 2049: the +x edges of voxels 2047 and 2048 (the last of chunk 0,
    the first of chunk 1) are cut, and `own` observes every corner of a cell on each so that both carry a vertex, referenced by faces of
    chunk 0; `unobs` then marks voxel 2048 unobserved, which silences cells of chunk 0 through a corner that lies in chunk 1."""
    vol = _random(dims, 1000 * dims[0] + dims[1]).copy()
    X, Y, Z = dims
    if X * Y * Z > CHUNK + 1:
        flat = vol.reshape(-1, 2)
        flat[CHUNK - 1, 0], flat[CHUNK, 0], flat[CHUNK + 1, 0] = -0.6, 0.7, -0.4
        for i in (CHUNK - 1, CHUNK):
            x, y, z = coords(seam_owner_cell(i, dims), dims)
            vol[z:z + 2, y:y + 2, x:x + 2, 1] = 1.0
        if kind == "unobs":
            flat[CHUNK, 1] = 0.0
    return vol, MI.SIZE, MI.POSE_R, MI.POSE_T


def _tiny(dims):
    X, Y, Z = dims
    rng = np.random.default_rng(X + 10 * Y + 100 * Z)
    return _volume(rng.uniform(-1, 1, (Z, Y, X))), MI.SIZE, MI.POSE_R, MI.POSE_T


def _degenerate(nan):
    """Values on which only the sign rule f < 0, the 1e-15f guard of interp, len2 > 0 and the device's subnormals decide.  Unit cells and
    the identity pose: a vertex on a grid node is there exactly.  `nan`: uniform noise with the degenerate values and NaN sprinkled in"""
    X, Y, Z = DEGENERATE_DIMS
    rng = np.random.default_rng(29 + nan)
    vals = np.array(DEGENERATE_VALUES, F)
    f = vals[rng.integers(0, len(vals), (Z, Y, X))]
    w = rng.uniform(0, 1, (Z, Y, X)) > 0.03
    if nan:
        noise = rng.uniform(-1, 1, (Z, Y, X)).astype(F)
        f = np.where(rng.uniform(0, 1, (Z, Y, X)) < 0.7, noise, f)
        f[rng.uniform(0, 1, (Z, Y, X)) < 0.02] = np.nan
    return _volume(f, w), tuple(float(v) for v in DEGENERATE_DIMS), IDENTITY[0], IDENTITY[1]


def _name(prefix, dims):
    return prefix + "_" + "x".join(str(v) for v in dims)


BUILDERS = {"carry": _carry, "plane": _plane, "degenerate": functools.partial(_degenerate, 0), "degenerate_nan": functools.partial(_degenerate, 1)}
for _d in SEAM_DIMS:
    BUILDERS[_name("seam", _d) + "_own"] = functools.partial(_seam, _d, "own")
    if _d[0] * _d[1] * _d[2] > CHUNK + 1:
        BUILDERS[_name("seam", _d) + "_unobs"] = functools.partial(_seam, _d, "unobs")
for _d in TINY_DIMS:
    BUILDERS[_name("tiny", _d)] = functools.partial(_tiny, _d)
for _d in FLAT_DIMS:
    BUILDERS[_name("flat", _d)] = functools.partial(_tiny, _d)
VOLUME_CASES = tuple(BUILDERS)
SEAM_CASES = tuple(n for n in VOLUME_CASES if n.startswith("seam_"))
FLAT_CASES = tuple(n for n in VOLUME_CASES if n.startswith("flat_"))
NAN_CASES = ("degenerate_nan",)


@functools.lru_cache(maxsize=None)
def case(name):
    """(vol (Z, Y, X, 2) float32, volume size, R, t) of a volume case"""
    vol, size, R, t = BUILDERS[name]()
    vol.setflags(write=False)
    return vol, size, R, t


def _oracle():
    import oracle as O

    O.build()
    return O


@functools.lru_cache(maxsize=None)
def reference(name):
    """The references of a volume case -> dict: count (active cells), occ (3, count) int32 (voxel index, vertex count, vertex offset),
    total (soup vertices), soup_v / soup_n (total, 4) from the oracle; indexed: the restatement's dict"""
    O = _oracle()
    vol, size, R, t = case(name)
    m = MI.marching_cubes_indexed(vol, size, R, t)
    cap = m["active"] + 3
    occ, count = O.mc_occupied_voxels(vol, cap)
    total = O.mc_offsets(occ, count)
    soup_v, soup_n = O.marching_cubes(vol, size, R, t, max_voxels=cap, max_vertices=total + 3)
    return dict(count=count, occ=occ[:, :count].copy(), total=total, soup_v=soup_v, soup_n=soup_n, indexed=m)


def vertex_owners(mask):
    """(owner voxel, axis) of every welded vertex, in vertex order: owners ascending, then axis"""
    flat = mask.reshape(-1).astype(np.int64)
    owners, axes = np.repeat(np.arange(flat.size), 3), np.tile(np.arange(3), flat.size)
    sel = ((flat[owners] >> axes) & 1) == 1
    return owners[sel], axes[sel]


def vertex_edge_values(name):
    """(fa, fb): the TSDF at the owner and at the far end of every welded vertex's edge"""
    vol = case(name)[0]
    X, Y, _ = dims_of(vol)
    owners, axes = vertex_owners(reference(name)["indexed"]["mask"])
    ff = vol[..., 0].reshape(-1)
    return ff[owners], ff[owners + np.where(axes == 0, 1, np.where(axes == 1, X, X * Y))]


def weld_error_ulps(soup_v, vertices, faces, keep=None):
    """vertices[faces[:, [0, 2, 1]]] against the soup triangles corner for corner -> the largest coordinate difference in ulps of the
    mesh's largest coordinate (0 for an empty mesh).  `keep`: per welded vertex, False drops the corners that use it"""
    if len(faces) == 0:
        return 0.0
    got = vertices[faces[:, [0, 2, 1]]][:, :, :3].astype(np.float64)
    want = soup_v.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    ok = np.ones(faces.shape, bool) if keep is None else keep[faces[:, [0, 2, 1]]]
    if not ok.any():
        return 0.0
    unit = float(np.spacing(F(max(np.abs(want[ok]).max(), np.abs(got[ok]).max()))))
    return float(np.abs(got - want)[ok].max()) / unit


def weld_keep(name):
    """The welded vertices the soup-against-indexed bound speaks about: finite ones whose edge is not decided by interp's 1e-15f guard.
    With |fb - fa| far below 1e-15 each end's walk stays at its own end: the two paths then differ by a whole cell, by their rule."""
    fa, fb = vertex_edge_values(name)
    with np.errstate(invalid="ignore"):
        return np.isfinite(fa) & np.isfinite(fb) & (np.abs(fb.astype(np.float64) - fa) > 1e-9)


# ---- the closed form of `plane` -------------------------------------------------------------------------------------------------------
def cell_sizes(size, dims):
    return np.array([F(F(size[i]) / F(dims[i])) for i in range(3)], np.float64)


def unpose(v, R, t):
    """float64 volume coordinates of float4 vertices (x, -y, -z, 1) under the pose"""
    return np.linalg.solve(np.asarray(R, np.float64), (v[:, :3].astype(np.float64) * FLIP - np.asarray(t, np.float64)).T).T


def plane_residual(v):
    """the largest distance of the vertices `v` (N, 4) of `plane` from the plane, in grid units, float64"""
    _, size, R, t = case("plane")
    g = unpose(v, R, t) / cell_sizes(size, PLANE_DIMS) - 0.5  # get_node_coo: node x sits at (x + 0.5) cs
    n = np.array(PLANE_N)
    return float(np.abs(g @ n - PLANE_D).max() / np.linalg.norm(n))


def plane_unit_normal():
    """normalize(n / cs): the direction of the TSDF gradient in metric volume coordinates"""
    _, size, _, _ = case("plane")
    g = np.array(PLANE_N) / cell_sizes(size, PLANE_DIMS)
    return g / np.linalg.norm(g)


def plane_indexed_normal_error(n):
    _, _, R, _ = case("plane")
    want = (np.asarray(R, np.float64) @ plane_unit_normal()) * FLIP
    return float(np.abs(n[:, :3].astype(np.float64) - want).max())


def plane_soup_normal_error(n):
    """-> (largest component error of the finite soup normals against the flipped, unrotated unit normal, number of finite normals);
    the error of a normal that points the other way is near 2"""
    want = plane_unit_normal() * FLIP
    fin = np.isfinite(n[:, :3]).all(1)
    return float(np.abs(n[fin, :3].astype(np.float64) - want).max()), int(fin.sum())


# ---- caps ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def caps_volume():
    vol = MI.case_volume(None, "random")
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def caps_counts():
    """(active cells, soup vertices) of the caps volume, uncapped"""
    O = _oracle()
    occ, count = O.mc_occupied_voxels(caps_volume(), caps_volume()[..., 0].size)
    return count, O.mc_offsets(occ, count)


def caps_max_voxels():
    count, _ = caps_counts()
    return (1, count - 1, count, count + 1)


def caps_max_vertices():
    _, total = caps_counts()
    return (3, 4, 5, total - 1, total, total + 1)


CAPS_EXTRA_STRIDE = 37


@functools.lru_cache(maxsize=None)
def caps_reference(max_voxels, max_vertices=None):
    """The oracle on the caps volume under the caps -> dict: count, occ (3, count), total (uncut by max_vertices), soup_v, soup_n (whole
    triangles below max_vertices; default: all of them)"""
    O = _oracle()
    vol = caps_volume()
    occ, count = O.mc_occupied_voxels(vol, max_voxels)
    total = O.mc_offsets(occ, count)
    v, n = O.marching_cubes(vol, MI.SIZE, MI.POSE_R, MI.POSE_T, max_voxels=max_voxels, max_vertices=total if max_vertices is None else max_vertices)
    return dict(count=count, occ=occ[:, :count].copy(), total=total, soup_v=v, soup_n=n)


# ---- synthetic mc_offsets inputs --------------------------------------------------------------------------------------------------------
OFFSET_COUNTS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, SLAB * CHUNK - 1, SLAB * CHUNK, SLAB * CHUNK + 1)
OFFSET_PAD, OFFSET_SENTINEL, OFFSET_BEYOND = 5, -7, 1_000_003


def offsets_input(count):
    """-> (occupied (3, count + OFFSET_PAD) int32, expected row 2 over [:count], expected total).  Row 1 holds vertex counts from
    {3, 6, 9, 12, 15} over [:count] and OFFSET_BEYOND past it (a scan that reads past `count` changes the total); rows 0 and 2 hold
    OFFSET_SENTINEL.  The expectation is numpy's int64 cumsum."""
    rng = np.random.default_rng(count)
    occ = np.full((3, count + OFFSET_PAD), OFFSET_SENTINEL, np.int32)
    occ[1, :count] = rng.choice(np.array([3, 6, 9, 12, 15], np.int32), count)
    occ[1, count:] = OFFSET_BEYOND
    incl = np.cumsum(occ[1, :count].astype(np.int64))
    assert incl[-1] < 2 ** 31
    return occ, (incl - occ[1, :count]).astype(np.int64), int(incl[-1])
