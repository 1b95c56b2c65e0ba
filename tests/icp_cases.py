"""The cases of tests/test_gpu_icp_edges.py and their restatement-side values, shared with tests/test_icp_cases_cpu.py (which shows on the
CPU that the cases are meaningful) and tests/test_gpu_icp.py: small, odd and pitched frames of the analytic scene of icp_reference.py,
the launch shape of the correspondence kernel for each, the sums check with its derived bound, the reference chain of an estimate, and
the frames of the failure tests.  Numpy only: nothing here needs a GPU.  Everything a function returns is cached and shared; treat it as
read-only."""
from __future__ import annotations

import functools
import math

import numpy as np

import icp_reference as IR

SIGMA = 0.04
DIST, ANGLE = 0.02, float(np.deg2rad(20.0))
TRUTH = IR.pose(IR.rot((0.3, 1.0, 0.2), 2.0), (0.012, -0.012, 0.0106))  # the second camera of the correspondence cases: 2 degrees, 2 cm
NEAR = IR.pose(IR.rot((0.2, 1.0, 0.1), 1.5), (0.008, -0.01, 0.007)).astype(np.float32)  # the pose of one pass: near, not at, the truth
SMALL = IR.pose(IR.rot((0.3, 1.0, 0.2), 0.5), (0.003, -0.003, 0.0025))  # the second camera of the estimates: every step of the chain solves

# name -> (rows, cols, (fx, fy, cx, cy)).  parts_of: 1, 3, 19, 34 workgroups
CASES = {
    "24x40": (24, 40, (64.0, 64.0, 19.5, 11.5)),      # one partly idle workgroup: lanes 192..255 hold 3 pixels, the others 4
    "33x67": (33, 67, (110.0, 110.0, 33.0, 16.0)),    # odd extents, a width above 64 that is no multiple of it, rows no multiple of 4
    "120x160": (120, 160, (260.0, 260.0, 80.0, 60.0)),  # 19 slabs
    "131x259": (131, 259, (420.0, 420.0, 129.0, 65.0)),  # 34 slabs, odd extents
}
MODES = ("points", "depth")
MARGIN = 1e-6  # a pixel whose decision lies closer than this to its threshold may fall either way
THREADS, MAX_PARTS = 256, 256

PLANE_INTR, PLANE_SHAPE, PLANE_MM = (64.0, 64.0, 32.0, 24.0), (48, 64), 800


def parts_of(rows, cols):
    """workgroups of one correspondence pass (icp_kernels.hip): at least 4 pixels per lane, at most MAX_PARTS"""
    return min(max((rows * cols + 4 * THREADS - 1) // (4 * THREADS), 1), MAX_PARTS)


def pixels_per_lane(rows, cols):
    """m: the most pixels one lane of the grid-stride loop visits"""
    return -(-(rows * cols) // (parts_of(rows, cols) * THREADS))


def level_intr(intr, level):
    return tuple(float(np.float32(np.float32(v) / np.float32(1 << level))) for v in intr)


@functools.lru_cache(maxsize=None)
def frames(name, motion="truth"):
    """(previous, current) depth of case `name`: the scene from the identity and from TRUTH (or SMALL)"""
    rows, cols, intr = CASES[name]
    return IR.render_depth(np.eye(4), intr, rows, cols), IR.render_depth(TRUTH if motion == "truth" else SMALL, intr, rows, cols)


@functools.lru_cache(maxsize=None)
def depth_levels(name, motion, levels):
    """((previous level 0, 1, ...), (current level 0, 1, ...)) depth pyramids"""
    out = []
    for d in frames(name, motion):
        dd = [d]
        for _ in range(1, levels):
            dd.append(IR.depth_pyramid(dd[-1], SIGMA))
        out.append(tuple(dd))
    return tuple(out)


def maps_of(depth, intr, level, mode):
    """(image, normals) of one frame at one level: (points, normals) or (masked depth, normals)"""
    li = level_intr(intr, level)
    return IR.point_normals(depth, li) if mode == "points" else IR.normals_mask_depth(depth, li)


@functools.lru_cache(maxsize=None)
def level_inputs(name, mode, level, motion="truth"):
    """(curr, ncurr, prev, nprev) of case `name` at pyramid level `level`"""
    intr = CASES[name][2]
    prev, curr = depth_levels(name, motion, level + 1)
    c, nc = maps_of(curr[level], intr, level, mode)
    p, np_ = maps_of(prev[level], intr, level, mode)
    return c, nc, p, np_


@functools.lru_cache(maxsize=None)
def reference_pass(name, mode, level):
    """(codes, masked rows, margins, unmasked rows) of the restatement at NEAR"""
    return IR.correspond(level, CASES[name][2], *level_inputs(name, mode, level), NEAR, DIST, ANGLE, unmasked=True)


def cap_of(margin):
    """the number of pixels whose code may differ: those with a decision closer than MARGIN to its threshold"""
    return int((margin < MARGIN).sum())


def sums_over(every, mask):
    """the 29 sums (fp32 products, fp64 sums) of the unmasked rows `every` over the pixels of `mask`, and the sums of their absolute values"""
    R = every[mask]
    terms = [R[:, i] * R[:, j] for i in range(6) for j in range(i, 6)] + [R[:, i] * R[:, 6] for i in range(6)]
    terms += [np.ones(len(R), np.float32), R[:, 6] * R[:, 6]]
    T = np.stack(terms, 0).astype(np.float64)
    return T.sum(1), np.abs(T).sum(1)


def pack(A, b, count, rms):
    """the 29 values of ops.icp_step's result, in the kernel's order"""
    return np.concatenate([np.asarray(A)[np.triu_indices(6)], b, [count, (rms ** 2) * count]])


def sums_error(got, s, sabs, rows, cols, parts=None):
    """Checks 29 sums `got` against the reference's (s, sabs) of a rows x cols pass; -> the largest error as a fraction of its bound.
    The count must be equal; every other value within (m + 10) 2^-24 sabs: the fp32 products are the same on both sides, and a value
    reaches its slab through at most m - 1 roundings in the lane, 6 in the wave butterfly and 3 across the waves, each at most 2^-24 of
    the sum of the absolute terms; the fp64 stage adds less than one more unit."""
    parts = parts_of(rows, cols) if parts is None else parts
    m = -(-(rows * cols) // (parts * THREADS))
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), got
    assert got[27] == s[27], (got[27], s[27])
    bound = (m + 10) * 2.0 ** -24 * sabs
    err = np.abs(got - s)
    k = np.delete(np.arange(29), 27)
    assert (err[k] <= bound[k]).all(), (err[k] / np.maximum(bound[k], 1e-300)).max()
    return float((err[k] / np.maximum(bound[k], 1e-300)).max())


def check_pass(got_codes, got29, ref, rows, cols, cap=None):
    """One correspondence pass against the restatement `ref` = (codes, rows, margins, unmasked rows): the codes agree except at marginal
    pixels, at most `cap` of them (default: the number of marginal pixels), and the sums -- ALWAYS -- match the reference's rows summed
    over the inlier mask of `got_codes` (the differing pixels, shown marginal, follow that decision).
    -> (differing pixels, the largest sums error as a fraction of its bound)"""
    rcodes, _, margin, every = ref
    differ = got_codes != rcodes
    assert (margin[differ] < MARGIN).all(), (int(differ.sum()), np.unique(got_codes[differ]), np.unique(rcodes[differ]))
    assert differ.sum() <= (cap_of(margin) if cap is None else cap), int(differ.sum())
    s, sabs = sums_over(every, got_codes == 0)
    return int(differ.sum()), sums_error(got29, s, sabs, rows, cols)


# ---- the estimate's reference chain -------------------------------------------------------------------------------------------------
def launch_levels(iters):
    """the level of every launch of an estimate with budgets `iters` (finest first): coarse to fine"""
    return [l for l in range(len(iters) - 1, -1, -1) for _ in range(iters[l])]


@functools.lru_cache(maxsize=None)
def reference_chain(name, mode, iters, motion="small"):
    """The restatement's estimate of case `name`: a list of (level, inliers, cond(A), solved, pose after) per launch"""
    intr = CASES[name][2]
    aff = np.eye(4, dtype=np.float32)
    out = []
    for level in launch_levels(iters):
        codes, row, _ = IR.correspond(level, intr, *level_inputs(name, mode, level, motion), aff, DIST, ANGLE)
        s, _ = IR.sums(row, codes)
        A, b = IR.unpack(s)
        with np.errstate(all="ignore"):
            ok, x = IR.solve(A, b)
        if ok:
            aff = IR.compose(x, aff)
        out.append((level, int(s[27]), float(np.linalg.cond(A)) if np.isfinite(A).all() else math.inf, ok, aff.copy()))
        if not ok:
            break
    return out


def ulps(a, b):
    """the distance of float32 arrays in units in the last place (on the ordered integers of the format; +0 and -0 coincide)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---- frames of the failure tests ------------------------------------------------------------------------------------------------------
def plane(shape=PLANE_SHAPE):
    """a fronto-parallel plane: every normal is (0, 0, -1), so the rotation about z is unobservable and A_22 is exactly 0"""
    return np.full(shape, PLANE_MM, np.uint16)


@functools.lru_cache(maxsize=None)
def plane_levels(levels, shape=PLANE_SHAPE):
    dd = [plane(shape)]
    for _ in range(1, levels):
        dd.append(IR.depth_pyramid(dd[-1], SIGMA))
    return tuple(dd)


@functools.lru_cache(maxsize=None)
def edge_depth():
    """A 22 x 26 depth image of 0, 1, 46341 (the first depth whose square exceeds INT_MAX), 65535 and values 119, 120 and 121 mm apart
    (3 sigma = 120 is the pyramid's strict threshold) next to each other, with a few blocks set by hand"""
    rng = np.random.default_rng(7)
    vals = np.array([0, 1, 46341, 65535, 1000, 1119, 1120, 1121, 46221, 46222, 65415, 65416, 46461], np.uint16)
    d = vals[rng.integers(0, len(vals), (22, 26))]
    d[0:2, 0:2] = 46341                       # d00 * d01 = 2147488281 > INT_MAX
    d[2:4, 0:2] = 65535                       # the largest product and sum
    d[4:6, 0:2] = [[65535, 46341], [0, 65535]]  # one hole among overflowing products
    d[6:8, 0:2] = [[1, 1], [1, 2]]            # sum / 4 truncates to 1
    d[8, 2:7] = [1121, 1120, 1000, 1119, 1000]  # around the centre (8, 4): 119 qualifies, 120 and 121 do not
    return d


@functools.lru_cache(maxsize=None)
def sparse_frame(name="24x40", motion="small"):
    """(points, normals) of the current frame with everything but one 2 x 2 patch invalid: four inliers at the most"""
    c, nc, _, _ = level_inputs(name, "points", 0, motion)
    ok = IR.valid(c, nc)
    full = ok[:-1, :-1] & ok[1:, :-1] & ok[:-1, 1:] & ok[1:, 1:]
    ys, xs = np.nonzero(full)
    k = len(ys) // 2
    y, x = int(ys[k]), int(xs[k])
    p, n = np.full_like(c, np.nan), np.full_like(nc, np.nan)
    p[y:y + 2, x:x + 2], n[y:y + 2, x:x + 2] = c[y:y + 2, x:x + 2], nc[y:y + 2, x:x + 2]
    return p, n


# ---- validity conventions ------------------------------------------------------------------------------------------------------------
PATCH_ROWS, PATCH = (28, 48, 68, 88), 8  # four 8 x 8 patches per frame: current frame at column 44, previous frame at column 104
CURR_COL, PREV_COL = 44, 104


def _spoil(p, n, col):
    for kind, y in enumerate(PATCH_ROWS):
        win = (slice(y, y + PATCH), slice(col, col + PATCH))
        if kind == 0:    # a raycaster miss: point and normal all zero
            p[win], n[win] = 0, 0
        elif kind == 1:  # +Inf in one component of the point
            p[win + (1,)] = np.inf
        elif kind == 2:  # a zero normal with a finite point
            n[win + (slice(0, 3),)] = 0
        else:            # a NaN normal with a finite point
            n[win + (slice(0, 3),)] = np.nan


@functools.lru_cache(maxsize=None)
def validity_inputs(name="120x160"):
    """(curr, ncurr, prev, nprev, current patch mask, previous patch mask): the points-mode inputs of `name` with disjoint patches of
    both frames overwritten by the four kinds of invalid pixel"""
    c, nc, p, np_ = (a.copy() for a in level_inputs(name, "points", 0))
    _spoil(c, nc, CURR_COL)
    _spoil(p, np_, PREV_COL)
    cm, pm = np.zeros(c.shape[:2], bool), np.zeros(c.shape[:2], bool)
    for y in PATCH_ROWS:
        cm[y:y + PATCH, CURR_COL:CURR_COL + PATCH] = True
        pm[y:y + PATCH, PREV_COL:PREV_COL + PATCH] = True
    return c, nc, p, np_, cm, pm


@functools.lru_cache(maxsize=None)
def validity_reference(name="120x160"):
    c, nc, p, np_, _, _ = validity_inputs(name)
    return IR.correspond(0, CASES[name][2], c, nc, p, np_, NEAR, DIST, ANGLE, unmasked=True)
