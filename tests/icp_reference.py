"""Numpy restatement of the camera-tracking rules of sobfu_amd/csrc/icp_kernels.hip (image pyramids, point / normal maps, projective ICP
correspondences, rows and sums, the fp64 solve), in float32 with the kernels' operation order, and an analytic depth renderer of a scene
that pins all six degrees of freedom: a slab, a box standing on it and a sphere, inside config 1's 0.5 m volume."""
from __future__ import annotations

import numpy as np

f32 = np.float32

# the scene, in the frame of the first camera (metres): config 1's volume spans x, y in [-0.25, 0.25], z in [0.5, 1.0]
SLAB = ((-0.23, -0.23, 0.88), (0.23, 0.23, 0.95))
BOX = ((-0.16, -0.12, 0.72), (-0.02, 0.06, 0.88))
SPHERE = ((0.09, 0.04, 0.80), 0.07)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(R=np.eye(3), t=(0, 0, 0)):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


def render_depth(cam_pose, intr, rows=480, cols=640):
    """uint16 mm depth of the scene seen by a camera whose pose (4 x 4, camera -> scene frame) is cam_pose; float64, rint; 0 = miss"""
    fx, fy, cx, cy = (float(v) for v in intr)
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)  # camera-frame ray, z = 1: the parameter is the depth
    R, o = cam_pose[:3, :3], cam_pose[:3, 3]
    d = dc @ R.T
    best = np.full(u.shape, np.inf)
    for lo, hi in (SLAB, BOX):
        t0, t1 = np.full(u.shape, -np.inf), np.full(u.shape, np.inf)
        for k in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                a, b = (lo[k] - o[k]) / d[..., k], (hi[k] - o[k]) / d[..., k]
            t0, t1 = np.maximum(t0, np.minimum(a, b)), np.minimum(t1, np.maximum(a, b))
        hit = (t0 <= t1) & (t0 > 0)
        best = np.where(hit & (t0 < best), t0, best)
    c, r = np.asarray(SPHERE[0]), SPHERE[1]
    oc = o - c
    A = (d * d).sum(-1)
    B = 2.0 * (d @ oc)
    Cc = oc @ oc - r * r
    disc = B * B - 4 * A * Cc
    ts = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
    best = np.where((ts > 0) & (ts < best), ts, best)
    return np.where(np.isfinite(best), np.rint(best * 1000.0), 0).astype(np.uint16)


# ---- image rules -----------------------------------------------------------------------------------------------------------------
def depth_pyramid(src, sigma_depth):
    src = np.asarray(src).astype(np.int64)
    rows, cols = src.shape
    dr, dc = rows // 2, cols // 2
    thr = f32(f32(sigma_depth) * f32(1000.0)) * f32(3.0)
    yy, xx = np.meshgrid(np.arange(dr), np.arange(dc), indexing="ij")
    centre = src[2 * yy, 2 * xx]
    s, n = np.zeros((dr, dc), np.int64), np.zeros((dr, dc), np.int64)
    for oy in range(-2, 3):
        for ox in range(-2, 3):
            cy, cx = 2 * yy + oy, 2 * xx + ox
            inside = (cy >= 0) & (cy < rows - 1) & (cx >= 0) & (cx < cols - 1)
            val = src[np.clip(cy, 0, rows - 1), np.clip(cx, 0, cols - 1)]
            ok = inside & (np.abs(val - centre).astype(np.float32) < thr)
            s += np.where(ok, val, 0)
            n += ok
    return np.where(n == 0, 0, s // np.maximum(n, 1)).astype(np.uint16)


def level_intr(intr, level):
    div = f32(1 << level)
    fx, fy, cx, cy = (f32(f32(v) / div) for v in intr)
    return fx, fy, cx, cy, f32(f32(1) / fx), f32(f32(1) / fy)


def reproject(li, u, v, z):
    fx, fy, cx, cy, fxi, fyi = li
    u, v, z = (np.asarray(a, np.float32) for a in (u, v, z))
    return (z * (u - cx)) * fxi, (z * (v - cy)) * fyi, z


def _normals(depth, intr):
    d = np.asarray(depth).astype(np.float32) * f32(0.001)
    rows, cols = d.shape
    li = level_intr(intr, 0)
    y, x = np.meshgrid(np.arange(rows, dtype=np.float32), np.arange(cols, dtype=np.float32), indexing="ij")
    z00 = d
    z01 = np.concatenate([d[:, 1:], np.zeros((rows, 1), np.float32)], 1)
    z10 = np.concatenate([d[1:], np.zeros((1, cols), np.float32)], 0)
    ok = (z00 * z01 * z10 != 0)
    ok[-1, :] = False
    ok[:, -1] = False
    v00 = reproject(li, x, y, z00)
    v01 = reproject(li, x + f32(1), y, z01)
    v10 = reproject(li, x, y + f32(1), z10)
    ax, ay, az = (v01[k] - v00[k] for k in range(3))
    bx, by, bz = (v10[k] - v00[k] for k in range(3))
    cx_, cy_, cz_ = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(cx_ * cx_ + cy_ * cy_ + cz_ * cz_)
        n = np.stack([-(cx_ / ln), -(cy_ / ln), -(cz_ / ln), np.zeros_like(ln)], -1)
    p = np.stack([v00[0], v00[1], v00[2], np.zeros_like(z00)], -1)
    return ok, p, n


def point_normals(depth, intr):
    ok, p, n = _normals(depth, intr)
    nan = np.float32(np.nan)
    return np.where(ok[..., None], p, nan).astype(np.float32), np.where(ok[..., None], n, nan).astype(np.float32)


def normals_mask_depth(depth, intr):
    ok, _, n = _normals(depth, intr)
    nrm = np.where(ok[..., None], n, np.float32(np.nan)).astype(np.float32)
    nrm[~ok, 3] = 0
    d = np.where(np.isnan(nrm[..., 0]), 0, depth).astype(np.uint16)
    return d, nrm


def _avg4(a, b, c, d):
    s = ((a + b) + c) + d
    out = s * f32(0.25)
    out[..., 3] = 0
    return out


def valid(p, n):
    fin = np.isfinite(p[..., :3]).all(-1) & np.isfinite(n[..., :3]).all(-1)
    with np.errstate(invalid="ignore"):
        return fin & (n[..., :3] != 0).any(-1)


def resize_depth_normals(depth, normals):
    d = np.asarray(depth).astype(np.int64)
    rows, cols = d.shape
    dr, dc = rows // 2, cols // 2
    q = lambda a, oy, ox: a[oy:2 * dr:2, ox:2 * dc:2]
    d00, d01, d10, d11 = q(d, 0, 0), q(d, 0, 1), q(d, 1, 0), q(d, 1, 1)
    ok = (d00 * d01 != 0) & (d10 * d11 != 0)
    dd = np.where(ok, (d00 + d01 + d10 + d11) // 4, 0).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        n = _avg4(q(normals, 0, 0), q(normals, 0, 1), q(normals, 1, 0), q(normals, 1, 1))
    n = np.where(ok[..., None], n, np.float32(np.nan)).astype(np.float32)
    return dd, n


def resize_points_normals(points, normals):
    rows, cols = points.shape[:2]
    dr, dc = rows // 2, cols // 2
    q = lambda a, oy, ox: a[oy:2 * dr:2, ox:2 * dc:2]
    ok = np.ones((dr, dc), bool)
    for oy in (0, 1):
        for ox in (0, 1):
            ok &= valid(q(points, oy, ox), q(normals, oy, ox))
    with np.errstate(invalid="ignore"):
        p = _avg4(q(points, 0, 0), q(points, 0, 1), q(points, 1, 0), q(points, 1, 1))
        n = _avg4(q(normals, 0, 0), q(normals, 0, 1), q(normals, 1, 0), q(normals, 1, 1))
    nan = np.float32(np.nan)
    return np.where(ok[..., None], p, nan).astype(np.float32), np.where(ok[..., None], n, nan).astype(np.float32)


# ---- ICP ------------------------------------------------------------------------------------------------------------------------
def correspond(level, intr, curr, ncurr, prev, nprev, aff, dist, angle, unmasked=False):
    """-> (codes (rows, cols) uint8, rows (rows, cols, 7) float32 (zero where code != 0), margins (rows, cols): the smallest relative
    distance of a decision of the pixel from its threshold); with unmasked also the rows of every pixel, whatever its code (the row a
    pixel would contribute were it an inlier; not finite where the pixel or its target is invalid)"""
    depth = np.asarray(curr).ndim == 2
    li = level_intr(intr, level)
    fx, fy, cx, cy = li[:4]
    rows, cols = ncurr.shape[:2]
    aff = np.asarray(aff, np.float32).reshape(4, 4)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    codes = np.zeros((rows, cols), np.uint8)
    margin = np.full((rows, cols), np.inf)
    with np.errstate(all="ignore"):
        if depth:
            zc = np.asarray(curr)
            ok = (zc != 0) & valid(np.zeros_like(ncurr), ncurr)
            s0 = reproject(li, x.astype(np.float32), y.astype(np.float32), zc.astype(np.float32) * f32(0.001))
        else:
            ok = valid(curr, ncurr)
            s0 = (curr[..., 0], curr[..., 1], curr[..., 2])
        codes[~ok] = 40
        s = [((aff[r, 0] * s0[0] + aff[r, 1] * s0[1]) + aff[r, 2] * s0[2]) + aff[r, 3] for r in range(3)]
        u = fx * (s[0] / s[2]) + cx
        v = fy * (s[1] / s[2]) + cy
        bad = (s[2] <= 0) | (u < 0) | (v < 0) | (u >= f32(cols)) | (v >= f32(rows))
        ui = np.floor(u + f32(0.5))
        vi = np.floor(v + f32(0.5))
        bad |= (ui >= cols) | (vi >= rows)
        bad |= ~np.isfinite(ui) | ~np.isfinite(vi)
        live = (codes == 0)
        codes[live & bad] = 80
        # margins of the rounding decision: distance of u + 0.5 from an integer
        fr = np.minimum(np.abs(u + f32(0.5) - np.round(u + f32(0.5))), np.abs(v + f32(0.5) - np.round(v + f32(0.5))))
        margin = np.where(live, np.minimum(margin, fr / np.maximum(1.0, np.abs(u) + np.abs(v))), margin)
        uic = np.clip(np.nan_to_num(ui, nan=0), 0, cols - 1).astype(np.int64)
        vic = np.clip(np.nan_to_num(vi, nan=0), 0, rows - 1).astype(np.int64)
        n4 = nprev[vic, uic]
        if depth:
            zp = np.asarray(prev)[vic, uic]
            tok = (zp != 0) & valid(np.zeros_like(n4), n4)
            d = reproject(li, u, v, zp.astype(np.float32) * f32(0.001))
        else:
            p4 = prev[vic, uic]
            tok = valid(p4, n4)
            d = (p4[..., 0], p4[..., 1], p4[..., 2])
        live = (codes == 0)
        codes[live & ~tok] = 120
        nd = (n4[..., 0], n4[..., 1], n4[..., 2])
        dx, dy, dz = s[0] - d[0], s[1] - d[1], s[2] - d[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2t = f32(dist) * f32(dist)
        live = (codes == 0)
        codes[live & (d2 > d2t)] = 160
        margin = np.where(live, np.minimum(margin, np.abs(d2 - d2t) / d2t), margin)
        nsv = [(aff[r, 0] * ncurr[..., 0] + aff[r, 1] * ncurr[..., 1]) + aff[r, 2] * ncurr[..., 2] for r in range(3)]
        cosv = np.abs((nsv[0] * nd[0] + nsv[1] * nd[1]) + nsv[2] * nd[2])
        mc = f32(np.cos(np.float64(f32(angle))))
        live = (codes == 0)
        codes[live & (cosv < mc)] = 200
        margin = np.where(live, np.minimum(margin, np.abs(cosv - mc)), margin)
        r = (nd[0] * (d[0] - s[0]) + nd[1] * (d[1] - s[1])) + nd[2] * (d[2] - s[2])
        row = np.stack([s[1] * nd[2] - s[2] * nd[1], s[2] * nd[0] - s[0] * nd[2], s[0] * nd[1] - s[1] * nd[0], nd[0], nd[1], nd[2], r], -1)
    every = row.astype(np.float32)
    row = np.where((codes == 0)[..., None], row, 0).astype(np.float32)
    return (codes, row, margin, every) if unmasked else (codes, row, margin)


def sums(row, codes):
    """the 29 sums (fp32 products, fp64 sums) and the sums of their terms' absolute values"""
    m = codes == 0
    R = row[m]
    terms = [R[:, i] * R[:, j] for i in range(6) for j in range(i, 6)] + [R[:, i] * R[:, 6] for i in range(6)]
    terms += [np.ones(len(R), np.float32), R[:, 6] * R[:, 6]]
    T = np.stack(terms, 0).astype(np.float64)
    return T.sum(1), np.abs(T).sum(1)


def unpack(s):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, np.asarray(s[21:27], np.float64)


def solve(A, b):
    """LDL^T in fp64 -> (ok, x)"""
    L, D = np.zeros((6, 6)), np.zeros(6)
    det, ok = 1.0, True
    for c in range(6):
        dc = A[c, c]
        for k in range(c):
            dc -= L[c, k] * L[c, k] * D[k]
        D[c] = dc
        det *= dc
        ok = ok and dc > 0
        for r in range(c + 1, 6):
            a = A[r, c]
            for k in range(c):
                a -= L[r, k] * L[c, k] * D[k]
            L[r, c] = a / dc
    if not (abs(det) >= 1e-15) or not ok:
        return False, None
    x = np.zeros(6)
    for r in range(6):
        y = b[r]
        for k in range(r):
            y -= L[r, k] * x[k]
        x[r] = y
    x = x / D
    for r in range(5, -1, -1):
        y = x[r]
        for k in range(r + 1, 6):
            y -= L[k, r] * x[k]
        x[r] = y
    return True, x


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        return np.eye(3)
    k = w / th
    c, s = np.cos(th), np.sin(th)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * K


def compose(x, aff):
    """aff' = (Rodrigues(x0..2), x3..5) * aff in fp64, rounded to float32"""
    T = pose(rodrigues(x[:3]), x[3:])
    return (T @ np.asarray(aff, np.float64)).astype(np.float32)


def rot_angle_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))
