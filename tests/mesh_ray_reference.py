"""numpy restatement of the ray-triangle rule of sobfu_amd/csrc/sobfu_mesh_ray.hpp (ray_setup, ray_triangle: operation by operation, in
float32), of the brute-force answer of sobfu_amd/csrc/mesh_ray_kernels.hip -- per ray the minimum t over all triangles, the lowest
triangle index attaining it, its barycentrics and side -- and of the camera entry's ray generation and output rules (render).
dtype=np.float64 gives the float64 twin: the same operations in double, without the recomputation of zero edge functions."""
import numpy as np

import mesh_distance_reference as MD

indexed_soup = MD.indexed_soup
icosphere = MD.icosphere


def _pick(v, k):
    """v (..., 3), k broadcastable to v.shape[:-1] -> v[..., k]"""
    k = np.broadcast_to(k, v.shape[:-1])
    return np.take_along_axis(v, k[..., None], -1)[..., 0]


def ray_setup(origins, dirs, dtype=np.float32):
    """-> dict(o (n, 3), kx, ky, kz (n,), Sx, Sy, Sz (n,), valid (n,))"""
    o = np.asarray(origins)[:, :3].astype(dtype)
    d = np.asarray(dirs)[:, :3].astype(dtype)
    ad = np.abs(d)
    kz = np.where(ad[:, 1] > ad[:, 0], 1, 0)
    kz = np.where(ad[:, 2] > np.fmax(ad[:, 0], ad[:, 1]), 2, kz)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    with np.errstate(all="ignore"):
        dz = _pick(d, kz)
        kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
        Sx, Sy, Sz = _pick(d, kx) / dz, _pick(d, ky) / dz, dtype(1) / dz
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.fmax(np.fmax(ad[:, 0], ad[:, 1]), ad[:, 2]) > 0) & np.isfinite(Sz)
    return dict(o=o, kx=kx, ky=ky, kz=kz, Sx=Sx.astype(dtype), Sy=Sy.astype(dtype), Sz=Sz.astype(dtype), valid=valid)


def ray_triangle(ray, a, b, c, t_min, t_max, dtype=np.float32, parts=False):
    """rays (n) against corners a, b, c (T, 3) -> t (n, T) (+Inf: a miss), u, v (n, T), side (n, T) int8.  parts=True also returns the
    edge functions (U, V, W)."""
    a, b, c = (np.asarray(x, dtype)[None] for x in (a, b, c))
    o = ray["o"][:, None, :]
    kx, ky, kz = (ray[k][:, None] for k in ("kx", "ky", "kz"))
    Sx, Sy, Sz = (ray[k][:, None] for k in ("Sx", "Sy", "Sz"))
    with np.errstate(all="ignore"):
        A, B, C = a - o, b - o, c - o
        Akz, Bkz, Ckz = _pick(A, kz), _pick(B, kz), _pick(C, kz)
        Ax, Ay = _pick(A, kx) - Sx * Akz, _pick(A, ky) - Sy * Akz
        Bx, By = _pick(B, kx) - Sx * Bkz, _pick(B, ky) - Sy * Bkz
        Cx, Cy = _pick(C, kx) - Sx * Ckz, _pick(C, ky) - Sy * Ckz
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        if dtype == np.float32:
            z = (U == 0) | (V == 0) | (W == 0)
            if z.any():
                ax, ay, bx, by, cx, cy = (np.broadcast_to(x, z.shape)[z].astype(np.float64) for x in (Ax, Ay, Bx, By, Cx, Cy))
                U, V, W = U.copy(), V.copy(), W.copy()
                U[z], V[z], W[z] = (cx * by - cy * bx).astype(dtype), (ax * cy - ay * cx).astype(dtype), (bx * ay - by * ax).astype(dtype)
        inside = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        det = (U + V) + W
        Az, Bz, Cz = Sz * Akz, Sz * Bkz, Sz * Ckz
        T = (U * Az + V * Bz) + W * Cz
        t = T / det
        hit = inside & (det != 0) & (t > dtype(t_min)) & (t <= dtype(t_max)) & ray["valid"][:, None]
        t = np.where(hit, t, np.inf).astype(dtype)
        u = np.where(hit, V / det, 0).astype(dtype)
        v = np.where(hit, W / det, 0).astype(dtype)
        side = np.where(hit, np.where(det > 0, 1, -1), 0).astype(np.int8)
    return (t, u, v, side, (U, V, W)) if parts else (t, u, v, side)


def corners(vertices, faces, dtype=np.float32):
    v = np.asarray(vertices)[:, :3].astype(dtype)
    f = np.asarray(faces).reshape(-1, 3)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def limits(t_min, t_max):
    """the C ABI's limits: t_max None, <= 0 or +Inf is unlimited"""
    return float(t_min), (np.inf if t_max is None or t_max <= 0 else float(t_max))


def brute_force(origins, dirs, vertices, faces, t_min=0.0, t_max=None, dtype=np.float32, chunk=256):
    """-> t (n,), tri (n,) int32, bary (n, 2), side (n,) int8: the answer of sobfu_hip_mesh_raycast.  np.argmin returns the first, i.e.
    lowest, index of the minimum: the tie rule.  A miss is (+Inf, -1, (0, 0), 0)."""
    n, T = len(origins), len(np.asarray(faces).reshape(-1, 3))
    t_min, t_max = limits(t_min, t_max)
    t = np.full(n, np.inf, dtype)
    tri = np.full(n, -1, np.int32)
    bary = np.zeros((n, 2), dtype)
    side = np.zeros(n, np.int8)
    if n and T:
        a, b, c = corners(vertices, faces, dtype)
        ray = ray_setup(origins, dirs, dtype)
        for i in range(0, n, chunk):
            part = {k: x[i:i + chunk] for k, x in ray.items()}
            tt, u, v, s = ray_triangle(part, a, b, c, t_min, t_max, dtype)
            k = np.argmin(tt, axis=1)
            r = np.arange(len(k))
            hit = np.isfinite(tt[r, k])
            t[i:i + chunk] = tt[r, k]
            tri[i:i + chunk] = np.where(hit, k, -1)
            bary[i:i + chunk, 0], bary[i:i + chunk, 1] = u[r, k], v[r, k]
            side[i:i + chunk] = s[r, k]
    return t, tri, bary, side


# ---- the camera entry (sobfu_hip_mesh_render) -----------------------------------------------------------------------------------------
F = np.float32


def _dot(m, x, y, z):  # (m0 x + m1 y) + m2 z
    return (F(m[0]) * x + F(m[1]) * y) + F(m[2]) * z


def camera_rays(intr, rows, cols, R=np.eye(3), t=(0, 0, 0)):
    """pixel (u, v) -> ((u - cx) / fx, (v - cy) / fy, 1) in the camera of (R, t), mesh frame -> camera frame: origins o = -R^T t (in
    float64, rounded once) and directions d = R^T ray in the mesh frame, (rows * cols, 4) each, and the camera-frame (dx, dy)"""
    fx, fy, cx, cy = (F(x) for x in intr)
    R = np.asarray(R, F).reshape(3, 3)
    u, v = np.meshgrid(np.arange(cols, dtype=F), np.arange(rows, dtype=F))
    dx, dy = ((u - cx) / fx).ravel(), ((v - cy) / fy).ravel()
    one = np.ones_like(dx)
    d = np.zeros((rows * cols, 4), F)
    for i in range(3):
        d[:, i] = _dot(R[:, i], dx, dy, one)
    o = np.zeros((rows * cols, 4), F)
    R64, t64 = R.astype(np.float64), np.asarray(t, F).astype(np.float64)
    for i in range(3):
        o[:, i] = F(((0.0 - R64[0, i] * t64[0]) - R64[1, i] * t64[1]) - R64[2, i] * t64[2])
    return o, d, dx, dy


def to_byte(x):
    return np.fmin(F(255), np.fmax(F(0), np.floor(x + F(0.5)))).astype(np.uint8)


def render(vertices, faces, intr, rows, cols, R=np.eye(3), t=(0, 0, 0), z_min=0.0, z_max=None, vertex_normals=None, vertex_colours=None):
    """-> dict(depth (rows, cols) uint16, tri (rows, cols) int32, points, normals (rows, cols, 4) float32, colour (rows, cols, 4) uint8
    when vertex_colours is given): the outputs of sobfu_hip_mesh_render"""
    o, d, dx, dy = camera_rays(intr, rows, cols, R, t)
    z, tri, bary, _ = brute_force(o, d, vertices, faces, z_min, z_max)
    hit = tri >= 0
    k = np.where(hit, tri, 0)
    f = np.asarray(faces).reshape(-1, 3)
    R = np.asarray(R, F).reshape(3, 3)
    out = {}
    with np.errstate(all="ignore"):
        mm = np.rint(F(1000) * z)
        out["depth"] = np.where(hit & (mm >= 1) & (mm <= 65535), mm, 0).astype(np.uint16).reshape(rows, cols)
        out["tri"] = tri.reshape(rows, cols)
        pts = np.zeros((rows * cols, 4), F)
        pts[:, 0], pts[:, 1], pts[:, 2] = z * dx, z * dy, z
        out["points"] = np.where(hit[:, None], pts, 0).astype(F).reshape(rows, cols, 4)
        u, v = bary[:, 0], bary[:, 1]
        w = (F(1) - u) - v
        if f.size == 0:
            f = np.zeros((1, 3), np.int32)
            vertices = np.zeros((1, 4), F)
        if vertex_normals is not None:
            vn = np.asarray(vertex_normals, F)[:, :3]
            na, nb, nc = vn[f[k, 0]], vn[f[k, 1]], vn[f[k, 2]]
            n = [(w * na[:, i] + u * nb[:, i]) + v * nc[:, i] for i in range(3)]
        else:
            a, b, c = (np.asarray(vertices, F)[f[k, j], :3] for j in range(3))
            e1, e2 = b - a, c - a
            n = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
        away = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2] > 0
        n = [np.where(away, -x, x) for x in n]
        cn = [_dot(R[i], n[0], n[1], n[2]) for i in range(3)]
        ln = np.sqrt((cn[0] * cn[0] + cn[1] * cn[1]) + cn[2] * cn[2])
        ok = ln > 0
        nrm = np.stack([np.where(ok, cn[i] / np.where(ok, ln, 1), 0) for i in range(3)] + [np.ones_like(ln)], -1)
        out["normals"] = np.where(hit[:, None], nrm, 0).astype(F).reshape(rows, cols, 4)
        if vertex_colours is not None:
            vc = np.asarray(vertex_colours, np.uint8).astype(F)
            ca, cb, cc = vc[f[k, 0]], vc[f[k, 1]], vc[f[k, 2]]
            col = np.stack([to_byte((w * ca[:, i] + u * cb[:, i]) + v * cc[:, i]) for i in range(3)] + [np.full(len(k), 255, np.uint8)], -1)
            out["colour"] = np.where(hit[:, None], col, 0).astype(np.uint8).reshape(rows, cols, 4)
    return out


# ---- seeded rays shared by the CPU and GPU tests ---------------------------------------------------------------------------------------
def soup_rays(vertices, faces, lo, hi, n=4096, seed=7):
    """n rays against the soup in the box [lo, hi]: a third from outside the box toward points inside it, a third starting inside, a
    tenth that miss the box entirely, the rest aimed at vertices and at edge midpoints exactly (as far as float32 can aim) -> origins,
    dirs (n, 4) float32.  Directions are not normalised: lengths from 0.3 to 3."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    size, mid = hi - lo, (lo + hi) / 2
    o, tgt = np.zeros((n, 3)), np.zeros((n, 3))

    def outside(m):
        p = rng.normal(size=(m, 3))
        return mid + p / np.linalg.norm(p, axis=1, keepdims=True) * np.linalg.norm(size) * rng.uniform(0.6, 1.5, (m, 1))

    n1, n2, n3 = n // 3, n // 3, n // 10
    o[:n1], tgt[:n1] = outside(n1), rng.uniform(lo, hi, (n1, 3))
    o[n1:n1 + n2], tgt[n1:n1 + n2] = rng.uniform(lo, hi, (n2, 3)), rng.uniform(lo - size, hi + size, (n2, 3))
    s = slice(n1 + n2, n1 + n2 + n3)  # beyond the +x face, heading further away or sideways
    o[s] = rng.uniform(lo, hi, (n3, 3))
    o[s, 0] = hi[0] + rng.uniform(0.05, 1.0, n3) * size[0]
    tgt[s] = o[s] + np.abs(rng.normal(size=(n3, 3))) * [1, 0, 0] + rng.normal(size=(n3, 3)) * [0, 1, 1]
    rest = n - (n1 + n2 + n3)
    tri = np.asarray(vertices)[np.asarray(faces)][:, :, :3].astype(np.float64)
    pick = rng.integers(0, len(tri), rest)
    corner = rng.integers(0, 3, rest)
    at = tri[pick, corner]
    half = rest // 2
    at[half:] = (tri[pick[half:], 0].astype(np.float32) + tri[pick[half:], 1].astype(np.float32)) / np.float32(2)
    o[n1 + n2 + n3:], tgt[n1 + n2 + n3:] = outside(rest), at
    origins, dirs = np.ones((n, 4), np.float32), np.zeros((n, 4), np.float32)
    origins[:, :3] = o
    d = tgt - origins[:, :3].astype(np.float64)
    dirs[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 3.0, (n, 1))
    return origins, dirs


def watertight_rays(vertices, faces, seed=3, n_random=2000, distance=3.0):
    """rays at a closed mesh around its centroid, each from a point outside (`distance` times the target's offset from the centroid) toward
    the centroid: one through every vertex, one through every edge midpoint, n_random through random points on edges"""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices)[:, :3].astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    centre = v[np.unique(f)].mean(0)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    pick = e[rng.integers(0, len(e), n_random)]
    s = rng.uniform(0, 1, (n_random, 1))
    tgt = np.concatenate([v[np.unique(f)], (v[e[:, 0]] + v[e[:, 1]]) / 2, v[pick[:, 0]] * (1 - s) + v[pick[:, 1]] * s])
    origins, dirs = np.ones((len(tgt), 4), np.float32), np.zeros((len(tgt), 4), np.float32)
    origins[:, :3] = centre + distance * (tgt - centre)
    dirs[:, :3] = centre - origins[:, :3].astype(np.float64)
    return origins, dirs
