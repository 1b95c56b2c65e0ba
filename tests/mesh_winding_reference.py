"""numpy restatement of the generalised winding number of sobfu_amd/csrc/sobfu_mesh_winding.hpp and sobfu_mesh_boundary.hpp (DESIGN.md
4.14): the signed row crossings (tests/mesh_parity_reference.py states them), the boundary chain of an indexed
mesh, the solid angle of the strip from a boundary edge to infinity along -x, van Oosterom and Strackee's solid angle of a triangle, the
seam predicate, and the two ways to the winding number: the definition (every triangle's solid angle) and the boundary formula
(crossings beyond the point + strips, the definition on seams).  Everything is float64 but the translation in y and z, which is the
crossing rule's float32 one."""
import numpy as np

import mesh_parity_reference as MP

F, D = np.float32, np.float64
FOUR_PI = 4.0 * np.pi


signed_crossings = MP.signed_crossings  # the crossing rule is stated once, there


def boundary_chain(faces, n_vertices):
    """faces (T, 3) -> (B, 3) int32 rows (u, v, k), u < v, k = (#triangles that run u -> v) - (#that run v -> u) != 0, sorted by (u, v)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_vertices):
        raise ValueError("a face index is out of range")
    p, q = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]), np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keep = p != q  # an edge from a vertex to itself has no direction
    p, q = p[keep], q[keep]
    lo, hi, s = np.minimum(p, q), np.maximum(p, q), np.where(p < q, 1, -1)
    key, inv = np.unique(lo * n_vertices + hi, return_inverse=True)
    k = np.bincount(inv.ravel(), weights=s, minlength=len(key)).astype(np.int64)
    out = np.stack([key // max(n_vertices, 1), key % max(n_vertices, 1), k], 1)[k != 0]
    return out.astype(np.int32).reshape(-1, 3)


def strip_angle(points, u, v):
    """points (n, 3) float32, u, v (B, 3) float32 -> (n, B) float64: the signed solid angle at each point of the strip that runs from the
    edge u -> v to infinity along -x.  sign = -parity_sign(W) from the float32 translations in y and z; magnitude 2 atan2(|W|, den)"""
    p = np.asarray(points, F)[:, None, :3]
    u, v = np.asarray(u, F)[None, :, :3], np.asarray(v, F)[None, :, :3]
    Ay, Az, By, Bz = (u[..., 1] - p[..., 1]).astype(F), (u[..., 2] - p[..., 2]).astype(F), (v[..., 1] - p[..., 1]).astype(F), (v[..., 2] - p[..., 2]).astype(F)
    ay, az, by, bz = Ay.astype(D), Az.astype(D), By.astype(D), Bz.astype(D)
    W = ay * bz - az * by
    s = -MP._sign(W, Ay, Az, By, Bz).astype(D)
    ax, bx = u[..., 0].astype(D) - p[..., 0].astype(D), v[..., 0].astype(D) - p[..., 0].astype(D)
    la, lb = np.sqrt(ax * ax + (ay * ay + az * az)), np.sqrt(bx * bx + (by * by + bz * bz))
    den = ((la * lb + (ax * bx + (ay * by + az * bz))) - bx * la) - ax * lb
    return s * (2.0 * np.arctan2(np.abs(W), den))


def triangle_angle(a, b, c):
    """a, b, c (..., 3) float64, the corners seen from the point -> the signed solid angle (van Oosterom and Strackee)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, D), np.asarray(b, D), np.asarray(c, D))

    def dot(u, v):
        return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]

    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    bc = np.stack([b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1], b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2], b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]], -1)
    num = dot(a, bc)
    den = ((la * lb * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
    return 2.0 * np.arctan2(num, den)


def winding_sum(points, vertices, faces, chunk=4096):
    """the definition: (n,) float64, the sum of every triangle's solid angle over 4 pi, in index order"""
    p = np.asarray(points, F)[:, :3].astype(D)
    out = np.zeros(len(p))
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return out
    a, b, c = (x.astype(D) for x in MP.corners(vertices, faces))
    for i in range(0, len(p), chunk):
        q = p[i:i + chunk, None, :]
        out[i:i + chunk] = triangle_angle(a[None] - q, b[None] - q, c[None] - q).sum(1) / FOUR_PI
    return out


def seam(points, vertices, chain):
    """(n,) bool: some boundary vertex has the point's y and z (zero float32 translations) and lies beyond it in x"""
    p = np.asarray(points, F)[:, :3]
    out = np.zeros(len(p), bool)
    if len(chain) == 0:
        return out
    bv = np.asarray(vertices, F)[np.unique(chain[:, :2]), :3]
    for v in bv:
        out |= ((v[1] - p[:, 1]).astype(F) == 0) & ((v[2] - p[:, 2]).astype(F) == 0) & (v[0] > p[:, 0])
    return out


def crossings_beyond(points, vertices, faces, chunk=1024):
    """N: (n,) int64, the signed number of crossings of the row beyond each point"""
    p = np.asarray(points, F)
    out = np.zeros(len(p), np.int64)
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return out
    for i in range(0, len(p), chunk):
        s, X = signed_crossings(p[i:i + chunk, 1:3], vertices, faces)
        out[i:i + chunk] = np.where(X > p[i:i + chunk, 0:1].astype(D), s, 0).sum(1)
    return out


def crossings_beyond_centres(vertices, faces, dims, vs):
    """N at the voxel centres of a volume, row by row as the row kernel counts: every crossing adds its sign at the first voxel whose centre
    is not below X; a voxel's N is the sum at higher voxels (and beyond the last) -> (Z, Y, X) int64, open_rows (odd totals)"""
    X, Y, Z = dims
    cx = MP.centres(X, vs[0]).astype(D)
    yz = np.stack(np.broadcast_arrays(MP.centres(Y, vs[1])[None, :], MP.centres(Z, vs[2])[:, None]), -1).reshape(-1, 2)
    N = np.zeros((Z * Y, X), np.int64)
    open_rows = 0
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return N.reshape(Z, Y, X), 0
    for i in range(0, len(yz), 256):
        s, Xc = signed_crossings(yz[i:i + 256], vertices, faces)
        for r in range(len(s)):
            hit = s[r] != 0
            first = np.searchsorted(cx, Xc[r][hit], side="left")
            add = np.bincount(first, weights=s[r][hit], minlength=X + 1).astype(np.int64)
            N[i + r] = np.cumsum(add[::-1])[::-1][1:]
            open_rows += int(hit.sum() & 1)
    return N.reshape(Z, Y, X), open_rows


def winding_boundary(points, vertices, faces, chunk=2048, return_seam=False, N=None):
    """the boundary formula: N + the strips of the chain over 4 pi, in edge order; the definition on seam points -> (n,) float64.  N: the
    crossings beyond the points where the caller has them (crossings_beyond_centres)"""
    p = np.asarray(points, F)
    v = np.asarray(vertices, F)
    chain = boundary_chain(faces, len(v))
    w = (crossings_beyond(p, v, faces) if N is None else np.asarray(N).reshape(-1)).astype(D)
    if len(chain):
        u_, v_, k = v[chain[:, 0], :3], v[chain[:, 1], :3], chain[:, 2].astype(D)
        for i in range(0, len(p), chunk):
            w[i:i + chunk] += (strip_angle(p[i:i + chunk], u_, v_) * k[None, :]).sum(1) / FOUR_PI
    sm = seam(p, v, chain)
    if sm.any():
        w[sm] = winding_sum(p[sm], v, faces)
    return (w, sm) if return_seam else w


def distance_to_edges(points, vertices, chain):
    """(n,) float64 distance of each point to the nearest boundary edge (+Inf without any)"""
    p = np.asarray(points, F)[:, :3].astype(D)
    out = np.full(len(p), np.inf)
    v = np.asarray(vertices, F)[:, :3].astype(D)
    for u_, v_ in zip(v[chain[:, 0]], v[chain[:, 1]]):
        e = v_ - u_
        t = np.clip(((p - u_) @ e) / max(float(e @ e), 1e-300), 0.0, 1.0)
        out = np.minimum(out, np.linalg.norm(p - (u_ + t[:, None] * e), axis=1))
    return out


def capped_icosphere(radius, level, centre, cut, axis=1):
    """the icosphere without the faces whose centroid lies above centre + cut * radius along `axis` -> vertices, faces (open)"""
    v, f = MP.icosphere(radius, level, centre)
    keep = v[f][:, :, axis].astype(D).mean(1) <= centre[axis] + cut * radius
    return v, np.ascontiguousarray(f[keep])
