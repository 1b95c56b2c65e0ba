"""The rules of sobfu_amd/csrc/mesh_align_kernels.hip and sobfu_rigid.hpp restated in numpy / Python float64, in the same operation order
(the kernels are built with -ffp-contract=off; Python floats and numpy arrays never fuse):

  pose        16 floats, row-major 4 x 4, source (the points) -> target (the mesh) frame
  transform   s = ((r0 x + r1 y) + r2 z) + t per row in float32, w = 1
  correspond  the nearest triangle, and its closest point c, of s (mesh_distance_reference.brute_force, or the GPU's TriangleGrid.query:
              that answer is pinned bit for bit elsewhere)
  inlier      source point finite in x, y, z; tri >= 0; the triangle's normal has positive length.  In float64 from the float32 corners:
              m = (b - a) x (c2 - a), len = sqrt((m.x m.x + m.y m.y) + m.z m.z), n = m / len; len == 0: outlier
  row         J = [s x n, n], r = (n.x (c.x - s.x) + n.y (c.y - s.y)) + n.z (c.z - s.z) in float64
  sums        29 values: the 21 upper-triangular J_i J_j (row-major), the 6 J_i r, the inlier count, r r -- here math.fsum-exact per
              value (the kernel adds in its own fixed order: the two differ by at most n 2^-52 sum |terms|, `bounds`)
  solve       LDL^T (D_j = A_jj - sum_k<j (L_jk L_jk) D_k, L_ij = (A_ij - sum_k<j (L_ik L_jk) D_k) / D_j, by repeated subtraction), failure
              when a pivot is <= 0 or non-finite; dof 3 solves the lower-right 3 x 3 block with w = 0
  update      Tinc = (Rodrigues(w), t_inc) -- theta = sqrt((w0 w0 + w1 w1) + w2 w2), theta == 0 gives I exactly -- and
              pose = Tinc pose in float64, rounded to float32
  stop        after the update: |w| < eps_rot and |t_inc| < eps_trans -> 0x20000 | iterations done; failure: 0x10000 | iteration and the
              pose of the iteration before; 0: every iteration ran
  trace       per iteration that ran: inliers, sqrt(sum r r / inliers), |w|, |t_inc| (float32)
"""
import math

import numpy as np

import mesh_distance_reference as MD


# ---- sobfu_rigid.hpp -------------------------------------------------------------------------------------------------------------------
def ldlt(A, b):
    """A (N, N) symmetric (read at and below the diagonal), b (N,) -> x (N,), D (N,), det, ok; Python floats, the header's order"""
    N = len(b)
    A = [[float(A[r][c]) for c in range(N)] for r in range(N)]
    L = [[0.0] * N for _ in range(N)]
    D = [0.0] * N
    det, ok = 1.0, True
    with np.errstate(all="ignore"):
        for c in range(N):
            dc = A[c][c]
            for k in range(c):
                dc -= L[c][k] * L[c][k] * D[k]
            D[c] = dc
            det *= dc
            ok = ok and dc > 0.0 and dc < math.inf
            for r in range(c + 1, N):
                a = A[r][c]
                for k in range(c):
                    a -= L[r][k] * L[c][k] * D[k]
                L[r][c] = float(np.float64(a) / np.float64(dc))  # numpy: x / 0 is Inf or NaN, as in C
        x = [0.0] * N
        for r in range(N):
            y = float(b[r])
            for k in range(r):
                y -= L[r][k] * x[k]
            x[r] = y
        for r in range(N):
            x[r] = float(np.float64(x[r]) / np.float64(D[r]))
        for r in range(N - 1, -1, -1):
            y = x[r]
            for k in range(r + 1, N):
                y -= L[k][r] * x[k]
            x[r] = y
    return np.array(x), np.array(D), det, ok


def rodrigues(w):
    """rotation vector -> (R (9,) float64 row-major, theta)"""
    w0, w1, w2 = (float(v) for v in w)
    R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    th = math.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    if th > 0.0:
        kx, ky, kz, c, s = w0 / th, w1 / th, w2 / th, math.cos(th), math.sin(th)
        c1 = 1.0 - c
        R = [c + c1 * kx * kx, c1 * kx * ky - s * kz, c1 * kx * kz + s * ky,
             c1 * ky * kx + s * kz, c + c1 * ky * ky, c1 * ky * kz - s * kx,
             c1 * kz * kx - s * ky, c1 * kz * ky + s * kx, c + c1 * kz * kz]
    return np.array(R), th


def pose_compose(R, t, pose):
    """(R (9,), t (3,)) float64 times the float32 4 x 4 `pose` -> float32 4 x 4 (row 3 kept)"""
    P = np.asarray(pose, np.float32).reshape(4, 4).astype(np.float64)
    out = np.asarray(pose, np.float32).reshape(4, 4).copy()
    for r in range(3):
        for c in range(3):
            out[r, c] = np.float32((R[3 * r] * P[0, c] + R[3 * r + 1] * P[1, c]) + R[3 * r + 2] * P[2, c])
        out[r, 3] = np.float32(((R[3 * r] * P[0, 3] + R[3 * r + 1] * P[1, 3]) + R[3 * r + 2] * P[2, 3]) + t[r])
    return out


def rigid_inverse(pose):
    P = np.asarray(pose, np.float32).reshape(4, 4)
    D = P.astype(np.float64)
    out = np.zeros((4, 4), np.float32)
    out[:3, :3] = P[:3, :3].T
    for r in range(3):
        out[r, 3] = np.float32(-((D[0, r] * D[0, 3] + D[1, r] * D[1, 3]) + D[2, r] * D[2, 3]))
    out[3, 3] = 1
    return out


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------
def transform(points, pose):
    p, m = np.asarray(points, np.float32), np.asarray(pose, np.float32).reshape(4, 4)
    out = np.ones((len(p), 4), np.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = ((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3]
    return out


def rows(points, s, tri, closest, vertices, faces):
    """-> J (n, 6), r (n,), inlier (n,) bool; float64, the kernel's operations"""
    src = np.asarray(points, np.float32)
    tri = np.asarray(tri)
    t = np.where(tri >= 0, tri, 0)
    V = np.asarray(vertices, np.float32)[:, :3].astype(np.float64)
    F = np.asarray(faces)
    if len(F) == 0:
        n = len(src)
        return np.zeros((n, 6)), np.zeros(n), np.zeros(n, bool)
    a, b, c2 = V[F[t, 0]], V[F[t, 1]], V[F[t, 2]]
    u, v = b - a, c2 - a
    m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    inlier = np.isfinite(src[:, :3]).all(1) & (tri >= 0) & (ln > 0)
    with np.errstate(all="ignore"):
        n = m / ln[:, None]
        S, Cp = np.asarray(s, np.float32)[:, :3].astype(np.float64), np.asarray(closest, np.float32)[:, :3].astype(np.float64)
        r = (n[:, 0] * (Cp[:, 0] - S[:, 0]) + n[:, 1] * (Cp[:, 1] - S[:, 1])) + n[:, 2] * (Cp[:, 2] - S[:, 2])
        J = np.stack([S[:, 1] * n[:, 2] - S[:, 2] * n[:, 1], S[:, 2] * n[:, 0] - S[:, 0] * n[:, 2], S[:, 0] * n[:, 1] - S[:, 1] * n[:, 0],
                      n[:, 0], n[:, 1], n[:, 2]], 1)
    return J, r, inlier


def terms(J, r, inlier):
    """the (inliers, 29) table of the values the kernel adds"""
    J, r = J[inlier], r[inlier]
    cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [np.ones(len(r)), r * r]
    return np.stack(cols, 1) if len(r) else np.zeros((0, 29))


def sums(J, r, inlier):
    """-> (29 sums, correctly rounded: math.fsum; bounds: n 2^-52 sum |terms| per value -- twice the textbook n u sum |terms| bound of
    one recursive or pairwise float64 sum (u = 2^-53), since the kernel's and this one's errors may add; 0 for the count, which is exact)"""
    T = terms(J, r, inlier)
    total = np.array([math.fsum(T[:, k]) for k in range(29)])
    bounds = len(T) * 2.0 ** -52 * np.abs(T).sum(0)
    bounds[27] = 0.0
    return total, bounds


def unpack(s):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    return A + np.triu(A, 1).T, np.array(s[21:27])


def update(pose, s, dof):
    """the solve and update of one iteration on the 29 sums -> (pose float32 4 x 4, ok, |w|, |t_inc|)"""
    A, b = unpack(s)
    if dof == 6:
        x, _, _, ok = ldlt(A, b)
        w, t = x[:3], x[3:]
    else:
        t, _, _, ok = ldlt(A[3:, 3:], b[3:])
        w = np.zeros(3)
    if not ok:
        return np.asarray(pose, np.float32).reshape(4, 4).copy(), False, 0.0, 0.0
    R, th = rodrigues(w)
    tn = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return pose_compose(R, t, pose), True, th, tn


def brute_correspond(vertices, faces, max_dist=None):
    def f(s):
        _, tri, closest = MD.brute_force(s, vertices, faces, max_dist=max_dist)
        return tri, closest
    return f


def align(points, vertices, faces, pose=None, iters=30, dof=6, eps_rot=0.0, eps_trans=0.0, correspond=None):
    """the whole loop -> (pose float32 4 x 4, status, trace (iterations run, 4) float32).  correspond(s) -> (tri, closest)"""
    correspond = correspond or brute_correspond(vertices, faces)
    pose = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32).reshape(4, 4).copy()
    status, trace = 0, []
    for it in range(iters):
        s = transform(points, pose)
        tri, closest = correspond(s)
        total, _ = sums(*rows(points, s, tri, closest, vertices, faces))
        pose, ok, th, tn = update(pose, total, dof)
        trace.append((total[27], math.sqrt(total[28] / total[27]) if total[27] > 0 else 0.0, th, tn))
        if not ok:
            status = 0x10000 | it
            break
        if th < float(np.float32(eps_rot)) and tn < float(np.float32(eps_trans)):
            status = 0x20000 | (it + 1)
            break
    return pose, status, np.array(trace, np.float32).reshape(-1, 4)


# ---- the test bodies shared by the CPU and GPU tests -----------------------------------------------------------------------------------
CENTRE = np.array([0.02, -0.01, -0.75])
SCALE = np.array([1.0, 0.7, 0.5])


def ellipsoid(subdivisions=3):
    """icosphere(0.1, subdivisions) scaled by (1, 0.7, 0.5) about its centre, at (0.02, -0.01, -0.75) -> vertices (V, 4) float32, faces"""
    v, f = MD.icosphere(0.1, subdivisions)
    out = np.ones_like(v)
    out[:, :3] = (v[:, :3].astype(np.float64) * SCALE + CENTRE).astype(np.float32)
    return out, f


def motion(degrees, millimetres, axis=(0.3, -0.5, 0.8), direction=(0.6, 0.5, -0.62), centre=CENTRE):
    """a rigid motion about `centre`: a rotation by `degrees` about `axis`, then a shift of `millimetres` along `direction` -> float64 4 x 4"""
    k = np.asarray(axis, np.float64)
    R = rodrigues(k / np.linalg.norm(k) * np.deg2rad(degrees))[0].reshape(3, 3)
    d = np.asarray(direction, np.float64)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre - R @ centre + d / np.linalg.norm(d) * millimetres * 1e-3
    return T


def moved(vertices, T):
    """vertices through the float64 motion T, rounded to float32 once"""
    out = np.ones((len(vertices), 4), np.float32)
    out[:, :3] = (vertices[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out
