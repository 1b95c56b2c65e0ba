"""Camera trajectories on the host: the TUM-format files apps/sobfu_headless --poses writes and --render-trajectory reads, and the two
standard errors of an estimated trajectory against the true one (Sturm et al., "A benchmark for the evaluation of RGB-D SLAM systems",
IROS 2012), in float64.  The C++ twin is include/sobfu_amd/trajectory.hpp.

A trajectory is an (n, 7) array of rows (tx, ty, tz, qx, qy, qz, qw) -- a file's line without its frame number -- or an (n, 4, 4) array
of rigid transforms; every function takes either.  A pose is camera -> frame 0's camera, as SobFusion.pose."""
from __future__ import annotations

import numpy as np


def to_matrices(poses):
    """(n, 7) rows (t, q) or (n, 4, 4) -> (n, 4, 4) float64; a quaternion is normalised first"""
    p = np.asarray(poses, np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        return p
    if p.ndim != 2 or p.shape[1] != 7:
        raise ValueError(f"expected (n, 7) or (n, 4, 4) poses, got {p.shape}")
    q = p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    x, y, z, w = q.T
    m = np.zeros((len(p), 4, 4))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    m[:, :3, 3], m[:, 3, 3] = p[:, :3], 1.0
    return m


def from_matrices(poses):
    """(n, 4, 4) -> (n, 7) rows (t, q), q = (x, y, z, w) by Shepperd's branch on the largest diagonal term (as the app writes them)"""
    m = np.asarray(poses, np.float64)
    out = np.zeros((len(m), 7))
    for i, M in enumerate(m):
        R = M[:3, :3]
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        if tr > 0:
            s = np.sqrt(tr + 1.0) * 2
            q = ((R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s)
        elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
            s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
            q = (0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s)
        elif R[1, 1] > R[2, 2]:
            s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
            q = ((R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s)
        else:
            s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
            q = ((R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s)
        out[i, :3], out[i, 3:] = M[:3, 3], q
    return out


def _rows(poses):
    p = np.asarray(poses)
    return from_matrices(p) if p.ndim == 3 else np.asarray(p, np.float64).reshape(-1, 7)


def write_tum(path, poses, frames=None):
    """one line per pose, "frame tx ty tz qx qy qz qw", the numbers at %.9g (which keeps every float32); frames: 0, 1, ... by default"""
    rows = _rows(poses)
    frames = range(len(rows)) if frames is None else frames
    with open(path, "w") as f:
        for n, r in zip(frames, rows):
            f.write("%d %s\n" % (int(n), " ".join("%.9g" % float(x) for x in r)))


def read_tum(path):
    """-> frames (n,) int64, poses (n, 7) float64 rows (tx, ty, tz, qx, qy, qz, qw).  Empty lines and lines that start with # are
    skipped; any other line that is not eight numbers raises ValueError."""
    frames, rows = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            try:
                if len(w) != 8:
                    raise ValueError
                frames.append(int(float(w[0])))
                rows.append([float(x) for x in w[1:]])
            except ValueError:
                raise ValueError(f"{path}:{ln}: expected 'frame tx ty tz qx qy qz qw'") from None
    return np.array(frames, np.int64), np.array(rows, np.float64).reshape(-1, 7)


def align(est, gt):
    """The rigid transform (R, t), no scale, that takes the positions of `est` closest to those of `gt` in the least-squares sense: Horn's
    closed form (JOSA A 4(4), 1987) -- the rotation is the eigenvector of the largest eigenvalue of the 4 x 4 matrix N of the
    cross-covariance, as a unit quaternion.  -> R (3, 3), t (3,)"""
    a, b = to_matrices(est)[:, :3, 3], to_matrices(gt)[:, :3, 3]
    if a.shape != b.shape or len(a) == 0:
        raise ValueError("the trajectories must have the same, non-zero number of poses")
    ca, cb = a.mean(0), b.mean(0)
    S = (a - ca).T @ (b - cb)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = to_matrices(np.array([[0, 0, 0, x, y, z, w]]))[0, :3, :3]
    return R, cb - R @ ca


def ate(est, gt):
    """absolute trajectory error: the root mean square of the distances between the positions of `gt` and those of `est` after align"""
    R, t = align(est, gt)
    d = to_matrices(est)[:, :3, 3] @ R.T + t - to_matrices(gt)[:, :3, 3]
    return float(np.sqrt((d * d).sum(1).mean()))


def _relative(m, delta):
    """pose_i^-1 pose_(i + delta) of every i: rotations (k, 3, 3), translations (k, 3); sums of products in a fixed order"""
    Ra, Rb, ta, tb = m[:-delta, :3, :3], m[delta:, :3, :3], m[:-delta, :3, 3], m[delta:, :3, 3]
    d = tb - ta
    R = np.zeros((len(Ra), 3, 3))
    t = np.zeros((len(Ra), 3))
    for i in range(3):
        t[:, i] = (Ra[:, 0, i] * d[:, 0] + Ra[:, 1, i] * d[:, 1]) + Ra[:, 2, i] * d[:, 2]
        for j in range(3):
            R[:, i, j] = (Ra[:, 0, i] * Rb[:, 0, j] + Ra[:, 1, i] * Rb[:, 1, j]) + Ra[:, 2, i] * Rb[:, 2, j]
    return R, t


def rpe(est, gt, delta=1):
    """relative pose error over steps of `delta` frames: with A_i = est_i^-1 est_(i + delta) and B_i likewise of gt, E_i = B_i^-1 A_i ->
    (the root mean square of |trans(E_i)|, metres; the root mean square of the rotation angle of E_i, radians).  The angle is atan2 of
    the length of the skew part of rot(E_i) and (trace - 1) / 2, and every sum of products runs in a fixed order: a trajectory against
    itself gives exactly (0, 0)."""
    a, b = to_matrices(est), to_matrices(gt)
    delta = int(delta)
    if a.shape != b.shape or delta < 1 or len(a) <= delta:
        raise ValueError("the trajectories must have the same number of poses, more than delta >= 1")
    Ra, ta = _relative(a, delta)
    Rb, tb = _relative(b, delta)
    d = ta - tb
    trans2 = np.zeros(len(d))
    for i in range(3):  # |R_B^T d|^2
        c = (Rb[:, 0, i] * d[:, 0] + Rb[:, 1, i] * d[:, 1]) + Rb[:, 2, i] * d[:, 2]
        trans2 += c * c

    def e(i, j):  # rot(E)_ij = sum_k R_B[k, i] R_A[k, j]
        return (Rb[:, 0, i] * Ra[:, 0, j] + Rb[:, 1, i] * Ra[:, 1, j]) + Rb[:, 2, i] * Ra[:, 2, j]

    sx, sy, sz = e(2, 1) - e(1, 2), e(0, 2) - e(2, 0), e(1, 0) - e(0, 1)
    angle = np.arctan2(0.5 * np.sqrt((sx * sx + sy * sy) + sz * sz), 0.5 * (((e(0, 0) + e(1, 1)) + e(2, 2)) - 1.0))
    return float(np.sqrt(trans2.mean())), float(np.sqrt((angle * angle).mean()))
