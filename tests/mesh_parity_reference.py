"""numpy restatement of the row-crossing rule of sobfu_amd/csrc/sobfu_mesh_parity.hpp (signed_crossings, operation by operation: the
translation in float32, the edge functions, det and X in float64) and of what sobfu_amd/csrc/mesh_voxel_kernels.hip computes with it by brute force: the inside
and open flags of a point list, and the signed TSDF volume of a closed mesh (voxel centres, sign bits, the exact minimum distance of
tests/mesh_distance_reference.py, pack_tsdf)."""
import numpy as np

import mesh_distance_reference as MD

icosphere = MD.icosphere
indexed_soup = MD.indexed_soup
MESH_MARGIN = 1e-4  # kMeshMargin of the kernels


def _sign(e, Py, Pz, Qy, Qz):
    """parity_sign: the sign of the edge function e of the ordered edge (P, Q); ties as if the row were moved by (+e, +e^2)"""
    tie = np.where(Pz != Qz, np.where(Pz > Qz, 1, -1), np.where(Qy != Py, np.where(Qy > Py, 1, -1), 0))
    return np.where(e > 0, 1, np.where(e < 0, -1, tie)).astype(np.int8)


def corners(vertices, faces):
    v = np.asarray(vertices)[:, :3].astype(np.float32)
    f = np.asarray(faces).reshape(-1, 3)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def signed_crossings(rows, vertices, faces):
    """rows (n, 2) float32 (py, pz) -> s (n, T) int8 (the common sign of the edge functions where the row crosses, else 0), X (n, T)
    float64 (0 where there is no crossing): signed_row_crossing's operations in its order, the one statement of the rule in numpy"""
    a, b, c = corners(vertices, faces)
    r = np.asarray(rows, np.float32).reshape(-1, 2)
    py, pz = r[:, 0:1], r[:, 1:2]
    F, D = np.float32, np.float64
    Ay, Az, By, Bz, Cy, Cz = (((x[None, :, k] - p).astype(F)) for x in (a, b, c) for k, p in ((1, py), (2, pz)))
    with np.errstate(all="ignore"):
        U = By.astype(D) * Cz.astype(D) - Bz.astype(D) * Cy.astype(D)
        V = Cy.astype(D) * Az.astype(D) - Cz.astype(D) * Ay.astype(D)
        W = Ay.astype(D) * Bz.astype(D) - Az.astype(D) * By.astype(D)
        su, sv, sw = _sign(U, By, Bz, Cy, Cz), _sign(V, Cy, Cz, Ay, Az), _sign(W, Ay, Az, By, Bz)
        det = (U + V) + W
        hit = (su != 0) & (su == sv) & (su == sw) & (det != 0)
        X = np.zeros_like(det)
        num = (U * a[None, :, 0].astype(D) + V * b[None, :, 0].astype(D)) + W * c[None, :, 0].astype(D)
        np.divide(num, det, out=X, where=hit)
    return np.where(hit, su, 0).astype(np.int8), X


def crossings(rows, vertices, faces):
    """rows (n, 2) float32 (py, pz) -> hit (n, T) bool, X (n, T) float64 (0 where there is no crossing): a crossing is sign != 0"""
    s, X = signed_crossings(rows, vertices, faces)
    return s != 0, X


def inside(points, vertices, faces, chunk=512):
    """points (n, >= 3) float32 -> inside (n,) uint8, open (n,) uint8: the answer of sobfu_hip_mesh_inside"""
    p = np.asarray(points, np.float32)
    ins, opn = np.zeros(len(p), np.uint8), np.zeros(len(p), np.uint8)
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return ins, opn
    for i in range(0, len(p), chunk):
        hit, X = crossings(p[i:i + chunk, 1:3], vertices, faces)
        beyond = hit & (X > p[i:i + chunk, 0:1].astype(np.float64))
        ins[i:i + chunk] = beyond.sum(1) & 1
        opn[i:i + chunk] = hit.sum(1) & 1
    return ins, opn


def centres(n, vs):
    """voxel centres along one axis: i vs + vs / 2 in float32"""
    vs = np.float32(vs)
    return (np.arange(n, dtype=np.float32) * vs + vs / np.float32(2)).astype(np.float32)


def voxel_centres(dims, vs):
    """(Z, Y, X, 4) float32 voxel centres (x, y, z, 1) of a volume of dims = (X, Y, Z)"""
    X, Y, Z = dims
    out = np.ones((Z, Y, X, 4), np.float32)
    out[..., 0] = centres(X, vs[0])[None, None, :]
    out[..., 1] = centres(Y, vs[1])[None, :, None]
    out[..., 2] = centres(Z, vs[2])[:, None, None]
    return out


def sign_bits(vertices, faces, dims, vs):
    """-> inside (Z, Y, X) bool, open_rows: per row the crossings flip the first voxel whose centre is not below X; a voxel is inside iff
    the flips at higher voxels (and beyond the last) are odd in number"""
    X, Y, Z = dims
    cx = centres(X, vs[0]).astype(np.float64)
    yz = np.stack(np.broadcast_arrays(centres(Y, vs[1])[None, :], centres(Z, vs[2])[:, None]), -1).reshape(-1, 2)
    ins = np.zeros((Z * Y, X), bool)
    open_rows = 0
    if len(np.asarray(faces).reshape(-1, 3)) == 0:
        return ins.reshape(Z, Y, X), 0
    for i in range(0, len(yz), 256):
        hit, Xc = crossings(yz[i:i + 256], vertices, faces)
        for r in range(len(hit)):
            first = np.searchsorted(cx, Xc[r][hit[r]], side="left")  # the first centre >= X
            flips = np.bincount(first, minlength=X + 1) & 1
            ins[i + r] = (np.cumsum(flips[::-1])[::-1][1:] & 1).astype(bool)  # flips at positions > voxel
            open_rows += int(hit[r].sum() & 1)
    return ins.reshape(Z, Y, X), open_rows


def pack_tsdf(sdf, trunc, weight):
    sdf, trunc = np.asarray(sdf, np.float32), np.float32(trunc)
    with np.errstate(all="ignore"):
        t = np.where(sdf >= trunc, np.float32(1), np.where(sdf <= -trunc, np.float32(-1), (sdf / trunc).astype(np.float32)))
    return np.stack([t.astype(np.float32), np.asarray(weight, np.float32)], -1)


def voxelise(vertices, faces, dims, vs, trunc, eta, chunk=2048):
    """-> volume (Z, Y, X, 2) float32, open_rows, inside (Z, Y, X) bool: the answer of sobfu_hip_mesh_voxelise by brute force"""
    X, Y, Z = dims
    ins, open_rows = sign_bits(vertices, faces, dims, vs)
    p = voxel_centres(dims, vs).reshape(-1, 4)[:, :3]
    d2 = np.full(len(p), np.inf, np.float32)
    f = np.asarray(faces).reshape(-1, 3)
    if len(f):
        a, b, c = corners(vertices, faces)
        for i in range(0, len(p), chunk):
            d2[i:i + chunk] = MD.closest_on_triangle(p[i:i + chunk, None, :], a[None], b[None], c[None])[1].min(1)
    d = np.sqrt(d2).astype(np.float32)
    s = np.where(ins.reshape(-1), -d, d).astype(np.float32)
    w = (s > -np.float32(eta)).astype(np.float32)
    return pack_tsdf(s, trunc, w).reshape(Z, Y, X, 2), open_rows, ins


def cube(lo, hi, drop=None):
    """the axis-aligned box [lo, hi] as 12 triangles, counter-clockwise from outside -> vertices (8, 4) float32, faces (12, 3) int32.
    Faces come in the order -x, +x, -y, +y, -z, +z, two triangles each; drop: the indices of triangles to leave out (an open mesh)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    v = np.ones((8, 4), np.float32)
    for i in range(8):
        v[i, :3] = [hi[k] if (i >> k) & 1 else lo[k] for k in range(3)]
    f = np.array([(0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6)], np.int32)
    if drop is not None:
        f = np.delete(f, list(drop), 0)
    return v, np.ascontiguousarray(f)


def box_sdf(p, lo, hi):
    """float64 signed distance of points (..., 3) to the box"""
    p = np.asarray(p, np.float64)
    c, b = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2, (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / 2
    q = np.abs(p - c) - b
    return np.minimum(q.max(-1), 0) + np.linalg.norm(np.maximum(q, 0), axis=-1)
