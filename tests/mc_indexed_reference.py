"""float32 numpy restatement of the indexed (welded) marching-cubes path of sobfu_amd/csrc/mc_kernels.hip: the edge rule, the vertex
order, positions, normals and faces.  fmaf / dot3 are those of tests/render_reference.py (an exact fmaf, one rounding).  Used by
tests/test_mc_indexed_cpu.py (against the oracle's triangle soup) and tests/test_gpu_mc_indexed.py (against the HIP path)."""
from __future__ import annotations

import os
import re

import numpy as np

import render_reference as RR

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# table edge -> (owner offset (dx, dy, dz), axis)
EDGE_OWNER = [((0, 0, 0), 0), ((1, 0, 0), 1), ((0, 1, 0), 0), ((0, 0, 0), 1), ((0, 0, 1), 0), ((1, 0, 1), 1), ((0, 1, 1), 0),
              ((0, 0, 1), 1), ((0, 0, 0), 2), ((1, 0, 0), 2), ((1, 1, 0), 2), ((0, 1, 0), 2)]
CANONICAL_EDGES = (0, 1, 4, 5, 8, 9, 10, 11)  # the soup walks these from the lower corner up: same bits as the welded vertex
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]  # (dx, dy, dz)


def case_table():
    txt = open(os.path.join(ROOT, "sobfu_amd", "csrc", "mc_table.inc")).read()
    vals = [int(v, 16) for v in re.findall(r"0x([0-9a-f]{16})ull", txt)]
    return np.array([[(v >> (4 * k)) & 15 for k in range(16)] for v in vals], np.int64)


TABLE = case_table()
NUM_VERTS = np.array([list(r).index(15) if 15 in r else 16 for r in TABLE], np.int64)


def classify(vol):
    """-> (cube (Z, Y, X) case index, nv (Z, Y, X) vertex count; 0 on the upper faces), classify_kernel's rule"""
    f, w = vol[..., 0], vol[..., 1]
    Z, Y, X = f.shape
    cube = np.zeros((Z, Y, X), np.int64)
    nv = np.zeros((Z, Y, X), np.int64)
    if min(X, Y, Z) < 2:
        return cube, nv
    seen = np.ones((Z - 1, Y - 1, X - 1), bool)
    c = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    for k, (dx, dy, dz) in enumerate(CORNERS):
        sl = (slice(dz, Z - 1 + dz), slice(dy, Y - 1 + dy), slice(dx, X - 1 + dx))
        seen &= w[sl] != 0
        c += (f[sl] < 0).astype(np.int64) << k
    c = np.where(seen, c, 0)
    cube[:-1, :-1, :-1] = c
    nv[:-1, :-1, :-1] = np.where((c == 0) | (c == 255), 0, NUM_VERTS[c])
    return cube, nv


def edge_mask(vol, nv):
    """-> (Z, Y, X) uint8: bit a = the +a edge of the voxel is cut and one of the cells sharing it is active"""
    f = vol[..., 0]
    neg = f < 0
    act = nv > 0
    mask = np.zeros(f.shape, np.uint8)
    for axis in range(3):
        ax = 2 - axis  # numpy axis of x, y, z
        cut = np.zeros(f.shape, bool)
        n = f.shape[ax]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        cut[tuple(lo)] = neg[tuple(lo)] != neg[tuple(hi)]
        # the cells sharing the edge: the owner shifted by -1 along each of the two other axes
        a = act.copy()
        others = [k for k in range(3) if k != ax]
        for sh in ([others[0]], [others[1]], others):
            s = act
            for k in sh:
                s = np.concatenate([np.zeros_like(s.take([0], axis=k)), s.take(range(s.shape[k] - 1), axis=k)], axis=k)
            a |= s
        mask |= ((cut & a).astype(np.uint8) << axis)
    return mask


def gradient(f, cs):
    """TSDF gradient per voxel (Z, Y, X, 3) x, y, z: central differences / (2 cs), one-sided / cs on a face"""
    g = np.zeros(f.shape + (3,), F)
    for axis in range(3):
        ax = 2 - axis
        n = f.shape[ax]
        if n < 2:
            continue
        idx = np.arange(n)
        lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
        den = ((hi - lo).astype(F) * cs[axis]).astype(F)
        d = (np.take(f, hi, axis=ax) - np.take(f, lo, axis=ax)).astype(F)
        shape = [1, 1, 1]
        shape[ax] = n
        g[..., axis] = d / den.reshape(shape)
    return g


def marching_cubes_indexed(vol, volume_size, R=np.eye(3), t=(0, 0, 0)):
    """-> dict: vertices (V, 4), normals (V, 4) float32, faces (F, 3) int32, edges (F, 3) table edge of each face corner, active (cells)"""
    vol = np.ascontiguousarray(vol, F)
    f = vol[..., 0]
    Z, Y, X = f.shape
    dims = (X, Y, Z)
    R = np.asarray(R, F).reshape(3, 3)
    t = np.asarray(t, F).reshape(3)
    cs = [F(F(volume_size[i]) / F(dims[i])) for i in range(3)]
    cube, nv = classify(vol)
    mask = edge_mask(vol, nv)
    flat_mask = mask.reshape(-1).astype(np.int64)
    pop = (flat_mask & 1) + ((flat_mask >> 1) & 1) + ((flat_mask >> 2) & 1)
    base = np.concatenate([[0], np.cumsum(pop)[:-1]]).astype(np.int64)
    V = int(pop.sum())
    # vertices: owners ascending, then axis
    owners = np.repeat(np.arange(flat_mask.size), 3)
    axes = np.tile(np.arange(3), flat_mask.size)
    sel = ((flat_mask[owners] >> axes) & 1) == 1
    owners, axes = owners[sel], axes[sel]
    x, y, z = owners % X, (owners // X) % Y, owners // (X * Y)
    step = np.where(axes == 0, 1, np.where(axes == 1, X, X * Y))
    ff = f.reshape(-1)
    fa, fb = ff[owners], ff[owners + step]
    a = [((c.astype(F) + F(0.5)) * cs[k]).astype(F) for k, c in enumerate((x, y, z))]
    b = [(((c + (axes == k)).astype(F) + F(0.5)) * cs[k]).astype(F) for k, c in enumerate((x, y, z))]
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = ((F(0) - fa) / (fb - fa + F(1e-15))).astype(F)
    p = [(a[k] + tt * (b[k] - a[k])).astype(F) for k in range(3)]
    w = [RR.dot3(R[i], *p) + t[i] for i in range(3)]
    vertices = np.stack([w[0], -w[1], -w[2], np.ones(V, F)], -1).astype(F)
    g = gradient(f, cs).reshape(-1, 3)
    ga, gb = g[owners], g[owners + step]
    gi = [(ga[:, k] + tt * (gb[:, k] - ga[:, k])).astype(F) for k in range(3)]
    len2 = RR.dot3(gi, *gi)
    nz = len2 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(nz, F(1) / np.sqrt(len2), F(0)).astype(F)
    nn = [np.where(nz, gi[k] * inv, F(0)).astype(F) for k in range(3)]
    r = [RR.dot3(R[i], *nn) for i in range(3)]
    normals = np.stack([r[0], -r[1], -r[2], np.ones(V, F)], -1).astype(F)
    # faces: active cells ascending, triangles in table order, corners 1 and 2 swapped
    flat_nv = nv.reshape(-1)
    cells = np.nonzero(flat_nv)[0]
    ntri = flat_nv[cells] // 3
    tc = np.repeat(cells, ntri)
    tk = np.arange(int(ntri.sum())) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    rows = TABLE[cube.reshape(-1)[tc]]
    edges = np.stack([rows[np.arange(len(tc)), 3 * tk + c] for c in range(3)], -1) if len(tc) else np.zeros((0, 3), np.int64)
    own_off = np.array([o[0] + o[1] * X + o[2] * X * Y for o, _ in EDGE_OWNER], np.int64)
    own_axis = np.array([ax for _, ax in EDGE_OWNER], np.int64)
    ow = tc[:, None] + own_off[edges]
    ax = own_axis[edges]
    below = flat_mask[ow] & ((1 << ax) - 1)
    idx = base[ow] + (below & 1) + ((below >> 1) & 1)
    faces = idx[:, [0, 2, 1]].astype(np.int32)
    return dict(vertices=vertices, normals=normals, faces=faces, edges=edges[:, [0, 2, 1]], active=int(cells.size), mask=mask)


# the volumes of tests/test_marching_cubes.py::test_hip_matches_oracle (its rotated pose and sizes)
CASES = ("sphere32", "sphere_odd", "random", "empty")
POSE_R = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], np.float32)
POSE_T = np.array([0.05, -0.1, 0.2], np.float32)
SIZE = (0.5, 0.45, 0.55)


def case_volume(oracle, case):
    if case == "sphere32":
        n, vs = 32, 0.5 / 32
        vol = oracle.new_volume((n, n, n))
        oracle.init_sphere(vol, (vs,) * 3, 5 * vs, 2 * vs, (0.25, 0.26, 0.24), 0.1)
    elif case == "sphere_odd":
        vs = 0.5 / 40
        vol = oracle.new_volume((70, 33, 19))
        oracle.init_sphere(vol, (vs,) * 3, 5 * vs, 2 * vs, (0.4, 0.2, 0.12), 0.09)
    elif case == "random":
        rng = np.random.default_rng(11)
        vol = np.stack([rng.uniform(-1, 1, (20, 24, 40)), (rng.uniform(0, 1, (20, 24, 40)) > 0.02)], -1).astype(np.float32)
    else:
        vol = oracle.new_volume((16, 16, 16))
    return vol


def read_ply(path):
    """minimal binary_little_endian PLY 1.0 reader for the two elements write_ply emits -> (header lines, vertex record array, faces)"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    nv = nf = None
    props = []
    for line in header:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[0] == "property" and nf is None:
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[0] == "property":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vt = np.dtype(props)
    verts = np.frombuffer(data, vt, nv, end)
    ft = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    fr = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(data)
    assert np.all(fr["n"] == 3)
    return header, verts, fr["i"].copy()
