"""numpy restatement of the mesh sampler (sobfu_amd/csrc/sobfu_mesh_sample.hpp, mesh_sample_kernels.hip), operation by
operation, and the meshes of its tests.  Everything here is meant to equal the header and the kernels bit for bit: the generator and the
variates use integers until their last step (tests/depth_sensor_reference.py), the fold of (r1, r2) is done on integers, the areas are
float64 and the points float32 in the header's order (the library is built with -ffp-contract=off; square root is the correctly rounded
one)."""
from __future__ import annotations

import numpy as np

import depth_sensor_reference as DS

F = np.float32
COUNT_STREAM, POINT_STREAM = 0, 1
ONE = 1 << 24


def key_of(seed):
    return (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def corners(vertices, faces):
    v, f = np.asarray(vertices, F), np.asarray(faces, np.int64).reshape(-1, 3)
    return v[f[:, 0], :3], v[f[:, 1], :3], v[f[:, 2], :3]


def areas(vertices, faces):
    """(T,) float64"""
    a, b, c = (x.astype(np.float64) for x in corners(vertices, faces))
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def counts(area, density, seed):
    """(T,) int64: floor(x) + (u < frac), x = area density, u the uniform variate of word 0 of the draw (t, 0, 0, COUNT_STREAM); 2^62 for
    x >= 2^62"""
    T = len(area)
    x = area * np.float64(density)
    fl = np.floor(x)
    frac = x - fl
    c = np.stack([np.arange(T), np.zeros(T, np.int64), np.zeros(T, np.int64), np.full(T, COUNT_STREAM)], 1)
    w = DS.philox4x32_10(c, key_of(seed)) if T else np.zeros((0, 4), np.uint32)
    u = DS.uniform_variate(w[:, 0]).astype(np.float64)
    small = x < 2.0 ** 62  # beyond: 2^62, whatever the coin (the header's guard for the conversion to an integer)
    return np.where(small, np.where(small, fl, 0.0).astype(np.int64) + (u < frac), np.int64(1) << np.int64(62))


def barycentrics(tri, k, seed):
    """(r1, r2) float32 of sample k of triangle tri (arrays): the draw (t, k, 0, POINT_STREAM), folded on integers"""
    n = len(tri)
    c = np.stack([tri, k, np.zeros(n, np.int64), np.full(n, POINT_STREAM)], 1)
    w = DS.philox4x32_10(c, key_of(seed)) if n else np.zeros((0, 4), np.uint32)
    m1, m2 = (w[:, 0] >> np.uint32(8)).astype(np.int64), (w[:, 1] >> np.uint32(8)).astype(np.int64)
    fold = m1 + m2 > ONE
    m1, m2 = np.where(fold, ONE - m1, m1), np.where(fold, ONE - m2, m2)
    return m1.astype(F) * F(2.0 ** -24), m2.astype(F) * F(2.0 ** -24)


def sample(vertices, faces, density, seed=0):
    """-> dict(points (N, 4) float32, tri (N,) int32, bary (N, 2) float32, areas (T,) float64, counts (T,) int64, offsets (T + 1,) int64)"""
    a, b, c = corners(vertices, faces)
    area = areas(vertices, faces)
    cnt = counts(area, density, seed)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    N = int(off[-1])
    tri = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    k = np.arange(N, dtype=np.int64) - off[tri]
    r1, r2 = barycentrics(tri, k, seed)
    ab, ac = b - a, c - a  # float32
    p = (a[tri] + ab[tri] * r1[:, None]) + ac[tri] * r2[:, None]
    assert p.dtype == F and r1.dtype == F, "an operation left float32"
    points = np.concatenate([p, np.ones((N, 1), F)], 1)
    return dict(points=points, tri=tri.astype(np.int32), bary=np.stack([r1, r2], 1), areas=area, counts=cnt, offsets=off)


# ---- the meshes of the tests -------------------------------------------------------------------------------------------------------------
def _v4(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.ones((len(xyz), 1), F)], 1)


def box(sx=1.0, sy=0.5, sz=0.25):
    """12 triangles"""
    v = _v4([(x, y, z) for z in (0, sz) for y in (0, sy) for x in (0, sx)])
    f = np.array([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)], np.int32)
    return v, f


def lattice(n=48, size=1.0, z=0.0, x0=0.0, y0=0.0, nx=None):
    """a flat lattice of n x (nx or n) squares of edge size / n at height z: 2 n nx triangles"""
    nx = n if nx is None else nx
    h = size / n
    ys, xs = np.mgrid[0:n + 1, 0:nx + 1]
    v = _v4(np.stack([x0 + xs.ravel() * h, y0 + ys.ravel() * h, np.full(xs.size, z)], 1))
    i = (ys[:-1, :-1] * (nx + 1) + xs[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)]).astype(np.int32)
    return v, f


def rectangle(w=2.0, h=1.0, z=0.0):
    """[0, w] x [0, h] as two triangles"""
    return _v4([(0, 0, z), (w, 0, z), (w, h, z), (0, h, z)]), np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def unit_right_triangle():
    return _v4([(0, 0, 0), (1, 0, 0), (0, 1, 0)]), np.array([(0, 1, 2)], np.int32)


def one_big_among_small(small=300):
    """`small` triangles of area 5e-11 (no samples at the densities used), the unit right triangle in their middle"""
    tiny = 1e-5
    xs = np.arange(small, dtype=np.float64) * 2e-4 + 2.0
    tv = np.stack([np.stack([xs, np.zeros(small), np.zeros(small)], 1), np.stack([xs + tiny, np.zeros(small), np.zeros(small)], 1),
                   np.stack([xs, np.full(small, tiny), np.zeros(small)], 1)], 1).reshape(-1, 3)
    v = np.concatenate([_v4(tv), unit_right_triangle()[0]])
    tf = np.arange(3 * small, dtype=np.int32).reshape(-1, 3)
    big = np.array([[3 * small, 3 * small + 1, 3 * small + 2]], np.int32)
    half = small // 2
    return v, np.concatenate([tf[:half], big, tf[half:]])


def degenerate():
    """the rectangle's two triangles around a zero-area (collinear) triangle and a repeated-corner one"""
    v, f = rectangle(1.0, 1.0)
    v = np.concatenate([v, _v4([(0.5, 0.5, 0.0)])])
    return v, np.array([f[0], (0, 4, 2), (1, 1, 3), f[1]], np.int32)


SEEDS = (0, (1 << 32) + 5)  # the second one: the high key word matters


def cases():
    """(name, vertices, faces, density): the meshes of tests/test_gpu_mesh_sample.py"""
    yield ("box", *box(), 1150.3)
    yield ("lattice", *lattice(48, 1.0176), 1500.0)
    yield ("one big among small", *one_big_among_small(300), 10000.0)
    yield ("degenerate", *degenerate(), 777.7)


def same_bits(got, want, what):
    for k in ("areas", "counts", "points", "tri", "bary"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        view = {8: np.uint64, 4: np.uint32}[g.dtype.itemsize]
        assert np.array_equal(g.view(view), w.view(view)), "%s: %s differs at %d entries" % (what, k, int((g.view(view) != w.view(view)).sum()))


def point_triangle_distance(p, a, b, c):
    """float64, (n,): the distance from p_i to triangle (a_i, b_i, c_i) (Ericson 5.1.5), for points known to lie near the triangle's plane"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    nn = np.einsum("ij,ij->i", n, n)
    ap = p - a
    with np.errstate(all="ignore"):
        # barycentrics of the projection; clamp to the triangle by the nearest of the three edges when outside
        v = np.einsum("ij,ij->i", np.cross(ap, ac), n) / nn
        w = np.einsum("ij,ij->i", np.cross(ab, ap), n) / nn
    inside = (nn > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
    q = a + ab * v[:, None] + ac * w[:, None]
    d_in = np.linalg.norm(p - np.where(inside[:, None], q, a), axis=1)

    def seg(u, e):
        l2 = np.einsum("ij,ij->i", e, e)
        with np.errstate(all="ignore"):
            s = np.clip(np.where(l2 > 0, np.einsum("ij,ij->i", e, p - u) / np.where(l2 > 0, l2, 1), 0.0), 0.0, 1.0)
        return np.linalg.norm(p - (u + e * s[:, None]), axis=1)

    d_edge = np.minimum(np.minimum(seg(a, ab), seg(b, c - b)), seg(a, ac))
    return np.where(inside, d_in, d_edge)
