"""numpy restatement of the point-triangle rule of sobfu_amd/csrc/sobfu_mesh_distance.hpp (closest_on_triangle, operation by operation, in
float32) and of the brute-force answer of sobfu_amd/csrc/mesh_distance_kernels.hip: per point the minimum squared distance over all
triangles, the lowest triangle index attaining it, its closest point, dist = sqrt(min).  dtype=np.float64 gives the float64 twin (the same
operations in double)."""
import numpy as np


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub(u, v):
    return [u[0] - v[0], u[1] - v[1], u[2] - v[2]]


def _along(u, e, s):
    return [u[0] + e[0] * s, u[1] + e[1] * s, u[2] + e[2] * s]


def _ratio(num, den):
    out = np.zeros_like(num)
    np.divide(num, den, out=out, where=den > 0)
    return out


def _segment(p, u, e):
    l2, t = _dot(e, e), _dot(e, _sub(p, u))
    s = np.zeros_like(t)
    np.divide(t, l2, out=s, where=l2 > 0)
    s = np.where(l2 > 0, np.minimum(np.maximum(s, 0), 1), 0).astype(t.dtype)
    return _along(u, e, s)


def closest_on_triangle(p, a, b, c, dtype=np.float32):
    """p, a, b, c: arrays broadcastable to (..., 3) -> q (..., 3), d2 (...)"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype) for x in (p, a, b, c)))
    p, a, b, c = ([x[..., k] for k in range(3)] for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, bc = _sub(b, a), _sub(c, a), _sub(c, b)
        ap, bp, cp = _sub(p, a), _sub(p, b), _sub(p, c)
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        tot = (va + vb) + vc
        e1, e2 = d4 - d3, d5 - d6
        safe = np.where(tot > 0, tot, 1).astype(dtype)
        # the regions, last to first: each np.where overrides what follows it in the header's order
        q = _along(_along(a, ab, vb / safe), ac, vc / safe)
        for cond, cand in (
            ((va <= 0) & (e1 >= 0) & (e2 >= 0), _along(b, bc, _ratio(e1, e1 + e2))),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), _along(a, ac, _ratio(d2, d2 - d6))),
            ((d6 >= 0) & (d5 <= d6), c),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), _along(a, ab, _ratio(d1, d1 - d3))),
            ((d3 >= 0) & (d4 <= d3), b),
            ((d1 <= 0) & (d2 <= 0), a),
        ):
            q = [np.where(cond, cand[k], q[k]) for k in range(3)]
        # degenerate: the nearest of the segments ab, bc, ac, a later one only when strictly nearer.  The threshold follows the format's
        # rounding noise: 256 eps/2 = 2^-16 in float32 (kMeshDegenerate), 2^-45 in the float64 twin
        E2 = np.maximum(np.maximum(_dot(ab, ab), _dot(ac, ac)), _dot(bc, bc))
        m = np.maximum(np.maximum(_dot(ap, ap), _dot(bp, bp)), _dot(cp, cp))
        deg = ~(tot > (dtype(128 * np.finfo(dtype).eps) * E2) * m)
        if deg.any():
            r = _segment(p, a, ab)
            rd = _dot(_sub(p, r), _sub(p, r))
            for u, e in ((b, bc), (a, ac)):
                s = _segment(p, u, e)
                sd = _dot(_sub(p, s), _sub(p, s))
                w = sd < rd
                r = [np.where(w, s[k], r[k]) for k in range(3)]
                rd = np.where(w, sd, rd)
            q = [np.where(deg, r[k], q[k]) for k in range(3)]
        d = _sub(p, q)
        return np.stack(q, -1).astype(dtype), _dot(d, d).astype(dtype)


def pair_distances(points, vertices, faces, dtype=np.float32, chunk=256):
    """(n, T) squared distances and (n, T, 3) closest points are too large to keep for real meshes: yields (rows, q, d2) per chunk of points"""
    v = np.asarray(vertices)[:, :3].astype(dtype)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    pts = np.asarray(points)[:, :3].astype(dtype)
    for i in range(0, len(pts), chunk):
        q, d2 = closest_on_triangle(pts[i:i + chunk, None, :], a, b, c, dtype)
        yield slice(i, i + chunk), q, d2


def brute_force(points, vertices, faces, max_dist=None, dtype=np.float32, chunk=256):
    """-> dist (n,), tri (n,) int32, closest (n, 4): the answer of sobfu_hip_mesh_distance.  np.argmin returns the first, i.e. lowest, index
    of the minimum: the tie rule."""
    n, T = len(points), len(np.asarray(faces).reshape(-1, 3))
    dist = np.full(n, np.inf, dtype)
    tri = np.full(n, -1, np.int32)
    closest = np.zeros((n, 4), dtype)
    if T and n:
        for rows, q, d2 in pair_distances(points, vertices, faces, dtype, chunk):
            k = np.argmin(d2, axis=1)
            r = np.arange(len(k))
            tri[rows] = k
            dist[rows] = np.sqrt(d2[r, k])
            closest[rows, :3] = q[r, k]
            closest[rows, 3] = 1
    if max_dist is not None and max_dist > 0 and np.isfinite(max_dist):
        far = dist > dtype(max_dist)
        dist[far], tri[far], closest[far] = np.inf, -1, 0
    return dist, tri, closest


def grid_plan(bbox, n_triangles, cell=0.0, divisor=4, max_dim=128):
    """sobfu_amd/csrc/sobfu_mesh_grid.hpp (mesh_grid_plan) -> origin (3,) float32, h float32, dims (3,) int"""
    bbox = np.asarray(bbox, np.float32)
    ext = bbox[3:].astype(np.float64) - bbox[:3].astype(np.float64)
    longest = float(ext.max())
    cells = max_dim
    if cell > 0:
        h = np.float32(cell)
        if float(h) * max_dim < longest:
            h = np.float32(longest / max_dim)
    elif longest == 0:
        h = np.float32(1)
    else:
        cells = min(max(int(np.ceil(np.sqrt(float(n_triangles)) / divisor)), 1), max_dim)
        h = np.float32(longest / cells)
    while float(h) * cells < longest:
        h = np.nextafter(h, np.float32(np.inf))
    dims = np.clip(np.ceil(ext / float(h)), 1, max_dim).astype(int)
    return bbox[:3].copy(), h, dims


# ---- seeded test meshes shared by the CPU and GPU tests -------------------------------------------------------------------------------
def degenerate_shapes(a, b, c, first):
    """overwrites six groups of four triangles from `first` with every degenerate shape: a == b, a == c, b == c, a == b == c, collinear
    with c the exact midpoint of ab (coordinates rounded to 2^-10 so that the midpoint is representable), collinear with c beyond b"""
    k = first
    b[k:k + 4] = a[k:k + 4]
    c[k + 4:k + 8] = a[k + 4:k + 8]
    c[k + 8:k + 12] = b[k + 8:k + 12]
    b[k + 12:k + 16] = a[k + 12:k + 16]
    c[k + 12:k + 16] = a[k + 12:k + 16]
    s = slice(k + 16, k + 20)
    a[s], b[s] = np.round(a[s] * 512) / 512, np.round(b[s] * 512) / 512
    c[s] = (a[s] + b[s]) / 2
    s = slice(k + 20, k + 24)
    a[s], b[s] = np.round(a[s] * 512) / 512, np.round(b[s] * 512) / 512
    c[s] = a[s] + 2 * (b[s] - a[s])
    return k + 24


def soup(seed, n_triangles, n_points, slivers=True):
    """random triangles in [-1, 1]^3 with edge scale 0.1, a tenth of them exact-midpoint slivers (c = the float32 midpoint of ab) and one
    group of every degenerate shape; points in [-1.2, 1.2]^3 -> points (n, 4), corners a, b, c (T, 3), float32"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n_triangles, 3)).astype(np.float32)
    b = (a + rng.normal(scale=0.1, size=a.shape)).astype(np.float32)
    c = (a + rng.normal(scale=0.1, size=a.shape)).astype(np.float32)
    k = degenerate_shapes(a, b, c, 0)
    if slivers:
        m = slice(k, k + n_triangles // 10)
        c[m] = a[m] + np.float32(0.5) * (b[m] - a[m])
    p = np.ones((n_points, 4), np.float32)
    p[:, :3] = rng.uniform(-1.2, 1.2, (n_points, 3))
    return p, a, b, c


def shell(seed, n_triangles, n_points, radius=0.3, edge=0.005, band=0.003):
    """right triangles of `edge` tangent to a sphere of `radius` at (0, 0, 1); points within `band` of it"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_triangles, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = np.array([0, 0, 1.0])
    t1 = np.cross(d, rng.normal(size=d.shape))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    a = centre + radius * d
    b, c = a + edge * t1, a + edge * np.cross(d, t1)
    e = rng.normal(size=(n_points, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    p = np.ones((n_points, 4), np.float32)
    p[:, :3] = centre + (radius + rng.uniform(-band, band, (n_points, 1))) * e
    return p, a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)


def as_mesh(a, b, c):
    """corner arrays -> vertices (3T, 4) float32, faces (T, 3) int32 (no sharing)"""
    T = len(a)
    v = np.ones((3 * T, 4), np.float32)
    v[:, :3] = np.concatenate([a, b, c])
    return v, np.arange(3 * T, dtype=np.int32).reshape(3, T).T.copy()


def icosphere(radius, subdivisions, centre=(0, 0, 0)):
    """-> vertices (V, 4) float32 on the sphere, faces (20 * 4^s, 3) int32, counter-clockwise from outside"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for i, j, k in f:
            a, b, c = midpoint(i, j), midpoint(j, k), midpoint(k, i)
            nf += [(i, a, c), (j, b, a), (k, c, b), (a, b, c)]
        f = nf
    out = np.ones((len(v), 4), np.float32)
    out[:, :3] = np.asarray(v) * radius + np.asarray(centre, np.float64)
    return out, np.asarray(f, np.int32)


def indexed_soup(seed=1, n_triangles=700, n_points=3000):
    """The GPU tests' soup: random triangles in a 2.6 x 2.1 x 1.6 box (edge scale 0.1), every degenerate shape among the first 24, packed as
    an indexed list in which every third triangle from the 30th on shares a corner with its predecessor (so some vertices are shared and
    some are referenced by no face).  Points: a tenth beyond the box's six faces in turn by up to half its size, 50 each exactly on
    vertices, edge midpoints and face centroids, the rest inside the box -> points (n, 4), vertices (3T, 4), faces (T, 3), box lo, hi"""
    rng = np.random.default_rng(seed + 100)
    _, a, b, c = soup(seed, n_triangles, 1, slivers=False)
    s = np.array([1.0, 0.8, 0.6], np.float32)
    a, b, c = a * s, b * s, c * s
    degenerate_shapes(a, b, c, 0)
    v, f = as_mesh(a, b, c)
    for k in range(30, n_triangles, 3):
        f[k, 0] = f[k - 1, 1]
    tri = v[f][:, :, :3]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    p = np.ones((n_points, 4), np.float32)
    p[:, :3] = rng.uniform(lo, hi, (n_points, 3))
    for i in range(n_points // 10):
        ax, side = (i % 6) // 2, i % 2
        off = rng.uniform(0, 0.5) * (hi - lo)[ax]
        p[i, ax] = hi[ax] + off if side else lo[ax] - off
    k = n_points - 150
    pick = rng.integers(0, n_triangles, 150)
    p[k:k + 50, :3] = tri[pick[:50], rng.integers(0, 3, 50)]
    p[k + 50:k + 100, :3] = (tri[pick[50:100], 0] + tri[pick[50:100], 1]) / np.float32(2)
    p[k + 100:, :3] = (tri[pick[100:], 0] + tri[pick[100:], 1] + tri[pick[100:], 2]) / np.float32(3)
    return p, v, f, lo, hi
