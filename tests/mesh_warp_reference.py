"""float32 numpy restatement of sobfu_amd/csrc/warp_points_kernels.hip in the kernels' operation order: points and normals carried through
psi (warp_points) and a TSDF sampled at points (sample_tsdf).  The point -> grid mapping is tests/colour_reference.py's (sample_colour),
the valid sampler tests/render_reference.py's; fma / dot3 / lerp1 / tri_setup are render_reference's (its fma is an exact fmaf: one
rounding, as on the device).  Used by tests/test_mesh_warp_cpu.py and tests/test_gpu_mesh_warp.py."""
from __future__ import annotations

import numpy as np

import render_reference as RR

F = np.float32


def grid_position(vs, R, t, points, mc_vertices=False):
    """-> (w, g): the unflipped point and its grid position, three float32 arrays each (colour_reference.sample_colour's mapping)"""
    vs = np.asarray(vs, F)
    Rt = np.asarray(R, F).reshape(3, 3).T.copy()
    t = np.asarray(t, F).reshape(3)
    p = np.asarray(points, F)
    sgn = F(-1) if mc_vertices else F(1)
    w = (p[..., 0], (sgn * p[..., 1]).astype(F), (sgn * p[..., 2]).astype(F))
    q = (w[0] - t[0], w[1] - t[1], w[2] - t[2])
    g = [(RR.dot3(Rt[i], *q) / vs[i]).astype(F) - F(0.5) for i in range(3)]
    return w, g


def _lerp3(a, b, t):  # lerp4: per component, a weighted by t
    return [RR.lerp1(a[c], b[c], t) for c in range(3)]


def _diff3(a, b):
    return [(a[c] - b[c]).astype(F) for c in range(3)]


def warp_points(psi, vs, R, t, points, normals=None, mc_vertices=False):
    """psi (Z, Y, X, 4) float32, points (n, 4) [, normals (n, 4)] -> points (n, 4) [, normals (n, 4)] float32"""
    Z, Y, X = psi.shape[:3]
    flat = np.ascontiguousarray(psi, F).reshape(-1, 4)
    vs = np.asarray(vs, F)
    Rm = np.asarray(R, F).reshape(3, 3)
    w, g = grid_position(vs, R, t, points, mc_vertices)
    (ag, ah, tx), (bg, bh, ty), (cg, ch, tz) = RR.tri_setup(g[0], X), RR.tri_setup(g[1], Y), RR.tri_setup(g[2], Z)

    def disp(x, y, z):  # disp_at: psi + (-id)
        v = flat[x + X * (y + Y * z)]
        return [(v[..., c] + (-q.astype(F))).astype(F) for c, q in enumerate((x, y, z))]

    hhh, hhg, hgh, hgg = disp(ah, bh, ch), disp(ah, bh, cg), disp(ah, bg, ch), disp(ah, bg, cg)
    ghh, ghg, ggh, ggg = disp(ag, bh, ch), disp(ag, bh, cg), disp(ag, bg, ch), disp(ag, bg, cg)
    zhh, zhg, zgh, zgg = _lerp3(hhh, hhg, tz), _lerp3(hgh, hgg, tz), _lerp3(ghh, ghg, tz), _lerp3(ggh, ggg, tz)
    yh, yg = _lerp3(zhh, zhg, ty), _lerp3(zgh, zgg, ty)
    u = _lerp3(yh, yg, tx)
    s = [(u[c] * vs[c]).astype(F) for c in range(3)]
    o = [(w[i] + RR.dot3(Rm[i], *s)).astype(F) for i in range(3)]
    sgn = F(-1) if mc_vertices else F(1)
    out = np.stack([o[0], (sgn * o[1]).astype(F), (sgn * o[2]).astype(F), np.ones_like(o[0])], -1).astype(F)
    if normals is None:
        return out

    d = [_diff3(yh, yg), _lerp3(_diff3(zhh, zhg), _diff3(zgh, zgg), tx),
         _lerp3(_lerp3(_diff3(hhh, hhg), _diff3(hgh, hgg), ty), _lerp3(_diff3(ghh, ghg), _diff3(ggh, ggg), ty), tx)]  # d[c][r] = du_r / dg_c
    with np.errstate(all="ignore"):
        j = [[((((F(1) + d[c][r]) if r == c else d[c][r]).astype(F) * vs[r]).astype(F) / vs[c]).astype(F) for c in range(3)] for r in range(3)]

        def m2(a, b, c, e):  # a * b - c * e
            return ((a * b).astype(F) - (c * e).astype(F)).astype(F)

        cof = [[m2(j[1][1], j[2][2], j[1][2], j[2][1]), m2(j[1][2], j[2][0], j[1][0], j[2][2]), m2(j[1][0], j[2][1], j[1][1], j[2][0])],
               [m2(j[0][2], j[2][1], j[0][1], j[2][2]), m2(j[0][0], j[2][2], j[0][2], j[2][0]), m2(j[0][1], j[2][0], j[0][0], j[2][1])],
               [m2(j[0][1], j[1][2], j[0][2], j[1][1]), m2(j[0][2], j[1][0], j[0][0], j[1][2]), m2(j[0][0], j[1][1], j[0][1], j[1][0])]]

        def row(c, v):  # (c0 v0 + c1 v1) + c2 v2
            return (((c[0] * v[0]).astype(F) + (c[1] * v[1]).astype(F)).astype(F) + (c[2] * v[2]).astype(F)).astype(F)

        det = row(j[0], cof[0])
        nin = np.asarray(normals, F)
        nx, ny, nz = nin[..., 0], (sgn * nin[..., 1]).astype(F), (sgn * nin[..., 2]).astype(F)
        Rt = Rm.T.copy()
        m = [RR.dot3(Rt[i], nx, ny, nz) for i in range(3)]
        q = [row(cof[r], m) for r in range(3)]
        q = [np.where(det < 0, -x, x).astype(F) for x in q]
        len2 = row(q, q)
        inv = (F(1) / np.sqrt(len2).astype(F)).astype(F)
        q = [(x * inv).astype(F) for x in q]
        r = [RR.dot3(Rm[i], *q) for i in range(3)]
        ok = ~((nin[..., 0] == 0) & (nin[..., 1] == 0) & (nin[..., 2] == 0)) & (len2 > 0) & (len2 < F(np.inf))
    zero = np.zeros_like(r[0])
    nout = np.stack([np.where(ok, r[0], zero), np.where(ok, (sgn * r[1]).astype(F), zero), np.where(ok, (sgn * r[2]).astype(F), zero),
                     np.ones_like(zero)], -1).astype(F)
    return out, nout


def sample_tsdf(vol, vs, R, t, points, mc_vertices=False):
    """vol (Z, Y, X, 2) float32 -> (n,) float32: render_reference's valid sampler at the points, NaN where a corner weight is <= 0"""
    Z, Y, X = vol.shape[:3]
    flat = np.ascontiguousarray(vol, F).reshape(-1, 2)
    _, g = grid_position(vs, R, t, points, mc_vertices)
    f, valid = RR.sample(flat, (X, Y, Z), *g)
    return np.where(valid, f, F(np.nan)).astype(F)
