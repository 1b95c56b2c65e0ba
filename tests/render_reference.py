"""float32 numpy restatement of the raycaster and the two shaders of sobfu_amd/csrc/render_kernels.hip, in the kernel's operation order.

fmaf(a, b, c) is exact (one rounding, as the device's): the product of two floats is exact in float64, the sum is rounded to odd in
float64 -- where the float64 sum is inexact and its last mantissa bit is even, it moves one ulp toward the exact sum (the sign of the
TwoSum error says which way) -- and that is rounded to float32; 53 >= 2 * 24 + 2 bits make the second rounding the only one that counts.
tests/test_render_cpu.py compares it with libm's fmaf.  Every ray is marched in lock step with the others (vectorised over rays); a
ray's arithmetic does not depend on the others.  Used by tests/test_render_cpu.py, tests/test_gpu_render.py
and tools/render_time.py (samples per ray)."""
from __future__ import annotations

import numpy as np

F = np.float32


def fma_double_rounded(a, b, c):
    """float32(float64(a) * float64(b) + float64(c)): rounds the sum twice, so it differs from fmaf at float32 ties (kept for the test
    that shows fma below is not this)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def fma(a, b, c):
    """fmaf on float32 values, one rounding (the module docstring says how)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    shape = a.shape
    with np.errstate(all="ignore"):
        p = np.atleast_1d(a).astype(np.float64) * np.atleast_1d(b).astype(np.float64)  # exact
        c = np.atleast_1d(c).astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # TwoSum: s + e = p + c exactly (NaN where s is not finite)
        bits = s.view(np.int64)
        odd = (e != 0) & np.isfinite(e) & np.isfinite(s) & ((bits & 1) == 0)
        toward = np.where((e > 0) == (s > 0), 1, -1)  # the magnitude grows when e has the sign of s
        return np.where(odd, bits + toward, bits).view(np.float64).astype(F).reshape(shape)


def lerp1(v0, v1, t):  # sobfu_device.hpp: fma(t, v0, fma(-t, v1, v1))
    return fma(t, v0, fma(-t, v1, v1))


def dot3(a, bx, by, bz):  # fma(a0, bx, fma(a1, by, a2 * bz))
    with np.errstate(invalid="ignore"):  # 0 * Inf
        return fma(a[0], bx, fma(a[1], by, F(a[2]) * bz))


def tri_setup(p, dim):
    top = F(dim - 1)
    cf = np.fmin(np.fmax(F(0), p), top)  # fmaxf(0, NaN) = 0
    g = np.floor(cf).astype(np.int64)
    h = g + np.where((cf == 0) | (cf == top), 0, 1)
    return g, h, (cf - g.astype(F)).astype(F)


def _cell(dims, gx, gy, gz):
    X, Y, _ = dims
    ag, ah, tx = tri_setup(gx, dims[0])
    bg, bh, ty = tri_setup(gy, dims[1])
    cg, ch, tz = tri_setup(gz, dims[2])

    def idx(a, b, c):
        return a + X * (b + Y * c)

    corners = {k: idx(a, b, c) for k, (a, b, c) in {
        "ggg": (ag, bg, cg), "ggh": (ag, bg, ch), "ghg": (ag, bh, cg), "ghh": (ag, bh, ch),
        "hgg": (ah, bg, cg), "hgh": (ah, bg, ch), "hhg": (ah, bh, cg), "hhh": (ah, bh, ch)}.items()}
    return corners, tx, ty, tz


def _tri(flat, c, tx, ty, tz):
    v = {k: flat[i, 0] for k, i in c.items()}
    return lerp1(lerp1(lerp1(v["hhh"], v["hhg"], tz), lerp1(v["hgh"], v["hgg"], tz), ty),
                 lerp1(lerp1(v["ghh"], v["ghg"], tz), lerp1(v["ggh"], v["ggg"], tz), ty), tx)


def sample(flat, dims, gx, gy, gz):
    """trilinear tsdf, valid (all 8 corner weights > 0)"""
    c, tx, ty, tz = _cell(dims, gx, gy, gz)
    valid = np.ones(gx.shape, bool)
    for i in c.values():
        valid &= flat[i, 1] > 0
    return _tri(flat, c, tx, ty, tz), valid


def sample_tsdf(flat, dims, gx, gy, gz):
    c, tx, ty, tz = _cell(dims, gx, gy, gz)
    return _tri(flat, c, tx, ty, tz)


def camera_rays(R, t, vs, intr, rows, cols):
    """per-call host values (R^T, -R^T t in double, rounded to float) + per-pixel ray in grid units"""
    R = np.asarray(R, F).reshape(3, 3)
    t = np.asarray(t, F).reshape(3)
    vs = np.asarray(vs, F)
    Rt = R.T.copy()
    o = np.array([-sum(float(R[j, i]) * float(t[j]) for j in range(3)) for i in range(3)], np.float64).astype(F)
    fx, fy, cx, cy = (F(v) for v in intr)
    u, v = np.meshgrid(np.arange(cols, dtype=F), np.arange(rows, dtype=F))
    dx, dy = ((u - cx) / fx).astype(F), ((v - cy) / fy).astype(F)
    one = F(1)
    D = [(dot3(Rt[i], dx, dy, one) / vs[i]).astype(F) for i in range(3)]
    O = [F(o[i] / vs[i] - F(0.5)) for i in range(3)]
    inv_len = (one / np.sqrt(dx * dx + dy * dy + one)).astype(F)
    return R, dx, dy, D, O, inv_len


def _clip(o, D, top, tmin, tmax):
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = ((F(0) - o) / D).astype(F), ((top - o) / D).astype(F)
    zero = D == 0
    inside = (o >= 0) & (o <= top)
    tmin = np.where(zero, np.where(inside, tmin, F(np.inf)), np.fmax(tmin, np.fmin(t0, t1)))
    tmax = np.where(zero, tmax, np.fmin(tmax, np.fmax(t0, t1)))
    return tmin.astype(F), tmax.astype(F)


def raycast(vol, vs, trunc, R, t, intr, rows, cols, step_factor=0.75, return_samples=False, trace=None):
    """vol: (Z, Y, X, 2) float32 -> points, normals (rows, cols, 4) float32 [, samples per ray (rows, cols) int].  trace: a dict that
    receives what the march did per ray, (rows, cols) arrays -- `enters` (tmin <= tmax), `crossing` (a crossing was found, whether
    or not its gradient made it a hit), `regained` (a valid sample after an invalid one after a valid one), `samples` -- and the
    host's `max_steps`, `D` and `O`"""
    Z, Y, X = vol.shape[:3]
    dims = (X, Y, Z)
    flat = np.ascontiguousarray(vol, F).reshape(-1, 2)
    vs = np.asarray(vs, F)
    trunc = F(trunc)
    R, dx, dy, D, O, inv_len = camera_rays(R, t, vs, intr, rows, cols)
    fine = F(F(step_factor) * min(vs[0], min(vs[1], vs[2])))
    ext = [float(d - 1) * float(s) for d, s in zip(dims, vs)]
    max_steps = int(np.sqrt(sum(e * e for e in ext)) / float(fine) + 2.0)
    tmin, tmax = np.zeros((rows, cols), F), np.full((rows, cols), np.inf, F)
    for i in range(3):
        tmin, tmax = _clip(O[i], D[i], F(dims[i] - 1), tmin, tmax)
    n = rows * cols
    D = [d.reshape(n) for d in D]
    inv_len, tmax, dxf, dyf = inv_len.reshape(n), tmax.reshape(n), dx.reshape(n), dy.reshape(n)
    points, normals = np.zeros((n, 4), F), np.zeros((n, 4), F)
    samples = np.zeros(n, np.int64)

    act = np.nonzero(tmin.reshape(n) <= tmax)[0]
    z = tmin.reshape(n)[act]
    crossing, stage = np.zeros(n, bool), np.zeros(n, np.int8)  # stage: 1 valid seen, 2 then invalid, 3 then valid again

    def note(ids, ok):
        st = stage[ids]
        stage[ids] = np.where(ok & (st != 1), np.where(st == 0, 1, 3), np.where(~ok & (st == 1), 2, st))

    def g_at(zz, ids):
        return [fma(zz, D[i][ids], O[i]) for i in range(3)]

    f, valid = sample(flat, dims, *g_at(z, act))
    samples[act] += 1
    note(act, valid)
    for _ in range(max_steps):
        if act.size == 0:
            break
        big = np.fmax(fine, (F(0.8) * f * trunc).astype(F))
        ds = np.where(valid & (f > 0), big, fine).astype(F)
        zp, fp, vp = z, f, valid
        z = fma(ds, inv_len[act], zp)
        keep = (z <= tmax[act]) & (z > zp)
        act, z, zp, fp, vp = act[keep], z[keep], zp[keep], fp[keep], vp[keep]
        if act.size == 0:
            break
        f, valid = sample(flat, dims, *g_at(z, act))
        samples[act] += 1
        note(act, valid)
        hit = vp & (fp > 0) & valid & (f < 0)
        if hit.any():
            h = act[hit]
            crossing[h] = True
            zs = (zp[hit] + ((z[hit] - zp[hit]) * fp[hit] / (fp[hit] - f[hit])).astype(F)).astype(F)
            gx, gy, gz = g_at(zs, h)
            tops = [F(d - 1) for d in dims]
            two = F(2)
            nx = ((sample_tsdf(flat, dims, np.fmin(gx + F(1), tops[0]), gy, gz) - sample_tsdf(flat, dims, np.fmax(gx - F(1), F(0)), gy, gz))
                  / (two * vs[0])).astype(F)
            ny = ((sample_tsdf(flat, dims, gx, np.fmin(gy + F(1), tops[1]), gz) - sample_tsdf(flat, dims, gx, np.fmax(gy - F(1), F(0)), gz))
                  / (two * vs[1])).astype(F)
            nz = ((sample_tsdf(flat, dims, gx, gy, np.fmin(gz + F(1), tops[2])) - sample_tsdf(flat, dims, gx, gy, np.fmax(gz - F(1), F(0))))
                  / (two * vs[2])).astype(F)
            c = [dot3(R[i], nx, ny, nz) for i in range(3)]
            ln = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]).astype(F)
            ok = ln > 0
            hk = h[ok]
            points[hk] = np.stack([zs[ok] * dxf[hk], zs[ok] * dyf[hk], zs[ok], np.zeros(hk.size, F)], 1)
            with np.errstate(invalid="ignore", divide="ignore"):
                normals[hk] = np.stack([c[0][ok] / ln[ok], c[1][ok] / ln[ok], c[2][ok] / ln[ok], np.ones(hk.size, F)], 1)
            act, z, f, valid = act[~hit], z[~hit], f[~hit], valid[~hit]
    if trace is not None:
        trace.update(enters=(tmin <= tmax.reshape(rows, cols)), crossing=crossing.reshape(rows, cols), regained=(stage == 3).reshape(rows, cols),
                     samples=samples.reshape(rows, cols), max_steps=max_steps, D=[d.reshape(rows, cols) for d in D], O=O)
    out = points.reshape(rows, cols, 4), normals.reshape(rows, cols, 4)
    return out + (samples.reshape(rows, cols),) if return_samples else out


def _byte(x):
    return np.fmin(F(255), np.fmax(F(0), np.floor(x + F(0.5)))).astype(np.uint8)


def render_image(points, normals, light=(0.0, 0.0, 0.0)):
    """BGRA uint8: grey = 0.2 + 0.8 max(0, n . normalize(light - p)) on hits, 0 on misses"""
    L = [F(v) for v in light]
    p, n = points.astype(F), normals.astype(F)
    lx, ly, lz = L[0] - p[..., 0], L[1] - p[..., 1], L[2] - p[..., 2]
    ll = np.sqrt(lx * lx + ly * ly + lz * lz).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        ndl = n[..., 0] * (lx / ll) + n[..., 1] * (ly / ll) + n[..., 2] * (lz / ll)
    g = _byte(F(255) * (F(0.2) + F(0.8) * np.fmax(F(0), ndl.astype(F))))
    hit = n[..., 3] != 0
    out = np.zeros(n.shape[:2] + (4,), np.uint8)
    out[hit, 0] = out[hit, 1] = out[hit, 2] = g[hit]
    out[hit, 3] = 255
    return out


def render_normals(normals):
    """BGRA uint8: (r, g, b) = (n * 0.5 + 0.5) * 255 on hits, 0 on misses"""
    n = normals.astype(F)
    hit = n[..., 3] != 0
    out = np.zeros(n.shape[:2] + (4,), np.uint8)
    for ch, axis in ((0, 2), (1, 1), (2, 0)):
        out[hit, ch] = _byte(((n[..., axis] * F(0.5) + F(0.5)) * F(255)))[hit]
    out[hit, 3] = 255
    return out
