"""float32 numpy restatement of the colour kernels of sobfu_amd/csrc/colour_kernels.hip, in the kernels' operation order: integrate_colour,
the renormalised trilinear colour sampler (apply_colour, sample_colour) and render_colour.  fmaf / dot3 / tri_setup are those of
tests/render_reference.py (an exact fmaf: one rounding, as on the device).  Used by
tests/test_colour_cpu.py and tests/test_gpu_colour.py."""
from __future__ import annotations

import numpy as np

import render_reference as RR

F = np.float32


def observed(tsdf):
    """integrate_fuse_kernel's observation predicate on (..., 2) {tsdf, weight}"""
    f, w = tsdf[..., 0], tsdf[..., 1]
    return ~((w == 0) | ((w == 1) & ((f == 0) | (f == -1))))


def integrate_colour(image, tsdf, psi, colour, vs, R, t, intr, cap):
    """-> the colour volume after fusing one BGRA frame; image (rows, cols, 4) uint8, tsdf (Z, Y, X, 2), psi (Z, Y, X, 4) or None,
    colour (Z, Y, X, 4) uint8"""
    out = colour.copy()
    rows, cols = image.shape[:2]
    zz, yy, xx = np.nonzero(observed(tsdf) & (np.abs(tsdf[..., 0]) < F(1)))
    if psi is None:
        px, py, pz = xx.astype(F), yy.astype(F), zz.astype(F)
    else:
        p = psi[zz, yy, xx]
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    vs = np.asarray(vs, F)
    R = np.asarray(R, F).reshape(3, 3)
    t = np.asarray(t, F).reshape(3)
    fx, fy, cx, cy = (F(v) for v in intr)
    m = [(q * vs[i]).astype(F) + vs[i] / F(2) for i, q in enumerate((px, py, pz))]
    cam = [RR.dot3(R[i], *m) + t[i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        coox, cooy = RR.fma(fx, cam[0] / cam[2], cx), RR.fma(fy, cam[1] / cam[2], cy)
        keep = ~((coox < 0) | (cooy < 0) | (coox >= F(cols)) | (cooy >= F(rows))) & (cam[2] > 0) & (coox == coox) & (cooy == cooy)
    zz, yy, xx, coox, cooy = zz[keep], yy[keep], xx[keep], coox[keep], cooy[keep]
    n = image[np.floor(cooy).astype(np.int64), np.floor(coox).astype(np.int64)].astype(F)
    c = colour[zz, yy, xx]
    w = c[:, 3].astype(F)
    for ch in range(3):
        out[zz, yy, xx, ch] = np.rint((c[:, ch].astype(F) * w + n[:, ch]) / (w + F(1))).astype(np.uint8)
    out[zz, yy, xx, 3] = np.minimum(c[:, 3].astype(np.int64) + 1, int(cap)).astype(np.uint8)
    return out


def sample(colour, gx, gy, gz):
    """the renormalised trilinear sampler at grid points (float32 arrays) -> (..., 4) uint8"""
    Z, Y, X = colour.shape[:3]
    flat = colour.reshape(-1, 4)
    gx, gy, gz = (np.asarray(g, F) for g in (gx, gy, gz))
    ag, ah, tx = RR.tri_setup(gx, X)
    bg, bh, ty = RR.tri_setup(gy, Y)
    cg, ch, tz = RR.tri_setup(gz, Z)
    xs, ys, zs = (ag, ah), (bg, bh), (cg, ch)
    wx, wy, wz = (F(1) - tx, tx), (F(1) - ty, ty), (F(1) - tz, tz)
    s = [np.zeros(gx.shape, F) for _ in range(4)]  # b, g, r, weight
    for i in range(2):
        for j in range(2):
            for k in range(2):
                v = flat[xs[i] + X * (ys[j] + Y * zs[k])]
                has = v[..., 3] != 0
                w = ((wx[i] * wy[j]).astype(F) * wz[k]).astype(F)
                for q in range(3):
                    s[q] = np.where(has, s[q] + w * v[..., q].astype(F), s[q]).astype(F)
                s[3] = np.where(has, s[3] + w, s[3]).astype(F)
    ok = s[3] > 0
    out = np.zeros(gx.shape + (4,), np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        for q in range(3):
            out[..., q] = np.where(ok, np.fmin(F(255), np.rint(s[q] / s[3])), 0).astype(np.uint8)
    out[..., 3] = ok.astype(np.uint8)
    return out


def apply_colour(colour, psi_inv):
    return sample(colour, psi_inv[..., 0], psi_inv[..., 1], psi_inv[..., 2])


def sample_colour(colour, vs, R, t, points, normals=None, mc_vertices=False):
    """points (..., 4) float32 of a frame whose pose from volume metres is (R, t) -> (..., 4) uint8"""
    vs = np.asarray(vs, F)
    Rt = np.asarray(R, F).reshape(3, 3).T.copy()
    t = np.asarray(t, F).reshape(3)
    p = points.astype(F)
    sgn = F(-1) if mc_vertices else F(1)
    q = (p[..., 0] - t[0], (sgn * p[..., 1]).astype(F) - t[1], (sgn * p[..., 2]).astype(F) - t[2])
    g = [(RR.dot3(Rt[i], *q) / vs[i]).astype(F) - F(0.5) for i in range(3)]
    out = sample(colour, *g)
    if normals is not None:
        out[normals[..., 3] == 0] = 0
    return out


def render_colour(points, normals, colours, light=(0.0, 0.0, 0.0)):
    """BGRA uint8: colour * (0.2 + 0.8 max(0, n . l)) on hits with colour, render_image's grey on hits without, 0 on misses"""
    L = [F(v) for v in light]
    p, n = points.astype(F), normals.astype(F)
    lx, ly, lz = L[0] - p[..., 0], L[1] - p[..., 1], L[2] - p[..., 2]
    ll = np.sqrt(lx * lx + ly * ly + lz * lz).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        ndl = n[..., 0] * (lx / ll) + n[..., 1] * (ly / ll) + n[..., 2] * (lz / ll)
    I = (F(0.2) + F(0.8) * np.fmax(F(0), ndl.astype(F))).astype(F)
    out = RR.render_image(points, normals, light)
    has = (n[..., 3] != 0) & (colours[..., 3] != 0)
    for q in range(3):
        out[has, q] = RR._byte((colours[..., q].astype(F) * I).astype(F))[has]
    return out
