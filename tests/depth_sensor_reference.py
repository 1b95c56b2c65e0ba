"""numpy restatement of the depth-sensor model (sobfu_amd/csrc/depth_sensor_kernels.hip, sobfu_random.hpp), operation by
operation in np.float32 / integer arithmetic, and an analytic scene for its tests.  Everything here is meant to equal the kernel bit for
bit: the generator and the variates use integers until their last step, and the rule's floating-point operations are written in the
kernel's order (the library is built with -ffp-contract=off; division and square root are the correctly rounded ones)."""
from __future__ import annotations

import types

import numpy as np

F = np.float32
VALID, MISS, RANGE, GRAZING, EDGE, DROPOUT = range(6)
FLAG_NAMES = ("valid", "miss", "range", "grazing", "edge", "dropout")
NORMAL_SCALE = F(float.fromhex("0x1.3988e2p-16"))
FIELDS = ("lateral", "z_min", "z_max", "cos_min", "edge_radius", "edge_jump", "edge_drop", "drop", "a0", "a1", "z0", "a2", "disparity")

# counter words, key words -> output words (Philox4x32-10)
PHILOX_KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def kinect(**changes):
    m = types.SimpleNamespace(lateral=0.8, z_min=0.4, z_max=4.0, cos_min=0.2, edge_radius=1, edge_jump=0.05, edge_drop=0.5, drop=0.0, a0=0.0012,
                              a1=0.0019, z0=0.4, a2=0.0001, disparity=348.0)
    m.__dict__.update(changes)
    return m


def ideal(**changes):
    m = types.SimpleNamespace(lateral=0.0, z_min=0.0, z_max=float("inf"), cos_min=0.0, edge_radius=0, edge_jump=0.0, edge_drop=0.0, drop=0.0, a0=0.0,
                              a1=0.0, z0=0.0, a2=0.0, disparity=0.0)
    m.__dict__.update(changes)
    return m


def parity_setting(**changes):
    """the setting the parity tests run with: kinect() with every depth of the scene in range and some random dropouts"""
    return kinect(**dict(dict(z_min=0.0, z_max=3.0, drop=0.02), **changes))



def philox4x32_10(counters, key):
    """counters (n, 4) uint32, key (2,) uint32 -> (n, 4) uint32"""
    c = np.array(counters, np.uint64).reshape(-1, 4) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 x 32 -> 64 bits: no overflow
        n0, n2 = (p1 >> s32) ^ c1 ^ np.uint64(k0), (p0 >> s32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & mask, n2, p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def draws(seed, frame, rows, cols, stream, u0=0, v0=0):
    """(rows, cols, 4) uint32: the draw of every pixel (u0 + column, v0 + row) of frame `frame`, stream `stream`"""
    v, u = np.mgrid[0:rows, 0:cols]
    c = np.stack([(u + u0).ravel(), (v + v0).ravel(), np.full(rows * cols, int(frame)), np.full(rows * cols, int(stream))], 1)
    return philox4x32_10(c, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)).reshape(rows, cols, 4)


def normal_variate(words):
    w = words.astype(np.int64)
    s = ((w & 0xFFFF) + (w >> 16)).sum(-1)
    return (s - 262140).astype(F) * NORMAL_SCALE


def uniform_variate(word):
    return (word >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def depth_sensor(points, normals, model, seed=0, frame=0, details=False):
    """points, normals (rows, cols, 4) float32 -> depth (rows, cols) uint16, flags (rows, cols) uint8; details: also a dict with the jitter
    (du, dv) and the source pixel (su, sv) of every pixel"""
    P, N = np.asarray(points, F), np.asarray(normals, F)
    rows, cols = P.shape[:2]
    m = model
    g0, g1, g2 = (normal_variate(draws(seed, frame, rows, cols, s)) for s in range(3))
    w3 = draws(seed, frame, rows, cols, 3)
    U0, U1 = uniform_variate(w3[..., 0]), uniform_variate(w3[..., 1])
    with np.errstate(all="ignore"):
        du = np.clip(np.rint(g0 * F(m.lateral)), F(-4), F(4)).astype(np.int64)
        dv = np.clip(np.rint(g1 * F(m.lateral)), F(-4), F(4)).astype(np.int64)
        v, u = np.mgrid[0:rows, 0:cols]
        su, sv = np.clip(u + du, 0, cols - 1), np.clip(v + dv, 0, rows - 1)
        # the edge test of every pixel as a source: any pixel of its window inside the frame that is a miss or jumps
        miss_map, z_map = N[..., 3] == 0, P[..., 2]
        r = int(m.edge_radius)
        edge_map = np.zeros((rows, cols), bool)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                qv, qu = v + dy, u + dx
                inside = (qv >= 0) & (qv < rows) & (qu >= 0) & (qu < cols)
                qv, qu = np.clip(qv, 0, rows - 1), np.clip(qu, 0, cols - 1)
                edge_map |= inside & (miss_map[qv, qu] | (np.abs(z_map[qv, qu] - z_map) > F(m.edge_jump)))
        x, y, z = P[sv, su, 0], P[sv, su, 1], P[sv, su, 2]
        nx, ny, nz = N[sv, su, 0], N[sv, su, 1], N[sv, su, 2]
        flags = np.full((rows, cols), 255, np.uint8)

        def end(cond, flag):
            flags[(flags == 255) & cond] = flag

        end(miss_map[sv, su], MISS)
        end(~((z > F(m.z_min)) & (z <= F(m.z_max))), RANGE)
        l = np.sqrt((x * x + y * y) + z * z)
        c = np.abs((nx * x + ny * y) + nz * z) / l
        end(c < F(m.cos_min), GRAZING)
        end((r > 0) & edge_map[sv, su] & (U0 < F(m.edge_drop)), EDGE)
        end(U1 < F(m.drop), DROPOUT)
        dz, cc = z - F(m.z0), c * c
        sigma = (F(m.a0) + F(m.a1) * (dz * dz)) + F(m.a2) * (((F(1) - cc) / cc) / np.sqrt(z))
        zn = z + g2 * sigma
        if m.disparity > 0:
            q = np.rint(F(m.disparity) / zn)
            end(~(q >= F(1)), RANGE)
            zn = F(m.disparity) / q
        mm = np.rint(F(1000) * zn)
        end(~((mm >= F(1)) & (mm <= F(65535))), RANGE)
        ok = flags == 255
        flags[ok] = VALID
        depth = np.where(ok, mm, F(0)).astype(np.uint16)
    assert all(a.dtype == F for a in (g0, U0, l, c, sigma, zn, mm)), "an operation left float32"
    if details:
        return depth, flags, dict(du=du, dv=dv, su=su, sv=sv, u=u, v=v)
    return depth, flags


def flag_counts(flags):
    return {name: int((flags == i).sum()) for i, name in enumerate(FLAG_NAMES)}


def scene(rows, cols, u0=0, v0=0, full=None):
    """The analytic scene in the renderer's format -> points, normals (rows, cols, 4) float32: a sphere, r = 0.1 m, centred at (0.02, -0.01,
    0.6), in front of a tilted plane (normal ~ (0.5, 0, -1), through (0, 0, 0.9)) that covers the left three quarters of the frame; f = 60,
    the principal point at the frame's centre.  (u0, v0, full = (rows, cols) of a larger frame): the window of that frame at this offset."""
    fr, fc = (rows, cols) if full is None else full
    f, cx, cy = 60.0, (fc - 1) / 2.0, (fr - 1) / 2.0
    v, u = np.mgrid[v0:v0 + rows, u0:u0 + cols].astype(np.float64)
    dx, dy = (u - cx) / f, (v - cy) / f
    points, normals = np.zeros((rows, cols, 4), np.float64), np.zeros((rows, cols, 4), np.float64)
    # the plane
    n = np.array([0.5, 0.0, -1.0]) / np.sqrt(1.25)
    zp = (n[2] * 0.9) / (n[0] * dx + n[2])
    on = u < 0.75 * fc
    points[on] = np.stack([zp * dx, zp * dy, zp, np.zeros_like(zp)], -1)[on]
    normals[on] = (n[0], n[1], n[2], 1.0)
    # the sphere, in front
    c, r = np.array([0.02, -0.01, 0.6]), 0.1
    a, b, k = dx * dx + dy * dy + 1.0, -2.0 * (dx * c[0] + dy * c[1] + c[2]), c @ c - r * r
    disc = b * b - 4.0 * a * k
    hit = disc > 0
    zs = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a)
    p = np.stack([zs * dx, zs * dy, zs], -1)
    points[hit] = np.concatenate([p, np.zeros(p.shape[:2] + (1,))], -1)[hit]
    normals[hit] = np.concatenate([(p - c) / r, np.ones(p.shape[:2] + (1,))], -1)[hit]
    return points.astype(F), normals.astype(F)
