// Diagnostics of the deformation psi: det J, folds, displacement and the residual of psi o psi^-1 -- the rules of warp_stats_kernels.hip
// (DESIGN.md 4.16), taken by a host compiler too.  tests/warp_stats_reference.py restates them operation by operation (every TU is built
// with -ffp-contract=off; the only fused operations are the sampler's two fmaf per lerp, spelt out below): the order of the floating-point
// operations is part of the contract.  Plain floats, doubles and integers, no HIP types.  The reference has no such step.
//
//   u            the displacement psi - id of a voxel (ws_disp; sobfu_device.hpp's disp_at)
//   derivative   along an axis of extent n at index i: n == 1 -> 0; i == 0 -> u(1) - u(0); i == n - 1 -> u(n - 1) - u(n - 2), one-sided and
//                not halved; otherwise (u(i + 1) - u(i - 1)) / 2 (ws_axis names the two taps, ws_deriv takes their difference)
//   det          J_rc = (r == c ? 1.f : 0.f) + d_c u_r; c00 = j11 j22 - j12 j21, c01 = j12 j20 - j10 j22, c02 = j10 j21 - j11 j20;
//                det = (j00 c00 + j01 c01) + j02 c02 (warp_points_kernel's expression).  psi = identity: det == 1.0f at every voxel
//   length       in metres: sqrtf(((a.x vs.x)^2 + (a.y vs.y)^2) + (a.z vs.z)^2)
//   mask         a voxel is in a mask {tsdf, weight} iff weight > 0 && fabsf(tsdf) < band (a NULL mask holds every voxel)
//   residual     at voxel x with p = psi^-1[x]: a non-finite component of p is "non-finite"; else p outside [0, dim - 1] on any axis is
//                "outside"; else e = (p + interp_disp(psi, p)) - id component by component (the sampler of sobfu_device.hpp: tri_setup's
//                clamp and upper-index rule, the lerp chain z, then y, then x, each lerp fmaf(t, upper, fmaf(-t, lower, lower))) and the
//                residual is len(e); a non-finite length is "non-finite"
//   sums         fx44(v) = llrint(clamp((double) v, -1024, 1024) 2^44), accumulated as two int64 words: sum(q >> 24) (arithmetic shift) and
//                sum(q & 0xffffff); the sum is hi 2^24 + lo, exact and independent of the order
//   keys         a minimum is the least uint64 (ord(v) << 32) | linear index, ord the order-preserving map of the float's bits after
//                v + 0.f (so -0 is +0); a maximum the least (~ord(v) << 32) | index.  Ties go to the lowest index.  An empty group leaves
//                kWsEmptyKey, which decodes to NaN and index -1
//   volumes      a NaN is stored as the quiet NaN 0x7fc00000 (ws_canonical), so the bits do not depend on which operation made it
//   launch       ws_launch / ws_tile: 64 x 4 tiles of (x, y) columns, each marched over a chunk of z planes; tiles numbered so that an XCD
//                owns a band of tile rows at every z (sobfu_device.hpp's xcd_tile, on a 1-D grid: no extent is bounded by a grid limit)
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SOBFU_WS_FN __host__ __device__ __forceinline__
#else
#define SOBFU_WS_FN inline
#endif

namespace sobfu_hip {

constexpr int kWsMaxEdges = 16;
constexpr uint64_t kWsEmptyKey = ~(uint64_t) 0;
constexpr int kWsTileX = 64, kWsTileY = 4;     // lanes of a workgroup: 64 consecutive x, 4 rows
constexpr int kWsMinChunk = 4;                 // planes: a chunk re-reads one plane of z halo on each side when it starts
constexpr long long kWsWorkgroups = 1024;      // aimed at: what the chip holds at once (256 CUs x 4 workgroups of 4 waves at <= 128 VGPRs); one set
                                               // of atomics each on the result block, and a chunk long enough to carry the workgroup's reduction
constexpr long long kWsMaxVoxels = 1LL << 31;  // a linear index fits 32 bits

struct WsV3 {
    float x, y, z;
};
struct WsDims {
    int x, y, z;
};

SOBFU_WS_FN bool ws_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }
SOBFU_WS_FN WsV3 ws_disp(float px, float py, float pz, int x, int y, int z) { return WsV3{px - (float) x, py - (float) y, pz - (float) z}; }

// the two taps of the derivative along an axis of extent n at index i, and whether their difference is halved (n == 1: lo == hi, and
// ws_deriv's `flat`)
SOBFU_WS_FN void ws_axis(int n, int i, int& lo, int& hi, bool& halved) {
    lo = i > 0 ? i - 1 : 0;
    hi = i < n - 1 ? i + 1 : n - 1;
    halved = i > 0 && i < n - 1;
}
SOBFU_WS_FN WsV3 ws_deriv(const WsV3& lo, const WsV3& hi, bool halved, bool flat) {
    if (flat) return WsV3{0.f, 0.f, 0.f};
    const WsV3 d{hi.x - lo.x, hi.y - lo.y, hi.z - lo.z};
    return halved ? WsV3{d.x / 2.f, d.y / 2.f, d.z / 2.f} : d;
}
// dx, dy, dz: the derivatives of u along x, y, z
SOBFU_WS_FN float ws_det(const WsV3& dx, const WsV3& dy, const WsV3& dz) {
    const float j00 = 1.f + dx.x, j01 = 0.f + dy.x, j02 = 0.f + dz.x;
    const float j10 = 0.f + dx.y, j11 = 1.f + dy.y, j12 = 0.f + dz.y;
    const float j20 = 0.f + dx.z, j21 = 0.f + dy.z, j22 = 1.f + dz.z;
    const float c00 = j11 * j22 - j12 * j21, c01 = j12 * j20 - j10 * j22, c02 = j10 * j21 - j11 * j20;
    return (j00 * c00 + j01 * c01) + j02 * c02;
}
SOBFU_WS_FN float ws_len(const WsV3& a, const float vs[3]) {
    const float sx = a.x * vs[0], sy = a.y * vs[1], sz = a.z * vs[2];
    return __builtin_sqrtf((sx * sx + sy * sy) + sz * sz);
}
SOBFU_WS_FN bool ws_in_mask(float tsdf, float weight, float band) { return weight > 0.f && __builtin_fabsf(tsdf) < band; }

SOBFU_WS_FN uint32_t ws_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
SOBFU_WS_FN float ws_canonical(float v) {
    if (v == v) return v;
    const uint32_t q = 0x7fc00000u;
    float r;
    __builtin_memcpy(&r, &q, 4);
    return r;
}
SOBFU_WS_FN uint32_t ws_ord(float v) {
    const uint32_t b = ws_bits(v + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SOBFU_WS_FN uint64_t ws_min_key(float v, uint32_t index) { return ((uint64_t) ws_ord(v) << 32) | index; }
SOBFU_WS_FN uint64_t ws_max_key(float v, uint32_t index) { return ((uint64_t) (~ws_ord(v)) << 32) | index; }

SOBFU_WS_FN int64_t ws_fx44(float v) {
    double d = (double) v;
    d = d < -1024.0 ? -1024.0 : (d > 1024.0 ? 1024.0 : d);
    return (int64_t) __builtin_llrint(d * 0x1p44);
}
struct WsSum {
    int64_t hi, lo;
};
SOBFU_WS_FN void ws_add(WsSum& s, float v) {
    const int64_t q = ws_fx44(v);
    s.hi += q >> 24;
    s.lo += q & 0xffffff;
}

// ---- the sampler of the residual: sobfu_device.hpp's tri_setup / lerp1 / interp_disp on plain floats ---------------------------------
struct WsTri {
    int g, h;
    float t;
};
SOBFU_WS_FN WsTri ws_tri(float p, int dim) {
    const float top = (float) dim - 1;
    const float cf = __builtin_fminf(__builtin_fmaxf(0.f, p), top);
    WsTri r;
    r.g = (int) __builtin_floorf(cf);
    r.h = r.g + ((cf == 0.f || cf == top) ? 0 : 1);
    r.t = cf - (float) r.g;
    return r;
}
SOBFU_WS_FN float ws_lerp1(float v0, float v1, float t) { return __builtin_fmaf(t, v0, __builtin_fmaf(-t, v1, v1)); }
SOBFU_WS_FN WsV3 ws_lerp(const WsV3& a, const WsV3& b, float t) { return WsV3{ws_lerp1(a.x, b.x, t), ws_lerp1(a.y, b.y, t), ws_lerp1(a.z, b.z, t)}; }
// disp(x, y, z): the displacement of a voxel
template <class Disp>
SOBFU_WS_FN WsV3 ws_interp_disp(Disp disp, const WsDims& d, float px, float py, float pz) {
    const WsTri a = ws_tri(px, d.x), b = ws_tri(py, d.y), c = ws_tri(pz, d.z);
    return ws_lerp(ws_lerp(ws_lerp(disp(a.h, b.h, c.h), disp(a.h, b.h, c.g), c.t), ws_lerp(disp(a.h, b.g, c.h), disp(a.h, b.g, c.g), c.t), b.t),
                   ws_lerp(ws_lerp(disp(a.g, b.h, c.h), disp(a.g, b.h, c.g), c.t), ws_lerp(disp(a.g, b.g, c.h), disp(a.g, b.g, c.g), c.t), b.t), a.t);
}

enum { kWsResOk = 0, kWsResNonFinite = 1, kWsResOutside = 2 };
// the residual at voxel (x, y, z) with p = psi^-1 there -> its class; *len: the residual (kWsResOk, or a non-finite length), else NaN
template <class Disp>
SOBFU_WS_FN int ws_residual(Disp disp, const WsDims& d, float px, float py, float pz, int x, int y, int z, const float vs[3], float* len) {
    *len = ws_canonical(__builtin_nanf(""));
    if (!(ws_finite(px) && ws_finite(py) && ws_finite(pz))) return kWsResNonFinite;
    if (px < 0.f || px > (float) (d.x - 1) || py < 0.f || py > (float) (d.y - 1) || pz < 0.f || pz > (float) (d.z - 1)) return kWsResOutside;
    const WsV3 u = ws_interp_disp(disp, d, px, py, pz);
    const WsV3 e{(px + u.x) - (float) x, (py + u.y) - (float) y, (pz + u.z) - (float) z};
    *len = ws_canonical(ws_len(e, vs));
    return ws_finite(*len) ? kWsResOk : kWsResNonFinite;
}

// ---- launch shape --------------------------------------------------------------------------------------------------------------------
struct WsLaunch {
    unsigned gx, gy, chunks;  // tiles along x and y, chunks along z
    int zc;                   // planes per chunk
};
inline WsLaunch ws_launch(int X, int Y, int Z) {
    WsLaunch l;
    l.gx = (unsigned) (((long long) X + kWsTileX - 1) / kWsTileX);
    l.gy = (unsigned) (((long long) Y + kWsTileY - 1) / kWsTileY);
    const long long tiles = (long long) l.gx * l.gy;
    const long long want = kWsWorkgroups / tiles > 1 ? kWsWorkgroups / tiles : 1;
    const long long zc = ((long long) Z + want - 1) / want;
    l.zc = (int) (zc > kWsMinChunk ? zc : kWsMinChunk);
    l.chunks = (unsigned) (((long long) Z + l.zc - 1) / l.zc);
    return l;
}
inline unsigned long long ws_workgroups(const WsLaunch& l) { return (unsigned long long) l.gx * l.gy * l.chunks; }
// workgroup w of ws_workgroups -> its tile (bx, by) and chunk bz.  Consecutive workgroups go round-robin to the 8 XCDs: XCD k owns the
// k-th eighth of the tile rows at every chunk when their count is a multiple of 8 (xcd_tile's rule), else the launch order is kept
SOBFU_WS_FN void ws_tile(unsigned w, const WsLaunch& l, unsigned& bx, unsigned& by, unsigned& bz) {
    if ((l.gy & 7u) != 0u) {
        bx = w % l.gx;
        const unsigned r = w / l.gx;
        by = r % l.gy, bz = r / l.gy;
        return;
    }
    const unsigned k = w & 7u, j = w >> 3, band = l.gy >> 3, per = l.gx * band;
    bz = j / per;
    const unsigned rem = j - bz * per, row = rem / l.gx;
    bx = rem - row * l.gx;
    by = k * band + row;
}

}  // namespace sobfu_hip
