// Device-side rules shared by the frame-side kernels (render, colour, warp_points, icp and the image half of tsdf_kernels.hip): pitched
// images, shading, the point -> grid mapping and the raycaster's TSDF sampler.  Their host-side argument checks are in sobfu_host.hpp.
// The numpy restatements under tests/ follow these functions operation by operation (-ffp-contract=off, as for sobfu_device.hpp): the
// order of the floating-point operations below is part of the contract.
#pragma once

#include "sobfu_device.hpp"

namespace sobfu_hip {

// row y of a pitched image (step in bytes)
template <class T>
SOBFU_DEV T* row_ptr(T* base, int step, int y) { return (T*) ((char*) base + (size_t) y * step); }
template <class T>
SOBFU_DEV const T* row_ptr(const T* base, int step, int y) { return (const T*) ((const char*) base + (size_t) y * step); }

SOBFU_DEV unsigned char to_byte(float x) { return (unsigned char) fminf(255.f, fmaxf(0.f, floorf(x + 0.5f))); }

// headlight-style Lambertian intensity of a hit (normal n at point p, light at l, all in the camera frame): I = 0.2 + 0.8 max(0, n . l^)
SOBFU_DEV float lambert(const float4& n, const float4& p, float light_x, float light_y, float light_z) {
    const float lx = light_x - p.x, ly = light_y - p.y, lz = light_z - p.z;
    const float ll = __builtin_sqrtf(lx * lx + ly * ly + lz * lz);
    const float ndl = n.x * (lx / ll) + n.y * (ly / ll) + n.z * (lz / ll);
    return 0.2f + 0.8f * fmaxf(0.f, ndl);
}

// A point p of a frame whose pose from volume metres is (R, t): the unflipped point w -- p, or (p.x, -p.y, -p.z) for marching-cubes
// vertices (include/sobfu_hip.h, marching cubes) -- and its grid position g_i = dot3(R^T_i, w - t) / vs_i - 0.5f.  Args: a kernel's
// argument struct with the members vsx, vsy, vsz, Rt[9], t[3] and flip (the structs keep their own layouts: a kernel's code follows it).
template <class Args>
SOBFU_DEV void grid_position(const Args& m, const float4& p, float& wx, float& wy, float& wz, float& gx, float& gy, float& gz) {
    wx = p.x, wy = m.flip ? -p.y : p.y, wz = m.flip ? -p.z : p.z;
    const float qx = wx - m.t[0], qy = wy - m.t[1], qz = wz - m.t[2];
    gx = dot3(m.Rt + 0, qx, qy, qz) / m.vsx - 0.5f;
    gy = dot3(m.Rt + 3, qx, qy, qz) / m.vsy - 0.5f;
    gz = dot3(m.Rt + 6, qx, qy, qz) / m.vsz - 0.5f;
}

// The raycaster's TSDF sampler.  Corner offsets of one trilinear sample (the index rule of tri_setup: clamped, upper index = lower index on the box faces)
struct Cell {
    const float2* base;
    size_t dx, dy, dz;
    float tx, ty, tz;
};

SOBFU_DEV Cell cell_at(const float2* __restrict__ v, const Dims& d, float gx, float gy, float gz) {
    const Tri a = tri_setup(gx, d.x), b = tri_setup(gy, d.y), c = tri_setup(gz, d.z);
    const size_t sy = (size_t) d.x, sz = (size_t) d.x * d.y;
    Cell r;
    r.base = v + (size_t) a.g + (size_t) b.g * sy + (size_t) c.g * sz;
    r.dx = (size_t) (a.h - a.g), r.dy = (size_t) (b.h - b.g) * sy, r.dz = (size_t) (c.h - c.g) * sz;
    r.tx = a.t, r.ty = b.t, r.tz = c.t;
    return r;
}

// lerp1(v0, v1, t) weights v0 by t (sobfu_device.hpp): the same nesting as interp_tsdf -- z, then y, then x
SOBFU_DEV float tri_lerp(const Cell& c, float ggg, float ggh, float ghg, float ghh, float hgg, float hgh, float hhg, float hhh) {
    return lerp1(lerp1(lerp1(hhh, hhg, c.tz), lerp1(hgh, hgg, c.tz), c.ty), lerp1(lerp1(ghh, ghg, c.tz), lerp1(ggh, ggg, c.tz), c.ty), c.tx);
}

// trilinear tsdf + validity (all 8 corner weights > 0).  Unlike interp_tsdf's nearest-floor weight, a cleared (0, 0) voxel or one
// behind the surface beyond eta among the corners makes the sample invalid: it can never be one side of a surface crossing.
SOBFU_DEV float sample_tsdf(const float2* __restrict__ v, const Dims& d, float gx, float gy, float gz, bool& valid) {
    const Cell c = cell_at(v, d, gx, gy, gz);
    const float2 ggg = c.base[0], ggh = c.base[c.dz], ghg = c.base[c.dy], ghh = c.base[c.dy + c.dz];
    const float2 hgg = c.base[c.dx], hgh = c.base[c.dx + c.dz], hhg = c.base[c.dx + c.dy], hhh = c.base[c.dx + c.dy + c.dz];
    // comparisons, not a minimum: fminf drops a NaN operand, and a NaN weight is not > 0
    valid = ggg.y > 0.f && ggh.y > 0.f && ghg.y > 0.f && ghh.y > 0.f && hgg.y > 0.f && hgh.y > 0.f && hhg.y > 0.f && hhh.y > 0.f;
    return tri_lerp(c, ggg.x, ggh.x, ghg.x, ghh.x, hgg.x, hgh.x, hhg.x, hhh.x);
}

SOBFU_DEV float sample_tsdf_only(const float2* __restrict__ v, const Dims& d, float gx, float gy, float gz) {
    const Cell c = cell_at(v, d, gx, gy, gz);
    return tri_lerp(c, c.base[0].x, c.base[c.dz].x, c.base[c.dy].x, c.base[c.dy + c.dz].x, c.base[c.dx].x, c.base[c.dx + c.dz].x,
                    c.base[c.dx + c.dy].x, c.base[c.dx + c.dy + c.dz].x);
}

}  // namespace sobfu_hip
