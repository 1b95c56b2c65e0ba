// Points through the deformation for gfx950: the canonical mesh's vertices and normals carried to the live frame by psi, and a TSDF
// sampled at points (the fit of the warped model to a frame).
//
// The reference has no such step (its live meshes are fresh marching-cubes runs on warped volumes); the rules below are this project's,
// and tests/mesh_warp_reference.py restates them in the same operation order (every TU is built with -ffp-contract=off: the fmaf below
// are the only fused operations).
//
//   inputs    n points (float4), optionally n normals (float4), psi (float4 per voxel: the absolute position, in voxel units, that the
//             canonical voxel maps to; dense, x fastest), the voxel size, a pose (R row-major, t) from volume metres to the points'
//             frame, and mc_vertices as in sobfu_hip_sample_colour: 1 = the points are marching-cubes vertices (x, -y, -z, 1) under the
//             marching-cubes pose, and the flip is undone first; 0 = plain points
//   direction v -> psi(v): psi maps a canonical position to its live position, so the canonical surface is carried forwards
//   position  1. w = unflip(v); g_i = dot3(R^T_i, w - t) / vs_i - 0.5f: sample_colour's mapping (grid_position, sobfu_frame.hpp)
//             2. u = interp_disp(psi, g) (sobfu_device.hpp): tri_setup's clamp and upper-index rule, corner displacement psi - id, the
//                lerp chain z, then y, then x
//             3. delta_i = dot3(R_i, u.x vs.x, u.y vs.y, u.z vs.z); the output is flip(w + delta), w = 1.  The vertex is not rebuilt
//                from g: with psi = identity every u is exactly 0 and the output equals the input
//   normal    4. J_g = I + du/dg, the analytic derivative of the same trilinear interpolant in the same cell, from the eight corner
//                displacements of step 2: du/dgx = (the yz-lerp of the upper x face) - (that of the lower x face), du/dgy = the x-lerp
//                of (z-lerp of the upper y edge - z-lerp of the lower y edge), du/dgz = the x-lerp of the y-lerp of (upper z corner -
//                lower z corner).  Along an axis that tri_setup collapses (h == g) the two sides are the same corners: the derivative is 0
//             5. J_rc = (J_g_rc vs_r) / vs_c (metres); m = R^T unflip(n.xyz); m' = cof(J) m (the cofactor matrix: J^-T without the
//                division), each row (c0 m0 + c1 m1) + c2 m2, negated when det J = (J00 c00 + J01 c01) + J02 c02 < 0; m' times
//                1 / sqrt((m'x^2 + m'y^2) + m'z^2); the output is flip(R m') with w = 1.  A zero input normal, or a zero or non-finite
//                squared length, gives (0, 0, 0, 1): the indexed mesh's "no normal"
//   sample    sample_tsdf: the mapping of step 1, then the raycaster's sampler (sample_tsdf, sobfu_frame.hpp): trilinear TSDF, valid only
//             when all eight corner weights are > 0.  One float per point: the TSDF (units of the truncation distance), NaN where not valid
//
// Launch shape: one lane per point, 256-thread workgroups.  Indexed-mesh vertices arrive in ascending owner-voxel order (x fastest), so
// the lanes of a wave are neighbours on the surface and share psi's cache lines: psi and the volume are taken with plain cached loads,
// points and normals as 16-byte loads and stores.  No LDS, no atomics.  Each lane reads its point and normal before it writes them:
// output = input is allowed.
#include "sobfu_frame.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"

#include <cmath>

using namespace sobfu_hip;

namespace {

struct PointMap {
    Dims d;
    float vsx, vsy, vsz;
    float R[9], Rt[9], t[3];
    int flip;  // marching-cubes vertices: (x, -y, -z)
    int n;
};

struct WarpArgs {
    const float4* psi;
    PointMap m;
    const float4* points;
    const float4* normals;
    float4* points_out;
    float4* normals_out;
};

struct SampleTsdfArgs {
    const float2* vol;
    PointMap m;
    const float4* points;
    float* out;
};

SOBFU_DEV float4 diff4(const float4& a, const float4& b) { return f4(a.x - b.x, a.y - b.y, a.z - b.z); }

template <bool NORMALS>
__global__ void __launch_bounds__(256) warp_points_kernel(WarpArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m.n) return;
    const float4 p = a.points[i];
    float4 nin = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NORMALS) nin = a.normals[i];
    float wx, wy, wz, gx, gy, gz;
    grid_position(a.m, p, wx, wy, wz, gx, gy, gz);  // step 1

    const Dims d = a.m.d;
    const Tri tx = tri_setup(gx, d.x), ty = tri_setup(gy, d.y), tz = tri_setup(gz, d.z);
    const float4 hhh = disp_at(a.psi, d, tx.h, ty.h, tz.h), hhg = disp_at(a.psi, d, tx.h, ty.h, tz.g);
    const float4 hgh = disp_at(a.psi, d, tx.h, ty.g, tz.h), hgg = disp_at(a.psi, d, tx.h, ty.g, tz.g);
    const float4 ghh = disp_at(a.psi, d, tx.g, ty.h, tz.h), ghg = disp_at(a.psi, d, tx.g, ty.h, tz.g);
    const float4 ggh = disp_at(a.psi, d, tx.g, ty.g, tz.h), ggg = disp_at(a.psi, d, tx.g, ty.g, tz.g);
    // interp_disp's chain, its intermediate values kept for the derivative
    const float4 zhh = lerp4(hhh, hhg, tz.t), zhg = lerp4(hgh, hgg, tz.t), zgh = lerp4(ghh, ghg, tz.t), zgg = lerp4(ggh, ggg, tz.t);
    const float4 yh = lerp4(zhh, zhg, ty.t), yg = lerp4(zgh, zgg, ty.t);
    const float4 u = lerp4(yh, yg, tx.t);

    const float sx = u.x * a.m.vsx, sy = u.y * a.m.vsy, sz = u.z * a.m.vsz;
    const float ox = wx + dot3(a.m.R + 0, sx, sy, sz), oy = wy + dot3(a.m.R + 3, sx, sy, sz), oz = wz + dot3(a.m.R + 6, sx, sy, sz);
    a.points_out[i] = make_float4(ox, a.m.flip ? -oy : oy, a.m.flip ? -oz : oz, 1.f);

    if (NORMALS) {
        const float4 dx = diff4(yh, yg);
        const float4 dy = lerp4(diff4(zhh, zhg), diff4(zgh, zgg), tx.t);
        const float4 dz = lerp4(lerp4(diff4(hhh, hhg), diff4(hgh, hgg), ty.t), lerp4(diff4(ghh, ghg), diff4(ggh, ggg), ty.t), tx.t);
        const float vx = a.m.vsx, vy = a.m.vsy, vz = a.m.vsz;
        // J_rc = d(metres r) / d(metres c): row r is the component of u, column c the axis of the derivative
        const float j00 = ((1.f + dx.x) * vx) / vx, j01 = (dy.x * vx) / vy, j02 = (dz.x * vx) / vz;
        const float j10 = (dx.y * vy) / vx, j11 = ((1.f + dy.y) * vy) / vy, j12 = (dz.y * vy) / vz;
        const float j20 = (dx.z * vz) / vx, j21 = (dy.z * vz) / vy, j22 = ((1.f + dz.z) * vz) / vz;
        const float c00 = j11 * j22 - j12 * j21, c01 = j12 * j20 - j10 * j22, c02 = j10 * j21 - j11 * j20;
        const float c10 = j02 * j21 - j01 * j22, c11 = j00 * j22 - j02 * j20, c12 = j01 * j20 - j00 * j21;
        const float c20 = j01 * j12 - j02 * j11, c21 = j02 * j10 - j00 * j12, c22 = j00 * j11 - j01 * j10;
        const float det = (j00 * c00 + j01 * c01) + j02 * c02;
        const float ny = a.m.flip ? -nin.y : nin.y, nz = a.m.flip ? -nin.z : nin.z;
        const float m0 = dot3(a.m.Rt + 0, nin.x, ny, nz), m1 = dot3(a.m.Rt + 3, nin.x, ny, nz), m2 = dot3(a.m.Rt + 6, nin.x, ny, nz);
        float q0 = (c00 * m0 + c01 * m1) + c02 * m2, q1 = (c10 * m0 + c11 * m1) + c12 * m2, q2 = (c20 * m0 + c21 * m1) + c22 * m2;
        const bool neg = det < 0.f;  // component by component: a select between two float3 objects would go through the stack
        q0 = neg ? -q0 : q0, q1 = neg ? -q1 : q1, q2 = neg ? -q2 : q2;
        const float len2 = (q0 * q0 + q1 * q1) + q2 * q2;
        const float inv = 1.f / __builtin_sqrtf(len2);
        q0 = q0 * inv, q1 = q1 * inv, q2 = q2 * inv;
        const float rx = dot3(a.m.R + 0, q0, q1, q2), ry = dot3(a.m.R + 3, q0, q1, q2), rz = dot3(a.m.R + 6, q0, q1, q2);
        const bool ok = !(nin.x == 0.f && nin.y == 0.f && nin.z == 0.f) && len2 > 0.f && len2 < INFINITY;
        a.normals_out[i] = make_float4(ok ? rx : 0.f, ok ? (a.m.flip ? -ry : ry) : 0.f, ok ? (a.m.flip ? -rz : rz) : 0.f, 1.f);
    }
}

__global__ void __launch_bounds__(256) sample_tsdf_points_kernel(SampleTsdfArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m.n) return;
    float wx, wy, wz, gx, gy, gz;
    grid_position(a.m, a.points[i], wx, wy, wz, gx, gy, gz);
    bool valid;
    const float f = sample_tsdf(a.vol, a.m.d, gx, gy, gz, valid);
    a.out[i] = valid ? f : __builtin_nanf("");
}

PointMap point_map(int X, int Y, int Z, const float vs[3], const float R[9], const float t[3], int mc_vertices, int n) {
    PointMap m{{X, Y, Z}, vs[0], vs[1], vs[2], {}, {}, {}, mc_vertices ? 1 : 0, n};
    fill_pose(R, t, m.R, m.Rt, m.t);
    return m;
}

}  // namespace

extern "C" {

int sobfu_hip_warp_points(const float* d_psi, int X, int Y, int Z, const float vs[3], const float R[9], const float t[3], int mc_vertices,
                          const float* d_points, const float* d_normals, int n, float* d_points_out, float* d_normals_out, void* stream) {
    SOBFU_CHECK_ARGS(d_psi && vs && R && t && d_points && d_points_out && volume_ok(X, Y, Z, INT_MAX) && n >= 0);
    SOBFU_CHECK_ARGS((d_normals != nullptr) == (d_normals_out != nullptr));
    SOBFU_CHECK_ARGS(aligned(d_psi, 0, 16) && aligned(d_points, 0, 16) && aligned(d_points_out, 0, 16));
    SOBFU_CHECK_ARGS(aligned(d_normals, 0, 16) && aligned(d_normals_out, 0, 16));
    SOBFU_CHECK_ARGS(positive_finite(vs[0]) && positive_finite(vs[1]) && positive_finite(vs[2]));
    if (n == 0) return 0;
    WarpArgs a{(const float4*) d_psi, point_map(X, Y, Z, vs, R, t, mc_vertices, n), (const float4*) d_points, (const float4*) d_normals,
               (float4*) d_points_out, (float4*) d_normals_out};
    const dim3 grid((unsigned) (((long long) n + 255) / 256));
    if (d_normals) hipLaunchKernelGGL(warp_points_kernel<true>, grid, dim3(256), 0, (hipStream_t) stream, a);
    else hipLaunchKernelGGL(warp_points_kernel<false>, grid, dim3(256), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

int sobfu_hip_sample_tsdf(const float* d_vol, int X, int Y, int Z, const float vs[3], const float R[9], const float t[3], int mc_vertices,
                          const float* d_points, int n, float* d_out, void* stream) {
    SOBFU_CHECK_ARGS(d_vol && vs && R && t && d_points && d_out && volume_ok(X, Y, Z, INT_MAX) && n >= 0);
    SOBFU_CHECK_ARGS(aligned(d_vol, 0, 8) && aligned(d_points, 0, 16) && aligned(d_out, 0, 4));
    SOBFU_CHECK_ARGS(positive_finite(vs[0]) && positive_finite(vs[1]) && positive_finite(vs[2]));
    if (n == 0) return 0;
    SampleTsdfArgs a{(const float2*) d_vol, point_map(X, Y, Z, vs, R, t, mc_vertices, n), (const float4*) d_points, d_out};
    hipLaunchKernelGGL(sample_tsdf_points_kernel, dim3((unsigned) (((long long) n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

}  // extern "C"
