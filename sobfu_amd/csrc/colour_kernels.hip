// Colour for gfx950: a canonical colour volume fused from registered BGRA frames through the deformation psi, its warp to live, and the
// samplers that put it on raycast views and marching-cubes vertices.
//
// The reference takes a colour image per frame (SobFusion::operator()(const Depth&, const Image&), include/sobfu/sob_fusion.hpp:44) and
// drops it; the rules below are this project's, and tests/colour_reference.py restates them in the same operation order (every TU is
// built with -ffp-contract=off: the fmaf below are the only fused operations).
//
//   volume     one uchar4 per voxel, kfusion::RGB order (b, g, r, a), dense and x fastest like the TSDF volumes; a = the colour weight
//              (0 = no colour)
//   integrate  voxel x of the TSDF about to be fused, read first: it is coloured only when the observation predicate of
//              integrate_fuse_kernel holds (weight != 0, and not weight 1 with tsdf 0 or -1) and |tsdf| < 1.  Then p = psi(x) (psi NULL:
//              p = x) in grid units, m = p * vs + vs / 2 (metres, the voxel centre of integrate_depth), cam = dot3(R_i, m) + t_i,
//              (u, v) = (fmaf(fx, cam.x / cam.z, cx), fmaf(fy, cam.y / cam.z, cy)) and integrate_depth's tests in its order: outside
//              [0, cols) x [0, rows) or cam.z <= 0 or NaN -> skipped; pixel (floorf u, floorf v).  With w = a:
//              c' = rintf(((float) c * (float) w + (float) c_new) / ((float) w + 1.f)) per channel, a' = min(w + 1, cap)
//   sampler    trilinear at grid point g with the clamp / upper-index rule of tri_setup; corner weight (wx * wy) * wz with w = 1 - t
//              for the lower and t for the upper index; corners with a == 0 are left out and the others renormalised:
//              c = min(255, rintf(sum_i w_i c_i / sum_i w_i)), the sums in corner order ggg, ggh, ghg, ghh, hgg, hgh, hhg, hhh (x
//              outermost, z innermost, g = lower, h = upper); a = 1.  No weighted corner with colour (sum w_i == 0): (0, 0, 0, 0)
//   apply      c_live(y) = sample(c_global, psi_inv(y))  (apply_kernel, field_kernels.hip)
//   sample     point p (float4) of a frame whose pose from the volume is (R, t): q = p, or (p.x, -p.y, -p.z) for marching-cubes
//              vertices (include/sobfu_hip.h, marching cubes); g_i = dot3(R^T_i, q - t) / vs_i - 0.5f (grid_position,
//              sobfu_frame.hpp); with a normals image, a point whose normal.w == 0 (a raycast miss) gives (0, 0, 0, 0)
//   render     I = 0.2 + 0.8 max(0, n . l), render_image_kernel's (lambert, sobfu_frame.hpp); a hit with colour: (c_i * I) rounded
//              to a byte per channel, alpha 255; a hit without colour: render_image's grey; a miss: (0, 0, 0, 0)
//
// Launch shapes: integrate / apply one lane per voxel, waves of 64 consecutive x (the TSDF read is 512 B per wave, coalesced); only
// the |tsdf| < 1 shell touches psi, the image and the colour volume.  Images and point lists: 64 x 4 lanes per workgroup.  No LDS.
#include "sobfu_frame.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"

using namespace sobfu_hip;

namespace {

struct ColourArgs {
    const uchar4* image;
    int image_step, rows, cols;
    const float2* tsdf;
    const float4* psi;  // NULL: identity
    uchar4* colour;
    Dims d;
    float vsx, vsy, vsz;
    float R[9], t[3];
    float fx, fy, cx, cy;
    int cap;
};

__global__ void __launch_bounds__(256) integrate_colour_kernel(ColourArgs a) {
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y, z = blockIdx.z;
    if (x >= a.d.x || y >= a.d.y) return;
    const size_t i = vidx(a.d, x, y, z);
    const float2 f = a.tsdf[i];
    if (f.y == 0.f || (f.y == 1.f && (f.x == 0.f || f.x == -1.f))) return;  // integrate_fuse_kernel's observation predicate
    if (!(fabsf(f.x) < 1.f)) return;
    float px = (float) x, py = (float) y, pz = (float) z;
    if (a.psi) {
        const float4 p = a.psi[i];
        px = p.x, py = p.y, pz = p.z;
    }
    const float mx = px * a.vsx + a.vsx / 2.f, my = py * a.vsy + a.vsy / 2.f, mz = pz * a.vsz + a.vsz / 2.f;
    const float camx = dot3(a.R + 0, mx, my, mz) + a.t[0];
    const float camy = dot3(a.R + 3, mx, my, mz) + a.t[1];
    const float camz = dot3(a.R + 6, mx, my, mz) + a.t[2];
    const float coox = __builtin_fmaf(a.fx, camx / camz, a.cx), cooy = __builtin_fmaf(a.fy, camy / camz, a.cy);
    if (coox < 0 || cooy < 0 || coox >= (float) a.cols || cooy >= (float) a.rows) return;
    if (!(camz > 0)) return;
    if (!(coox == coox) || !(cooy == cooy)) return;
    const int u = (int) floorf(coox), v = (int) floorf(cooy);
    const uchar4 n = row_ptr(a.image, a.image_step, v)[u];
    const uchar4 c = a.colour[i];
    const float w = (float) c.w, w1 = w + 1.f;
    auto avg = [&](unsigned char old, unsigned char obs) { return (unsigned char) rintf(((float) old * w + (float) obs) / w1); };
    a.colour[i] = make_uchar4(avg(c.x, n.x), avg(c.y, n.y), avg(c.z, n.z), (unsigned char) min((int) c.w + 1, a.cap));
}

// the colour sampler of the header comment
SOBFU_DEV uchar4 sample_colour_at(const uchar4* __restrict__ col, const Dims& d, float gx, float gy, float gz) {
    const Tri a = tri_setup(gx, d.x), b = tri_setup(gy, d.y), c = tri_setup(gz, d.z);
    const int xs[2] = {a.g, a.h}, ys[2] = {b.g, b.h}, zs[2] = {c.g, c.h};
    const float wx[2] = {1.f - a.t, a.t}, wy[2] = {1.f - b.t, b.t}, wz[2] = {1.f - c.t, c.t};
    float sb = 0.f, sg = 0.f, sr = 0.f, sw = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uchar4 v = col[vidx(d, xs[i], ys[j], zs[k])];
                if (v.w != 0) {
                    const float w = (wx[i] * wy[j]) * wz[k];
                    sb = sb + w * (float) v.x;
                    sg = sg + w * (float) v.y;
                    sr = sr + w * (float) v.z;
                    sw = sw + w;
                }
            }
    if (!(sw > 0.f)) return make_uchar4(0, 0, 0, 0);
    return make_uchar4((unsigned char) fminf(255.f, rintf(sb / sw)), (unsigned char) fminf(255.f, rintf(sg / sw)),
                       (unsigned char) fminf(255.f, rintf(sr / sw)), 1);
}

__global__ void __launch_bounds__(256) apply_colour_kernel(const uchar4* __restrict__ col, uchar4* __restrict__ out,
                                                           const float4* __restrict__ psi_inv, Dims d) {
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y, z = blockIdx.z;
    if (x >= d.x || y >= d.y) return;
    const size_t i = vidx(d, x, y, z);
    const float4 p = psi_inv[i];
    out[i] = sample_colour_at(col, d, p.x, p.y, p.z);
}

struct SampleArgs {
    const uchar4* col;
    Dims d;
    float vsx, vsy, vsz;
    float Rt[9], t[3];
    int flip;  // marching-cubes vertices: (x, -y, -z)
    const float4* points;
    int points_step;
    const float4* normals;  // NULL: every point is sampled
    int normals_step;
    int rows, cols;
    uchar4* out;
    int out_step;
};

__global__ void __launch_bounds__(256) sample_colour_kernel(SampleArgs a) {
    const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
    if (u >= a.cols || v >= a.rows) return;
    uchar4 px = make_uchar4(0, 0, 0, 0);
    const bool hit = !a.normals || row_ptr(a.normals, a.normals_step, v)[u].w != 0.f;
    if (hit) {
        float wx, wy, wz, gx, gy, gz;
        grid_position(a, row_ptr(a.points, a.points_step, v)[u], wx, wy, wz, gx, gy, gz);
        px = sample_colour_at(a.col, a.d, gx, gy, gz);
    }
    row_ptr(a.out, a.out_step, v)[u] = px;
}

struct RenderColourArgs {
    const float4* points;
    int points_step;
    const float4* normals;
    int normals_step;
    const uchar4* colour;
    int colour_step;
    int rows, cols;
    float lx, ly, lz;
    uchar4* image;
    int image_step;
};

__global__ void __launch_bounds__(256) render_colour_kernel(RenderColourArgs a) {
    const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
    if (u >= a.cols || v >= a.rows) return;
    const float4 n = row_ptr(a.normals, a.normals_step, v)[u];
    uchar4 px = make_uchar4(0, 0, 0, 0);
    if (n.w != 0.f) {
        const float I = lambert(n, row_ptr(a.points, a.points_step, v)[u], a.lx, a.ly, a.lz);
        const uchar4 c = row_ptr(a.colour, a.colour_step, v)[u];
        if (c.w != 0) {
            px = make_uchar4(to_byte((float) c.x * I), to_byte((float) c.y * I), to_byte((float) c.z * I), 255);
        } else {
            const unsigned char g = to_byte(255.f * I);
            px = make_uchar4(g, g, g, 255);
        }
    }
    row_ptr(a.image, a.image_step, v)[u] = px;
}

}  // namespace

extern "C" {

int sobfu_hip_integrate_colour(const uint8_t* d_image, int image_step, int rows, int cols, const float* d_tsdf, const float* d_psi,
                               uint8_t* d_colour, int X, int Y, int Z, const float vs[3], const float R[9], const float t[3], float fx, float fy,
                               float cx, float cy, int cap, void* stream) {
    SOBFU_CHECK_ARGS(d_image && d_tsdf && d_colour && vs && R && t);
    SOBFU_CHECK_ARGS(volume_ok(X, Y, Z, kGridZ) && rows >= 1 && cols >= 1 && (long long) image_step >= (long long) cols * 4);
    SOBFU_CHECK_ARGS(aligned(d_image, image_step, 4) && aligned(d_colour, 0, 4) && aligned(d_tsdf, 0, 8) && (!d_psi || aligned(d_psi, 0, 16)));
    SOBFU_CHECK_ARGS(cap >= 1 && cap <= 255);
    SOBFU_CHECK_ARGS(positive_finite(vs[0]) && positive_finite(vs[1]) && positive_finite(vs[2]));
    SOBFU_CHECK_ARGS(intr_ok(fx, fy, cx, cy));
    ColourArgs a{(const uchar4*) d_image, image_step, rows, cols, (const float2*) d_tsdf, (const float4*) d_psi, (uchar4*) d_colour, {X, Y, Z},
                 vs[0], vs[1], vs[2], {}, {}, fx, fy, cx, cy, cap};
    fill_pose(R, t, a.R, nullptr, a.t);
    hipLaunchKernelGGL(integrate_colour_kernel, voxel_grid(X, Y, Z), voxel_block(), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

int sobfu_hip_apply_colour(const uint8_t* d_colour, uint8_t* d_colour_warped, const float* d_psi_inv, int X, int Y, int Z, void* stream) {
    SOBFU_CHECK_ARGS(d_colour && d_colour_warped && d_psi_inv && d_colour != d_colour_warped && volume_ok(X, Y, Z, kGridZ));
    SOBFU_CHECK_ARGS(aligned(d_colour, 0, 4) && aligned(d_colour_warped, 0, 4) && aligned(d_psi_inv, 0, 16));
    hipLaunchKernelGGL(apply_colour_kernel, voxel_grid(X, Y, Z), voxel_block(), 0, (hipStream_t) stream, (const uchar4*) d_colour,
                       (uchar4*) d_colour_warped, (const float4*) d_psi_inv, Dims{X, Y, Z});
    return (int) hipGetLastError();
}

int sobfu_hip_sample_colour(const uint8_t* d_colour, int X, int Y, int Z, const float vs[3], const float R[9], const float t[3], int mc_vertices,
                            const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols, uint8_t* d_out,
                            int out_step, void* stream) {
    SOBFU_CHECK_ARGS(d_colour && vs && R && t && d_points && d_out && volume_ok(X, Y, Z, kGridZ) && rows >= 1 && cols >= 1 && rows <= 65535 * 4);
    SOBFU_CHECK_ARGS((long long) points_step >= (long long) cols * 16 && (long long) out_step >= (long long) cols * 4);
    SOBFU_CHECK_ARGS(!d_normals || (long long) normals_step >= (long long) cols * 16);
    SOBFU_CHECK_ARGS(aligned(d_colour, 0, 4) && aligned(d_points, points_step, 16) && aligned(d_out, out_step, 4));
    SOBFU_CHECK_ARGS(!d_normals || aligned(d_normals, normals_step, 16));
    SOBFU_CHECK_ARGS(positive_finite(vs[0]) && positive_finite(vs[1]) && positive_finite(vs[2]));
    SampleArgs a{(const uchar4*) d_colour, {X, Y, Z}, vs[0], vs[1], vs[2], {}, {}, mc_vertices ? 1 : 0, (const float4*) d_points, points_step,
                 (const float4*) d_normals, normals_step, rows, cols, (uchar4*) d_out, out_step};
    fill_pose(R, t, nullptr, a.Rt, a.t);
    hipLaunchKernelGGL(sample_colour_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

int sobfu_hip_render_colour(const float* d_points, int points_step, const float* d_normals, int normals_step, const uint8_t* d_colour_image,
                            int colour_step, int rows, int cols, float lx, float ly, float lz, uint8_t* d_image, int image_step, void* stream) {
    SOBFU_CHECK_ARGS(d_points && d_normals && d_colour_image && d_image && rows >= 1 && cols >= 1 && rows <= 65535 * 4);
    SOBFU_CHECK_ARGS((long long) points_step >= (long long) cols * 16 && (long long) normals_step >= (long long) cols * 16);
    SOBFU_CHECK_ARGS((long long) colour_step >= (long long) cols * 4 && (long long) image_step >= (long long) cols * 4);
    SOBFU_CHECK_ARGS(aligned(d_points, points_step, 16) && aligned(d_normals, normals_step, 16) && aligned(d_colour_image, colour_step, 4) &&
                     aligned(d_image, image_step, 4));
    RenderColourArgs a{(const float4*) d_points, points_step, (const float4*) d_normals, normals_step, (const uchar4*) d_colour_image,
                       colour_step, rows, cols, lx, ly, lz, (uchar4*) d_image, image_step};
    hipLaunchKernelGGL(render_colour_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

}  // extern "C"
