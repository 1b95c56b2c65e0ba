// Rendering of TSDF volumes for gfx950: a KinectFusion-style raycaster (one ray per pixel, marched through the trilinear TSDF),
// Lambertian shading and normal colouring into 8-bit BGRA images.
//
// The reference declares kfusion::cuda::renderImage / renderTangentColors (include/kfusion/cuda/imgproc.hpp:30,42-46) but defines
// neither, and has no raycaster at all; the rules below are this project's, and tests/render_reference.py restates them in the
// same operation order (every TU is built with -ffp-contract=off: the fmaf below are the only fused operations).
//
//   ray      pixel (u, v) -> d = ((u - cx) / fx, (v - cy) / fy, 1), parameter = camera depth z; in grid units the sample at z is
//            g = fmaf(z, D, O) with D = (R^T d) / vs and O = (-R^T t) / vs - 0.5 (R^T, -R^T t from the host in double)
//   clip     slab test against g in [0, dim - 1] per axis, and z >= 0
//   sampler  trilinear tsdf with the clamp / upper-index rule of tri_setup; valid when all 8 corner weights are > 0 (sample_tsdf,
//            sobfu_frame.hpp)
//   march    step (in metres of ray length) = (valid && f > 0) ? max(fine, 0.8 f trunc) : fine, fine = step_factor * min(vs);
//            hit = previous sample valid with f > 0, current sample valid with f < 0; one secant step refines z
//   output   point (z d, 0), normal (normalize(R grad f), 1); grad f by central differences at +-1 grid unit (clamped into the box)
//            over 2 vs; a miss (or a zero gradient) writes zeros, so normal.w is the hit flag
//
// Launch shape of the raycaster: 256-thread workgroups of 16 x 16 pixels, each 64-lane wave an 8 x 8 tile, so the rays of a wave
// are neighbours in both image directions and gather the same cache lines of the volume.  No LDS.
#include "sobfu_frame.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"

#include <cmath>

using namespace sobfu_hip;

namespace {

struct RaycastArgs {
    const float2* vol;
    Dims d;
    float vsx, vsy, vsz, trunc;
    float R[9];   // vol2cam rotation (normals to the camera frame)
    float Rt[9];  // R^T (rays to the volume frame)
    float o[3];   // -R^T t: the camera centre in volume metres
    float fx, fy, cx, cy;
    int rows, cols;
    float fine;     // step_factor * min(vs), metres of ray length
    int max_steps;  // the box diagonal over fine, + 2: no ray inside the box takes more steps (a bound, never reached by a march)
    float4* points;
    int points_step;
    float4* normals;
    int normals_step;
};

// [tmin, tmax] &= the z range where o + z D stays in [0, top] (one slab; D == 0: all or nothing)
SOBFU_DEV void clip_slab(float o, float D, float top, float& tmin, float& tmax) {
    if (D == 0.f) {
        if (!(o >= 0.f && o <= top)) tmin = INFINITY;
        return;
    }
    const float t0 = (0.f - o) / D, t1 = (top - o) / D;
    tmin = fmaxf(tmin, fminf(t0, t1));
    tmax = fminf(tmax, fmaxf(t0, t1));
}

__global__ void __launch_bounds__(256) raycast_kernel(RaycastArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= a.cols || v >= a.rows) return;
    float4* P = row_ptr(a.points, a.points_step, v) + u;
    float4* N = row_ptr(a.normals, a.normals_step, v) + u;

    const float dx = ((float) u - a.cx) / a.fx, dy = ((float) v - a.cy) / a.fy;
    const float Dx = dot3(a.Rt + 0, dx, dy, 1.f) / a.vsx, Dy = dot3(a.Rt + 3, dx, dy, 1.f) / a.vsy, Dz = dot3(a.Rt + 6, dx, dy, 1.f) / a.vsz;
    const float Ox = a.o[0] / a.vsx - 0.5f, Oy = a.o[1] / a.vsy - 0.5f, Oz = a.o[2] / a.vsz - 0.5f;
    const float inv_len = 1.f / __builtin_sqrtf(dx * dx + dy * dy + 1.f);  // dz per metre of ray length

    float tmin = 0.f, tmax = INFINITY;
    clip_slab(Ox, Dx, (float) (a.d.x - 1), tmin, tmax);
    clip_slab(Oy, Dy, (float) (a.d.y - 1), tmin, tmax);
    clip_slab(Oz, Dz, (float) (a.d.z - 1), tmin, tmax);

    float4 pt = make_float4(0.f, 0.f, 0.f, 0.f), nm = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tmin <= tmax) {
        float z = tmin;
        bool valid;
        float f = sample_tsdf(a.vol, a.d, __builtin_fmaf(z, Dx, Ox), __builtin_fmaf(z, Dy, Oy), __builtin_fmaf(z, Dz, Oz), valid);
        for (int i = 0; i < a.max_steps; ++i) {
            const float ds = (valid && f > 0.f) ? fmaxf(a.fine, 0.8f * f * a.trunc) : a.fine;
            const float zp = z, fp = f;
            const bool vp = valid;
            z = __builtin_fmaf(ds, inv_len, z);
            if (!(z <= tmax) || !(z > zp)) break;
            f = sample_tsdf(a.vol, a.d, __builtin_fmaf(z, Dx, Ox), __builtin_fmaf(z, Dy, Oy), __builtin_fmaf(z, Dz, Oz), valid);
            if (vp && fp > 0.f && valid && f < 0.f) {
                const float zs = zp + (z - zp) * fp / (fp - f);
                const float gx = __builtin_fmaf(zs, Dx, Ox), gy = __builtin_fmaf(zs, Dy, Oy), gz = __builtin_fmaf(zs, Dz, Oz);
                const float tx = (float) (a.d.x - 1), ty = (float) (a.d.y - 1), tz = (float) (a.d.z - 1);
                const float nx = (sample_tsdf_only(a.vol, a.d, fminf(gx + 1.f, tx), gy, gz) - sample_tsdf_only(a.vol, a.d, fmaxf(gx - 1.f, 0.f), gy, gz)) / (2.f * a.vsx);
                const float ny = (sample_tsdf_only(a.vol, a.d, gx, fminf(gy + 1.f, ty), gz) - sample_tsdf_only(a.vol, a.d, gx, fmaxf(gy - 1.f, 0.f), gz)) / (2.f * a.vsy);
                const float nz = (sample_tsdf_only(a.vol, a.d, gx, gy, fminf(gz + 1.f, tz)) - sample_tsdf_only(a.vol, a.d, gx, gy, fmaxf(gz - 1.f, 0.f))) / (2.f * a.vsz);
                const float cx = dot3(a.R + 0, nx, ny, nz), cy = dot3(a.R + 3, nx, ny, nz), cz = dot3(a.R + 6, nx, ny, nz);
                const float len = __builtin_sqrtf(cx * cx + cy * cy + cz * cz);
                if (len > 0.f) {
                    pt = make_float4(zs * dx, zs * dy, zs, 0.f);
                    nm = make_float4(cx / len, cy / len, cz / len, 1.f);
                }
                break;
            }
        }
    }
    *P = pt;
    *N = nm;
}

struct ShadeArgs {
    const float4* points;
    int points_step;
    const float4* normals;
    int normals_step;
    int rows, cols;
    float lx, ly, lz;
    uchar4* image;
    int image_step;
};

// renderImage: headlight-style Lambertian grey, I = 0.2 + 0.8 max(0, n . l), BGRA
__global__ void __launch_bounds__(256) render_image_kernel(ShadeArgs a) {
    const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
    if (u >= a.cols || v >= a.rows) return;
    const float4 n = row_ptr(a.normals, a.normals_step, v)[u];
    uchar4 px = make_uchar4(0, 0, 0, 0);
    if (n.w != 0.f) {
        const unsigned char g = to_byte(255.f * lambert(n, row_ptr(a.points, a.points_step, v)[u], a.lx, a.ly, a.lz));
        px = make_uchar4(g, g, g, 255);
    }
    row_ptr(a.image, a.image_step, v)[u] = px;
}

// renderTangentColors: (r, g, b) = (n * 0.5 + 0.5) * 255, BGRA
__global__ void __launch_bounds__(256) render_normals_kernel(ShadeArgs a) {
    const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
    if (u >= a.cols || v >= a.rows) return;
    const float4 n = row_ptr(a.normals, a.normals_step, v)[u];
    uchar4 px = make_uchar4(0, 0, 0, 0);
    if (n.w != 0.f) px = make_uchar4(to_byte((n.z * 0.5f + 0.5f) * 255.f), to_byte((n.y * 0.5f + 0.5f) * 255.f), to_byte((n.x * 0.5f + 0.5f) * 255.f), 255);
    row_ptr(a.image, a.image_step, v)[u] = px;
}

}  // namespace

extern "C" {

int sobfu_hip_raycast(const float* d_vol, int X, int Y, int Z, float vsx, float vsy, float vsz, float trunc, const float R[9], const float t[3],
                      float fx, float fy, float cx, float cy, int rows, int cols, float step_factor, float* d_points, int points_step,
                      float* d_normals, int normals_step, void* stream) {
    SOBFU_CHECK_ARGS(d_vol && R && t && d_points && d_normals);
    SOBFU_CHECK_ARGS(X >= 2 && Y >= 2 && Z >= 2 && rows >= 1 && cols >= 1);
    SOBFU_CHECK_ARGS(points_step >= cols * 16 && normals_step >= cols * 16);
    SOBFU_CHECK_ARGS(aligned(d_points, points_step, 16) && aligned(d_normals, normals_step, 16));
    SOBFU_CHECK_ARGS(positive_finite(trunc) && positive_finite(step_factor));
    SOBFU_CHECK_ARGS(positive_finite(vsx) && positive_finite(vsy) && positive_finite(vsz));
    SOBFU_CHECK_ARGS(intr_ok(fx, fy, cx, cy) && finite_all(R, 9) && finite_all(t, 3));
    RaycastArgs a{(const float2*) d_vol, {X, Y, Z}, vsx, vsy, vsz, trunc, {}, {}, {}, fx, fy, cx, cy, rows, cols, 0.f, 0,
                  (float4*) d_points, points_step, (float4*) d_normals, normals_step};
    fill_pose(R, t, a.R, a.Rt, nullptr);
    for (int i = 0; i < 3; ++i) {
        double o = 0.0;
        for (int j = 0; j < 3; ++j) o -= (double) R[3 * j + i] * (double) t[j];
        a.o[i] = (float) o;
    }
    a.fine = step_factor * fminf(vsx, fminf(vsy, vsz));
    const double ex = (double) (X - 1) * vsx, ey = (double) (Y - 1) * vsy, ez = (double) (Z - 1) * vsz;
    const double steps = std::sqrt(ex * ex + ey * ey + ez * ez) / (double) a.fine + 2.0;
    if (!(steps < 1e6)) return SOBFU_E_UNSUPPORTED;  // a step this small against the box is not a raycast anyone can wait for
    a.max_steps = (int) steps;
    hipLaunchKernelGGL(raycast_kernel, dim3((unsigned) ((cols + 15) / 16), (unsigned) ((rows + 15) / 16)), dim3(256), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

int sobfu_hip_render_image(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols, float lx,
                           float ly, float lz, uint8_t* d_image, int image_step, void* stream) {
    SOBFU_CHECK_ARGS(d_points && d_normals && d_image && rows >= 1 && cols >= 1);
    SOBFU_CHECK_ARGS(points_step >= cols * 16 && normals_step >= cols * 16 && image_step >= cols * 4);
    SOBFU_CHECK_ARGS(aligned(d_points, points_step, 16) && aligned(d_normals, normals_step, 16) && aligned(d_image, image_step, 4));
    ShadeArgs a{(const float4*) d_points, points_step, (const float4*) d_normals, normals_step, rows, cols, lx, ly, lz, (uchar4*) d_image, image_step};
    hipLaunchKernelGGL(render_image_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

int sobfu_hip_render_normals(const float* d_normals, int normals_step, int rows, int cols, uint8_t* d_image, int image_step, void* stream) {
    SOBFU_CHECK_ARGS(d_normals && d_image && rows >= 1 && cols >= 1);
    SOBFU_CHECK_ARGS(normals_step >= cols * 16 && image_step >= cols * 4);
    SOBFU_CHECK_ARGS(aligned(d_normals, normals_step, 16) && aligned(d_image, image_step, 4));
    ShadeArgs a{nullptr, 0, (const float4*) d_normals, normals_step, rows, cols, 0.f, 0.f, 0.f, (uchar4*) d_image, image_step};
    hipLaunchKernelGGL(render_normals_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

}  // extern "C"
