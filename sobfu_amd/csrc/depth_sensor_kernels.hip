// A depth sensor's view of a clean render on gfx950: the float4 point and normal images of sobfu_hip_mesh_render or
// sobfu_hip_raycast into the uint16 millimetre frame a structured-light camera would report, with a flag per pixel saying what became of
// it.  The reference has no such step; the rule is this project's (include/sobfu_hip.h states it, tests/depth_sensor_reference.py restates
// it operation by operation), after Nguyen, Izadi and Lovell (3DIMPVT 2012) for the axial noise and ICL-NUIM (Handa et al., ICRA 2014)
// for the jitter and the disparity quantisation.  The random numbers are sobfu_random.hpp's: every draw is a function of (seed, frame,
// pixel, stream), so no state is kept and nothing about the launch can change a bit of the frame.
//
//   tile     a 16 x 16 workgroup stages z and the hit bit of its pixels plus a halo of 4 + edge_radius pixels in LDS, once: the jitter
//            moves a pixel's source by at most 4, the edge window reaches edge_radius beyond that.  A tile cell outside the frame is
//            marked as such (it is no part of any window); the miss, range and edge steps of every lane read the tile, the grazing step
//            reads x, y and the normal of the one source pixel from memory.
//   lanes    of a workgroup beyond the frame's right or bottom border stage their share and write nothing.
#include "sobfu_frame.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_random.hpp"

using namespace sobfu_hip;

namespace {

constexpr int kTile = 16, kJitter = 4, kMaxRadius = 3;
constexpr int kMaxSide = kTile + 2 * (kJitter + kMaxRadius);
constexpr unsigned char kCellMiss = 0, kCellHit = 1, kCellOutside = 2;

struct SensorArgs {
    const float4* points;
    int points_step;
    const float4* normals;
    int normals_step;
    int rows, cols;
    sobfu_hip_sensor_params p;
    unsigned short* depth;
    int depth_step;
    unsigned char* flags;  // may be null
    int flags_step;
};

SOBFU_DEV int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }
SOBFU_DEV int jitter(float g, float lateral) { return (int) fminf(4.f, fmaxf(-4.f, rintf(g * lateral))); }

__global__ void __launch_bounds__(kTile * kTile) depth_sensor_kernel(SensorArgs a) {
    __shared__ float tile_z[kMaxSide * kMaxSide];
    __shared__ unsigned char tile_hit[kMaxSide * kMaxSide];
    const sobfu_hip_sensor_params& p = a.p;
    const int r = p.edge_radius, halo = kJitter + r, side = kTile + 2 * halo;
    const int u0 = (int) blockIdx.x * kTile - halo, v0 = (int) blockIdx.y * kTile - halo;
    for (int i = (int) threadIdx.x; i < side * side; i += kTile * kTile) {
        const int ty = i / side, tx = i - ty * side, qu = u0 + tx, qv = v0 + ty;
        float z = 0.f;
        unsigned char hit = kCellOutside;
        if (qu >= 0 && qu < a.cols && qv >= 0 && qv < a.rows) {
            hit = row_ptr(a.normals, a.normals_step, qv)[qu].w == 0.f ? kCellMiss : kCellHit;
            z   = row_ptr(a.points, a.points_step, qv)[qu].z;
        }
        tile_z[i] = z, tile_hit[i] = hit;
    }
    __syncthreads();
    const int lx = (int) threadIdx.x % kTile, ly = (int) threadIdx.x / kTile;
    const int u = (int) blockIdx.x * kTile + lx, v = (int) blockIdx.y * kTile + ly;
    if (u >= a.cols || v >= a.rows) return;

    const float g0 = normal_variate(pixel_draw(p.seed, p.frame, u, v, 0)), g1 = normal_variate(pixel_draw(p.seed, p.frame, u, v, 1));
    const float g2 = normal_variate(pixel_draw(p.seed, p.frame, u, v, 2));
    const Philox w3 = pixel_draw(p.seed, p.frame, u, v, 3);
    const float U0 = uniform_variate(w3.w[0]), U1 = uniform_variate(w3.w[1]);

    const int su = clampi(u + jitter(g0, p.lateral), 0, a.cols - 1), sv = clampi(v + jitter(g1, p.lateral), 0, a.rows - 1);
    const int sx = su - u0, sy = sv - v0;  // the source pixel in the tile: |su - u| <= 4, so r <= sx < side - r
    unsigned short mm_out = 0;
    unsigned char flag;
    const float z = tile_z[sy * side + sx];
    if (tile_hit[sy * side + sx] == kCellMiss) {
        flag = SOBFU_SENSOR_MISS;
    } else if (!(z > p.z_min && z <= p.z_max)) {
        flag = SOBFU_SENSOR_RANGE;
    } else {
        const float4 P = row_ptr(a.points, a.points_step, sv)[su], N = row_ptr(a.normals, a.normals_step, sv)[su];
        const float l = __builtin_sqrtf((P.x * P.x + P.y * P.y) + z * z);
        const float c = fabsf((N.x * P.x + N.y * P.y) + N.z * z) / l;
        bool edge = false;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const int q = (sy + dy) * side + (sx + dx);
                const unsigned char h = tile_hit[q];
                edge = edge || h == kCellMiss || (h == kCellHit && fabsf(tile_z[q] - z) > p.edge_jump);
            }
        if (c < p.cos_min) {
            flag = SOBFU_SENSOR_GRAZING;
        } else if (r > 0 && edge && U0 < p.edge_drop) {
            flag = SOBFU_SENSOR_EDGE;
        } else if (U1 < p.drop) {
            flag = SOBFU_SENSOR_DROPOUT;
        } else {
            const float dz = z - p.z0, cc = c * c;
            const float sigma = (p.a0 + p.a1 * (dz * dz)) + p.a2 * (((1.f - cc) / cc) / __builtin_sqrtf(z));
            float zn = z + g2 * sigma;
            bool in_range = true;
            if (p.disparity > 0.f) {
                const float q = rintf(p.disparity / zn);
                in_range = q >= 1.f;
                zn = p.disparity / q;
            }
            const float mm = rintf(1000.f * zn);
            in_range = in_range && mm >= 1.f && mm <= 65535.f;
            flag = in_range ? SOBFU_SENSOR_VALID : SOBFU_SENSOR_RANGE;
            if (in_range) mm_out = (unsigned short) mm;
        }
    }
    row_ptr(a.depth, a.depth_step, v)[u] = mm_out;
    if (a.flags) row_ptr(a.flags, a.flags_step, v)[u] = flag;
}

__global__ void __launch_bounds__(256) philox_kernel(const uint32_t* __restrict__ counters, uint32_t k0, uint32_t k1, int n, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = counters + 4 * (size_t) i;
    const Philox r = philox4x32_10(c[0], c[1], c[2], c[3], k0, k1);
    for (int k = 0; k < 4; ++k) out[4 * (size_t) i + k] = r.w[k];
}

bool unit(float x) { return x >= 0.f && x <= 1.f; }  // a NaN fails
bool image_ok(const void* ptr, int step, int cols, int size) { return ptr && (long long) step >= (long long) cols * size && aligned(ptr, step, size); }

bool params_ok(const sobfu_hip_sensor_params* p) {
    if (!p) return false;
    const float finite[] = {p->lateral, p->z_min, p->a0, p->a1, p->z0, p->a2, p->disparity};
    return finite_all(finite, 7) && p->lateral >= 0.f && !std::isnan(p->z_max) && unit(p->cos_min) && p->edge_radius >= 0 && p->edge_radius <= kMaxRadius &&
           p->edge_jump >= 0.f && unit(p->edge_drop) && unit(p->drop) && p->disparity >= 0.f;
}

}  // namespace

extern "C" {

int sobfu_hip_philox4x32_10(const uint32_t* d_counters, const uint32_t key[2], int n, uint32_t* d_out, void* stream) {
    SOBFU_CHECK_ARGS(d_counters && key && d_out && n >= 0 && aligned(d_counters, 0, 4) && aligned(d_out, 0, 4));
    if (n == 0) return 0;
    hipLaunchKernelGGL(philox_kernel, dim3((unsigned) (((long long) n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, d_counters, key[0], key[1], n, d_out);
    return (int) hipGetLastError();
}

int sobfu_hip_depth_sensor(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols,
                           const sobfu_hip_sensor_params* p, uint16_t* d_depth, int depth_step, uint8_t* d_flags, int flags_step, void* stream) {
    SOBFU_CHECK_ARGS(rows >= 0 && cols >= 0 && params_ok(p));
    SOBFU_CHECK_ARGS(image_ok(d_points, points_step, cols, 16) && image_ok(d_normals, normals_step, cols, 16) && image_ok(d_depth, depth_step, cols, 2));
    SOBFU_CHECK_ARGS(!d_flags || image_ok(d_flags, flags_step, cols, 1));
    if (rows == 0 || cols == 0) return 0;
    const SensorArgs a{(const float4*) d_points, points_step, (const float4*) d_normals, normals_step, rows, cols, *p, d_depth, depth_step, d_flags, flags_step};
    hipLaunchKernelGGL(depth_sensor_kernel, dim3((unsigned) ((cols + kTile - 1) / kTile), (unsigned) ((rows + kTile - 1) / kTile)), dim3(kTile * kTile), 0,
                       (hipStream_t) stream, a);
    return (int) hipGetLastError();
}

}  // extern "C"
