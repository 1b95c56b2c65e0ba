// Camera tracking for gfx950: the image pyramids and normal maps of KinectFusion's projective ICP and the whole coarse-to-fine ICP loop,
// kept on the device.
//
// The reference carries kfusion::cuda::ProjectiveICP (src/kfusion/projective_icp.cpp, src/kfusion/cuda/proj_icp.cu) and the image helpers
// of include/kfusion/cuda/imgproc.hpp but never calls them.  Its loop makes two launches per iteration, copies the 27 sums to the host,
// synchronises and solves with OpenCV.  Here one iteration is two launches that read and write the pose in device memory -- a
// correspondence + reduction kernel and a one-workgroup solve -- so an estimate is a chain of launches on one stream with no host
// synchronisation (it can be captured into a graph).  tests/icp_reference.py restates the rules below in the same operation order (every
// TU is built with -ffp-contract=off; there is no fused operation and no fast division in this file).
//
//   pyramid      half resolution: dst(x, y) averages, in integer arithmetic (sum / count, truncating), the samples of the window
//                rows [max(0, 2y - 2), min(2y + 3, rows - 1)) x cols [max(0, 2x - 2), min(2x + 3, cols - 1)) of src with
//                |val - centre| < 3 sigma_depth 1000 (int compared as float), centre = src(2y, 2x); 0 when none qualifies.  The clipped
//                upper bounds are the reference's (pyramid_kernel): they drop the last row / column of the image.  Bit-exact by construction.
//   reproject    z = depth * 0.001f; p = (z * (u - cx) * finv_x, z * (v - cy) * finv_y, z) with finv = 1.f / f, left to right
//   normals      at (x, y) < (cols - 1, rows - 1) with z00 * z01 * z10 != 0: c = cross(v01 - v00, v10 - v00) (component order of
//                kfusion's cross), n = -(c / sqrtf(c . c)) per component (IEEE sqrt and division, not rsqrt), point = (v00, 0),
//                normal = (n, 0); elsewhere point and normal are (NaN, NaN, NaN, NaN) -- the reference's convention.
//                normals_mask_depth writes normal (NaN, NaN, NaN, 0) at the invalid pixels and, in a second launch, zeroes the depth
//                where normal.x is NaN.
//   resize       half resolution of (depth, normals): d = (d00 + d01 + d10 + d11) / 4 (int) when all four depths are non-zero, and
//                n = (n00 + n01 + n10 + n11) * 0.25f per component (left to right), w = 0; else d = 0, n = NaN.
//                Of (points, normals): when the four source pixels are all VALID (below), p = (p00 + p01 + p10 + p11) * 0.25f and n alike,
//                w = 0; else both NaN.  The reference tests only the points for NaN; the validity rule also refuses the raycaster's misses
//                (all zeros), which the reference's rule would average into the neighbouring hits.
//   valid        a pixel is valid iff its point and normal are finite in x, y, z and the normal is non-zero.  This takes the reference's
//                NaN misses and this repository's raycaster misses (zeros, normal.w == 0) alike.  In depth mode the point is valid iff the
//                depth is non-zero.
//   level intr   level l of base intrinsics (fx, fy, cx, cy): f = fx / 2^l, c = cx / 2^l (float division), finv = 1.f / f
//   correspond   per current pixel (x, y), with aff = (R row-major, t) read from device memory:
//                  points mode: s0 = vcurr(y, x); depth mode: s0 = reproject(x, y, dcurr(y, x)); invalid (s0, ncurr(y, x)) -> code 40
//                  s = R s0 + t, each row r0 * x + r1 * y + r2 * z + t (left to right)
//                  u = f_x * (s.x / s.z) + c_x, v likewise; s.z <= 0 or u < 0 or v < 0 or u >= cols or v >= rows -> 80
//                  target pixel (ui, vi) = ((int) floorf(u + 0.5f), (int) floorf(v + 0.5f)); ui >= cols or vi >= rows -> 80
//                  points mode: d = vprev(vi, ui); depth mode: d = reproject(u, v, dprev(vi, ui)) at the unrounded (u, v);
//                  nd = nprev(vi, ui); invalid (d, nd) -> 120
//                  |s - d|^2 = dx * dx + dy * dy + dz * dz with d* = s* - d* > dist^2 -> 160
//                  ns = R ncurr(y, x); fabsf(ns . nd) < cos(angle) -> 200; else code 0 and the row
//                  [cross(s, nd), nd | r], r = nd.x * (d.x - s.x) + nd.y * (d.y - s.y) + nd.z * (d.z - s.z)
//                The reference samples the previous frame through tex2D point filtering, which truncates (u, v): a projection that lands
//                a rounding error below an integer pixel then fetches the neighbour.  The nearest pixel is used here on purpose, so that
//                two identical frames correspond pixel for pixel.
//   sums         29 values per inlier: the 21 upper-triangular products row_i * row_j (i <= j < 6, row-major), the 6 products
//                row_i * r, 1 (the inlier count) and r * r.  All in fp32; the products of outliers are not added.
//   solve        in fp64: sums of the partials in slab order; A (symmetric) x = b by LDL^T with D_j = A_jj - sum_k<j L_jk^2 D_k and
//                L_ij = (A_ij - sum_k<j L_ik L_jk D_k) / D_j; det A = prod D_j.  Failure -- |det| < 1e-15, det NaN (the reference's
//                null-space check) or a pivot D_j <= 0 -- leaves the pose and records 0x10000 | level << 8 | iteration in the status
//                word (the first failure ends the estimate: every later launch sees status != 0 and exits at once).  Else
//                Tinc = (Rodrigues(x0..2), x3..5) -- theta = |w|, theta == 0 gives I exactly, else
//                R = cos I + (1 - cos) k k^T + sin [k]x with k = w / theta -- and aff = Tinc * aff in fp64, rounded to float.
//
// Launch shape of the correspondence kernel: 256-thread workgroups, grid-stride over the row-major pixels with at most kMaxParts
// workgroups, so a lane handles several pixels (about 5 at 640 x 480).  Each lane accumulates its 29 sums in registers; a workgroup
// reduces them with a wave64 __shfl_xor butterfly and then across its 4 waves through LDS (wave 0 + 1 + 2 + 3, in that order), and writes
// one 32-float slab.  No float atomics anywhere: the sums, and so the pose, are bitwise reproducible.  The solve is one 256-thread
// workgroup: thread j converts slab j to fp64, the same butterfly and LDS order reduce the slabs, lane 0 solves.  Every index of the
// 6 x 6 system is a compile-time constant (fully unrolled loops): nothing goes to scratch.  The sums of a row, the workgroup reduction,
// the unpacking into A x = b, the pose update and the four launch constants (kMaxParts = the solve's workgroup size) are
// sobfu_normal_eq.hpp's, shared with mesh_align_kernels.hip; the LDL^T, Rodrigues and the pose composition are sobfu_rigid.hpp's.
#include "sobfu_frame.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_normal_eq.hpp"

#include <cmath>

using namespace sobfu_hip;

namespace {

SOBFU_DEV bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }
SOBFU_DEV bool valid_pn(const float4& p, const float4& n) {
    return finite3(p.x, p.y, p.z) && finite3(n.x, n.y, n.z) && (n.x != 0.f || n.y != 0.f || n.z != 0.f);
}
SOBFU_DEV float4 nan4() { return make_float4(NAN, NAN, NAN, NAN); }

struct Reproj {
    float fx, fy, cx, cy, fxinv, fyinv;
    SOBFU_DEV float3 operator()(float u, float v, float z) const { return make_float3(z * (u - cx) * fxinv, z * (v - cy) * fyinv, z); }
};

// ---- image kernels (64 x 4 workgroups, one pixel per thread) -------------------------------------------------------------------
__global__ void __launch_bounds__(256) pyramid_kernel(const uint16_t* __restrict__ src, int sstep, int rows, int cols, uint16_t* __restrict__ dst,
                                                      int dstep, int drows, int dcols, float thr) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dcols || y >= drows) return;
    const int centre = row_ptr(src, sstep, 2 * y)[2 * x];
    const int tx = min(2 * x - 2 + 5, cols - 1), ty = min(2 * y - 2 + 5, rows - 1);
    int sum = 0, count = 0;
    for (int cy = max(0, 2 * y - 2); cy < ty; ++cy) {
        const uint16_t* r = row_ptr(src, sstep, cy);
        for (int cx = max(0, 2 * x - 2); cx < tx; ++cx) {
            const int val = r[cx];
            if ((float) abs(val - centre) < thr) {
                sum += val;
                ++count;
            }
        }
    }
    row_ptr(dst, dstep, y)[x] = (uint16_t) (count == 0 ? 0 : sum / count);
}

// normal (and point) of pixel (x, y) from depth; false where the reference writes NaN
SOBFU_DEV bool normal_at(const uint16_t* __restrict__ depth, int step, int rows, int cols, const Reproj& rp, int x, int y, float3& v00, float3& n) {
    if (x >= cols - 1 || y >= rows - 1) return false;
    const float z00 = row_ptr(depth, step, y)[x] * 0.001f, z01 = row_ptr(depth, step, y)[x + 1] * 0.001f, z10 = row_ptr(depth, step, y + 1)[x] * 0.001f;
    if (!(z00 * z01 * z10 != 0.f)) return false;
    v00 = rp((float) x, (float) y, z00);
    const float3 v01 = rp((float) (x + 1), (float) y, z01), v10 = rp((float) x, (float) (y + 1), z10);
    const float ax = v01.x - v00.x, ay = v01.y - v00.y, az = v01.z - v00.z;
    const float bx = v10.x - v00.x, by = v10.y - v00.y, bz = v10.z - v00.z;
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const float len = __builtin_sqrtf(cx * cx + cy * cy + cz * cz);
    n = make_float3(-(cx / len), -(cy / len), -(cz / len));
    return true;
}

__global__ void __launch_bounds__(256) point_normals_kernel(const uint16_t* __restrict__ depth, int dstep, int rows, int cols, Reproj rp,
                                                            float4* __restrict__ points, int pstep, float4* __restrict__ normals, int nstep) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    float3 v, n;
    const bool ok = normal_at(depth, dstep, rows, cols, rp, x, y, v, n);
    row_ptr(points, pstep, y)[x] = ok ? make_float4(v.x, v.y, v.z, 0.f) : nan4();
    row_ptr(normals, nstep, y)[x] = ok ? make_float4(n.x, n.y, n.z, 0.f) : nan4();
}

__global__ void __launch_bounds__(256) normals_kernel(const uint16_t* __restrict__ depth, int dstep, int rows, int cols, Reproj rp,
                                                      float4* __restrict__ normals, int nstep) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    float3 v, n;
    const bool ok = normal_at(depth, dstep, rows, cols, rp, x, y, v, n);
    row_ptr(normals, nstep, y)[x] = ok ? make_float4(n.x, n.y, n.z, 0.f) : make_float4(NAN, NAN, NAN, 0.f);
}

__global__ void __launch_bounds__(256) mask_depth_kernel(const float4* __restrict__ normals, int nstep, uint16_t* __restrict__ depth, int dstep,
                                                         int rows, int cols) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    if (__builtin_isnan(row_ptr(normals, nstep, y)[x].x)) row_ptr(depth, dstep, y)[x] = 0;
}

SOBFU_DEV float4 avg4(const float4& a, const float4& b, const float4& c, const float4& d) {
    return make_float4((a.x + b.x + c.x + d.x) * 0.25f, (a.y + b.y + c.y + d.y) * 0.25f, (a.z + b.z + c.z + d.z) * 0.25f, 0.f);
}

__global__ void __launch_bounds__(256) resize_depth_normals_kernel(const uint16_t* __restrict__ ds, int dsstep, const float4* __restrict__ ns, int nsstep,
                                                                   uint16_t* __restrict__ dd, int ddstep, float4* __restrict__ nd, int ndstep, int drows,
                                                                   int dcols) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dcols || y >= drows) return;
    const int xs = 2 * x, ys = 2 * y;
    const int d00 = row_ptr(ds, dsstep, ys)[xs], d01 = row_ptr(ds, dsstep, ys)[xs + 1];
    const int d10 = row_ptr(ds, dsstep, ys + 1)[xs], d11 = row_ptr(ds, dsstep, ys + 1)[xs + 1];
    uint16_t d = 0;
    float4 n = nan4();
    if (d00 != 0 && d01 != 0 && d10 != 0 && d11 != 0) {  // not d00 * d01: the product of two depths >= 46341 overflows int
        d = (uint16_t) ((d00 + d01 + d10 + d11) / 4);
        n = avg4(row_ptr(ns, nsstep, ys)[xs], row_ptr(ns, nsstep, ys)[xs + 1], row_ptr(ns, nsstep, ys + 1)[xs], row_ptr(ns, nsstep, ys + 1)[xs + 1]);
    }
    row_ptr(dd, ddstep, y)[x] = d;
    row_ptr(nd, ndstep, y)[x] = n;
}

__global__ void __launch_bounds__(256) resize_points_normals_kernel(const float4* __restrict__ ps, int psstep, const float4* __restrict__ ns, int nsstep,
                                                                    float4* __restrict__ pd, int pdstep, float4* __restrict__ nd, int ndstep, int drows,
                                                                    int dcols) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dcols || y >= drows) return;
    const int xs = 2 * x, ys = 2 * y;
    const float4 p00 = row_ptr(ps, psstep, ys)[xs], p01 = row_ptr(ps, psstep, ys)[xs + 1];
    const float4 p10 = row_ptr(ps, psstep, ys + 1)[xs], p11 = row_ptr(ps, psstep, ys + 1)[xs + 1];
    const float4 n00 = row_ptr(ns, nsstep, ys)[xs], n01 = row_ptr(ns, nsstep, ys)[xs + 1];
    const float4 n10 = row_ptr(ns, nsstep, ys + 1)[xs], n11 = row_ptr(ns, nsstep, ys + 1)[xs + 1];
    float4 p = nan4(), n = nan4();
    if (valid_pn(p00, n00) && valid_pn(p01, n01) && valid_pn(p10, n10) && valid_pn(p11, n11)) {
        p = avg4(p00, p01, p10, p11);
        n = avg4(n00, n01, n10, n11);
    }
    row_ptr(pd, pdstep, y)[x] = p;
    row_ptr(nd, ndstep, y)[x] = n;
}

// ---- ICP ------------------------------------------------------------------------------------------------------------------------
struct IcpLevel {
    const void* curr;  // float4 points or uint16 depth
    const float4* ncurr;
    const void* prev;
    const float4* nprev;
    int curr_step, ncurr_step, prev_step, nprev_step;
    int rows, cols;
    Reproj rp;  // the level's intrinsics
};

// correspondence code of pixel (x, y); on 0, s, d and nd of the pair
template <bool DEPTH>
SOBFU_DEV int correspond(const IcpLevel& L, const float* aff, int x, int y, float3& s, float3& d, float3& nd) {
    const float4 nc = row_ptr(L.ncurr, L.ncurr_step, y)[x];
    float3 s0;
    if (DEPTH) {
        const uint16_t z = row_ptr((const uint16_t*) L.curr, L.curr_step, y)[x];
        if (z == 0 || !valid_pn(make_float4(0.f, 0.f, 0.f, 0.f), nc)) return 40;
        s0 = L.rp((float) x, (float) y, z * 0.001f);
    } else {
        const float4 p = row_ptr((const float4*) L.curr, L.curr_step, y)[x];
        if (!valid_pn(p, nc)) return 40;
        s0 = make_float3(p.x, p.y, p.z);
    }
    s = make_float3(aff[0] * s0.x + aff[1] * s0.y + aff[2] * s0.z + aff[3], aff[4] * s0.x + aff[5] * s0.y + aff[6] * s0.z + aff[7],
                    aff[8] * s0.x + aff[9] * s0.y + aff[10] * s0.z + aff[11]);
    const float u = L.rp.fx * (s.x / s.z) + L.rp.cx, v = L.rp.fy * (s.y / s.z) + L.rp.cy;
    if (s.z <= 0.f || u < 0.f || v < 0.f || u >= (float) L.cols || v >= (float) L.rows) return 80;
    const int ui = (int) floorf(u + 0.5f), vi = (int) floorf(v + 0.5f);
    if (ui >= L.cols || vi >= L.rows) return 80;
    const float4 n4 = row_ptr(L.nprev, L.nprev_step, vi)[ui];
    if (DEPTH) {
        const uint16_t z = row_ptr((const uint16_t*) L.prev, L.prev_step, vi)[ui];
        if (z == 0 || !valid_pn(make_float4(0.f, 0.f, 0.f, 0.f), n4)) return 120;
        d = L.rp(u, v, z * 0.001f);
    } else {
        const float4 p = row_ptr((const float4*) L.prev, L.prev_step, vi)[ui];
        if (!valid_pn(p, n4)) return 120;
        d = make_float3(p.x, p.y, p.z);
    }
    nd = make_float3(n4.x, n4.y, n4.z);
    return 0;
}

template <bool DEPTH>
__global__ void __launch_bounds__(kThreads) icp_correspond_kernel(IcpLevel L, const float* __restrict__ d_aff, const int* __restrict__ status,
                                                                  float dist2, float min_cos, float* __restrict__ parts, uint8_t* __restrict__ codes,
                                                                  int codes_step) {
    __shared__ float lds[4][kSums];
    if (status && *status != 0) return;  // uniform: the whole grid exits before any barrier
    float aff[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) aff[k] = d_aff[k];
    float acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.f;
    const int npix = L.rows * L.cols;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < npix; p += gridDim.x * kThreads) {
        const int y = p / L.cols, x = p - y * L.cols;
        float3 s, d, nd;
        int code = correspond<DEPTH>(L, aff, x, y, s, d, nd);
        if (code == 0) {
            const float dx = s.x - d.x, dy = s.y - d.y, dz = s.z - d.z;
            if (dx * dx + dy * dy + dz * dz > dist2) {
                code = 160;
            } else {
                const float4 nc = row_ptr(L.ncurr, L.ncurr_step, y)[x];
                const float nsx = aff[0] * nc.x + aff[1] * nc.y + aff[2] * nc.z, nsy = aff[4] * nc.x + aff[5] * nc.y + aff[6] * nc.z,
                            nsz = aff[8] * nc.x + aff[9] * nc.y + aff[10] * nc.z;
                if (fabsf(nsx * nd.x + nsy * nd.y + nsz * nd.z) < min_cos) code = 200;
            }
        }
        if (codes) row_ptr(codes, codes_step, y)[x] = (uint8_t) code;
        if (code == 0) {
            const float r = nd.x * (d.x - s.x) + nd.y * (d.y - s.y) + nd.z * (d.z - s.z);
            const float row[6] = {s.y * nd.z - s.z * nd.y, s.z * nd.x - s.x * nd.z, s.x * nd.y - s.y * nd.x, nd.x, nd.y, nd.z};
            add_row(acc, row, r);
        }
    }
    block_sum<float, kSums>(acc, lds);
    if (threadIdx.x == 0) {
        float* o = parts + (size_t) blockIdx.x * kSlab;
#pragma unroll
        for (int k = 0; k < kSums; ++k) o[k] = acc[k];
    }
}

__global__ void __launch_bounds__(kThreads) icp_init_kernel(float* __restrict__ pose, int* __restrict__ status) {
    if (threadIdx.x < 16) pose[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.f : 0.f;
    if (threadIdx.x == 0) *status = 0;
}

// Solve of one iteration (or, with sums_out, the fp64 sums alone: sobfu_hip_icp_step)
__global__ void __launch_bounds__(kThreads) icp_solve_kernel(const float* __restrict__ parts, int nparts, float* __restrict__ pose, int* __restrict__ status,
                                                             int tag, float* __restrict__ trace, double* __restrict__ sums_out) {
    __shared__ double lds[4][kSums];
    if (status && *status != 0) return;
    double acc[kSums];
    const int j = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = j < nparts ? (double) parts[(size_t) j * kSlab + k] : 0.0;
    block_sum<double, kSums>(acc, lds);
    if (threadIdx.x != 0) return;
    if (sums_out) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums_out[k] = acc[k];
        return;
    }
    if (trace) {
        trace[0] = (float) acc[27];
        trace[1] = acc[27] > 0.0 ? (float) sqrt(acc[28] / acc[27]) : 0.f;
    }
    double A[6][6], b[6];
    unpack_sums(acc, A, b);
    Ldlt<6> f;
    ldlt_factor<6>(A, f);
    if (!(fabs(f.det) >= 1e-15) || !f.positive) {
        *status = tag;
        return;
    }
    double x[6];
    ldlt_solve<6>(f, b, x);
    // Tinc = (Rodrigues(x0..2), x3..5)
    const double w[3] = {x[0], x[1], x[2]}, t[3] = {x[3], x[4], x[5]};
    apply_increment(w, t, pose);
}

Reproj level_reproj(float fx, float fy, float cx, float cy, int level) {
    const float div = (float) (1 << level);
    Reproj r{fx / div, fy / div, cx / div, cy / div, 0.f, 0.f};
    r.fxinv = 1.f / r.fx;
    r.fyinv = 1.f / r.fy;
    return r;
}
int parts_of(int rows, int cols) {
    const int n = (int) (((long long) rows * cols + 4 * kThreads - 1) / (4 * kThreads));  // at least 4 pixels per lane
    return n < 1 ? 1 : n > kMaxParts ? kMaxParts : n;
}
bool level_ok(const sobfu_hip_icp_level& l, int depth_mode) {
    const int pix = depth_mode ? 2 : 16;
    if (!(l.curr && l.ncurr && l.prev && l.nprev && l.rows >= 1 && l.cols >= 1)) return false;
    if (!((long long) l.rows * l.cols < (1LL << 30))) return false;
    if ((long long) l.curr_step < (long long) l.cols * pix || (long long) l.prev_step < (long long) l.cols * pix) return false;
    if (!aligned(l.ncurr, l.ncurr_step, 16) || !aligned(l.nprev, l.nprev_step, 16) || l.ncurr_step < l.cols * 16 || l.nprev_step < l.cols * 16) return false;
    return aligned(l.curr, l.curr_step, pix) && aligned(l.prev, l.prev_step, pix);
}
IcpLevel make_level(const sobfu_hip_icp_level& l, const Reproj& rp) {
    return IcpLevel{l.curr, (const float4*) l.ncurr, l.prev, (const float4*) l.nprev, l.curr_step, l.ncurr_step, l.prev_step, l.nprev_step, l.rows, l.cols, rp};
}
void launch_correspond(const IcpLevel& L, int depth_mode, const float* aff, const int* status, float dist2, float min_cos, float* parts, uint8_t* codes,
                       int codes_step, hipStream_t s) {
    const dim3 grid((unsigned) parts_of(L.rows, L.cols));
    if (depth_mode) hipLaunchKernelGGL(icp_correspond_kernel<true>, grid, dim3(kThreads), 0, s, L, aff, status, dist2, min_cos, parts, codes, codes_step);
    else hipLaunchKernelGGL(icp_correspond_kernel<false>, grid, dim3(kThreads), 0, s, L, aff, status, dist2, min_cos, parts, codes, codes_step);
}
bool thresholds_ok(float dist, float angle) { return positive_finite(dist) && std::isfinite(angle) && angle >= 0.f; }

constexpr size_t kWorkspaceBytes = (size_t) kMaxParts * kSlab * sizeof(float);

}  // namespace

extern "C" {

int sobfu_hip_depth_pyramid(const uint16_t* d_src, int src_step, int rows, int cols, uint16_t* d_dst, int dst_step, float sigma_depth, void* stream) {
    SOBFU_CHECK_ARGS(d_src && d_dst && rows >= 2 && cols >= 2 && std::isfinite(sigma_depth));
    SOBFU_CHECK_ARGS(src_step >= cols * 2 && dst_step >= (cols / 2) * 2 && aligned(d_src, src_step, 2) && aligned(d_dst, dst_step, 2));
    const int drows = rows / 2, dcols = cols / 2;
    const float thr = sigma_depth * 1000.f * 3.f;
    hipLaunchKernelGGL(pyramid_kernel, image_grid(drows, dcols), dim3(64, 4), 0, (hipStream_t) stream, d_src, src_step, rows, cols, d_dst, dst_step,
                       drows, dcols, thr);
    return (int) hipGetLastError();
}

int sobfu_hip_compute_point_normals(const uint16_t* d_depth, int depth_step, int rows, int cols, float fx, float fy, float cx, float cy, float* d_points,
                                    int points_step, float* d_normals, int normals_step, void* stream) {
    SOBFU_CHECK_ARGS(d_depth && d_points && d_normals && rows >= 1 && cols >= 1 && intr_ok(fx, fy, cx, cy));
    SOBFU_CHECK_ARGS(depth_step >= cols * 2 && points_step >= cols * 16 && normals_step >= cols * 16 && aligned(d_depth, depth_step, 2));
    SOBFU_CHECK_ARGS(aligned(d_points, points_step, 16) && aligned(d_normals, normals_step, 16));
    hipLaunchKernelGGL(point_normals_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, d_depth, depth_step, rows, cols,
                       level_reproj(fx, fy, cx, cy, 0), (float4*) d_points, points_step, (float4*) d_normals, normals_step);
    return (int) hipGetLastError();
}

int sobfu_hip_compute_normals_mask_depth(uint16_t* d_depth, int depth_step, int rows, int cols, float fx, float fy, float cx, float cy, float* d_normals,
                                         int normals_step, void* stream) {
    SOBFU_CHECK_ARGS(d_depth && d_normals && rows >= 1 && cols >= 1 && intr_ok(fx, fy, cx, cy));
    SOBFU_CHECK_ARGS(depth_step >= cols * 2 && normals_step >= cols * 16 && aligned(d_depth, depth_step, 2) && aligned(d_normals, normals_step, 16));
    hipLaunchKernelGGL(normals_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, d_depth, depth_step, rows, cols,
                       level_reproj(fx, fy, cx, cy, 0), (float4*) d_normals, normals_step);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mask_depth_kernel, image_grid(rows, cols), dim3(64, 4), 0, (hipStream_t) stream, (const float4*) d_normals, normals_step, d_depth,
                       depth_step, rows, cols);
    return (int) hipGetLastError();
}

int sobfu_hip_resize_depth_normals(const uint16_t* d_depth, int depth_step, const float* d_normals, int normals_step, int rows, int cols,
                                   uint16_t* d_depth_out, int depth_out_step, float* d_normals_out, int normals_out_step, void* stream) {
    SOBFU_CHECK_ARGS(d_depth && d_normals && d_depth_out && d_normals_out && rows >= 2 && cols >= 2);
    const int drows = rows / 2, dcols = cols / 2;
    SOBFU_CHECK_ARGS(depth_step >= cols * 2 && normals_step >= cols * 16 && depth_out_step >= dcols * 2 && normals_out_step >= dcols * 16);
    SOBFU_CHECK_ARGS(aligned(d_depth, depth_step, 2) && aligned(d_depth_out, depth_out_step, 2) && aligned(d_normals, normals_step, 16) &&
                     aligned(d_normals_out, normals_out_step, 16));
    hipLaunchKernelGGL(resize_depth_normals_kernel, image_grid(drows, dcols), dim3(64, 4), 0, (hipStream_t) stream, d_depth, depth_step,
                       (const float4*) d_normals, normals_step, d_depth_out, depth_out_step, (float4*) d_normals_out, normals_out_step, drows, dcols);
    return (int) hipGetLastError();
}

int sobfu_hip_resize_points_normals(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols,
                                    float* d_points_out, int points_out_step, float* d_normals_out, int normals_out_step, void* stream) {
    SOBFU_CHECK_ARGS(d_points && d_normals && d_points_out && d_normals_out && rows >= 2 && cols >= 2);
    const int drows = rows / 2, dcols = cols / 2;
    SOBFU_CHECK_ARGS(points_step >= cols * 16 && normals_step >= cols * 16 && points_out_step >= dcols * 16 && normals_out_step >= dcols * 16);
    SOBFU_CHECK_ARGS(aligned(d_points, points_step, 16) && aligned(d_points_out, points_out_step, 16) && aligned(d_normals, normals_step, 16) &&
                     aligned(d_normals_out, normals_out_step, 16));
    hipLaunchKernelGGL(resize_points_normals_kernel, image_grid(drows, dcols), dim3(64, 4), 0, (hipStream_t) stream, (const float4*) d_points,
                       points_step, (const float4*) d_normals, normals_step, (float4*) d_points_out, points_out_step, (float4*) d_normals_out,
                       normals_out_step, drows, dcols);
    return (int) hipGetLastError();
}

size_t sobfu_hip_icp_workspace_bytes(void) { return kWorkspaceBytes; }

int sobfu_hip_icp_step(const sobfu_hip_icp_level* level, int level_index, int depth_mode, float fx, float fy, float cx, float cy, float dist_thres,
                       float angle_thres, const float* d_aff, void* d_workspace, size_t workspace_bytes, double* d_sums, uint8_t* d_codes,
                       int codes_step, void* stream) {
    SOBFU_CHECK_ARGS(level && d_aff && d_workspace && d_sums && workspace_bytes >= kWorkspaceBytes);
    SOBFU_CHECK_ARGS(level_index >= 0 && level_index < 4 && (depth_mode == 0 || depth_mode == 1) && intr_ok(fx, fy, cx, cy));
    SOBFU_CHECK_ARGS(thresholds_ok(dist_thres, angle_thres) && level_ok(*level, depth_mode));
    SOBFU_CHECK_ARGS(!d_codes || codes_step >= level->cols);
    const IcpLevel L = make_level(*level, level_reproj(fx, fy, cx, cy, level_index));
    float* parts = (float*) d_workspace;
    launch_correspond(L, depth_mode, d_aff, nullptr, dist_thres * dist_thres, (float) std::cos((double) angle_thres), parts, d_codes, codes_step,
                      (hipStream_t) stream);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t) stream, parts, parts_of(L.rows, L.cols), nullptr, nullptr, 0, nullptr,
                       d_sums);
    return (int) hipGetLastError();
}

int sobfu_hip_icp_estimate(const sobfu_hip_icp_level* levels, int n_levels, const int iters[4], int depth_mode, float fx, float fy, float cx, float cy,
                           float dist_thres, float angle_thres, void* d_workspace, size_t workspace_bytes, float* d_pose, int* d_status, float* d_trace,
                           void* stream) {
    SOBFU_CHECK_ARGS(levels && iters && d_workspace && d_pose && d_status && workspace_bytes >= kWorkspaceBytes);
    SOBFU_CHECK_ARGS(n_levels >= 1 && n_levels <= 4 && (depth_mode == 0 || depth_mode == 1) && intr_ok(fx, fy, cx, cy));
    SOBFU_CHECK_ARGS(thresholds_ok(dist_thres, angle_thres));
    for (int l = 0; l < n_levels; ++l) SOBFU_CHECK_ARGS(iters[l] >= 0 && iters[l] <= 1000 && level_ok(levels[l], depth_mode));
    const hipStream_t s = (hipStream_t) stream;
    const float dist2 = dist_thres * dist_thres, min_cos = (float) std::cos((double) angle_thres);
    float* parts = (float*) d_workspace;
    hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(kThreads), 0, s, d_pose, d_status);
    SOBFU_HIP_TRY(hipGetLastError());
    int it_global = 0;
    for (int l = n_levels - 1; l >= 0; --l) {  // coarse to fine (projective_icp.cpp)
        const IcpLevel L = make_level(levels[l], level_reproj(fx, fy, cx, cy, l));
        for (int it = 0; it < iters[l]; ++it, ++it_global) {
            launch_correspond(L, depth_mode, d_pose, d_status, dist2, min_cos, parts, nullptr, 0, s);
            SOBFU_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(kThreads), 0, s, parts, parts_of(L.rows, L.cols), d_pose, d_status,
                               0x10000 | (l << 8) | it, d_trace ? d_trace + 2 * it_global : nullptr, nullptr);
            SOBFU_HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

}  // extern "C"
