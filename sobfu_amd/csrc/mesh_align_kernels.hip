// Rigid alignment of a point list to an indexed triangle mesh on gfx950: point-to-plane ICP whose correspondences are the exact nearest
// triangles of mesh_distance_kernels.hip, the whole loop enqueued on one stream with no host synchronisation.  The
// reference has no such step; the rules are this project's, and tests/mesh_align_reference.py restates them in the same operation order
// (every TU is built with -ffp-contract=off; there is no fused operation and no fast division in this file).  The 6 x 6 solve, Rodrigues,
// the pose composition and the rigid inverse are sobfu_rigid.hpp's; the sums of a row, the workgroup reduction, the unpacking into A x = b,
// the pose update and the launch constants sobfu_normal_eq.hpp's, shared with icp_kernels.hip; the target and its check sobfu_mesh.hpp's.
//
//   pose         16 floats in device memory, row-major 4 x 4, mapping the source (the points) to the target (the mesh) frame; rows 0..2 are
//                read and written, row 3 is the caller's
//   transform    s = ((r0 x + r1 y) + r2 z) + t per row in fp32 -- the convention of transform_points and SobFusion.evaluate -- written as
//                the dense float4 list s with w = 1
//   correspond   sobfu_hip_mesh_distance on s with the caller's max_dist, mode and ring_cap -> (dist, tri, c); that code is unchanged
//   inlier       the source point is finite in x, y, z; tri >= 0; the triangle's normal has positive length.  The normal, in fp64 from the
//                fp32 corners a, b, c2: m = (b - a) x (c2 - a), len = sqrt((m.x m.x + m.y m.y) + m.z m.z), n = m / len per component.  A
//                zero-area triangle (len == 0) makes its points outliers.
//   row (fp64)   J = [s x n, n] = (s.y n.z - s.z n.y, s.z n.x - s.x n.z, s.x n.y - s.y n.x, n.x, n.y, n.z) and
//                r = (n.x (c.x - s.x) + n.y (c.y - s.y)) + n.z (c.z - s.z), s and c converted from float
//   sums         29 values, laid out as in ICP: the 21 upper-triangular products J_i J_j (i <= j < 6, row-major), the 6 products J_i r, 1
//                (the inlier count) and r r.  Per lane in fp64 over a grid-stride loop (at most 256 workgroups of 256), then a wave64
//                butterfly, then LDS across the four waves (wave 0 + 1 + 2 + 3, in that order), then one 32-double slab per workgroup.
//                No floating-point atomics anywhere: the sums, and so the pose, are bitwise reproducible run to run.
//   solve        one workgroup: lane k < 29 adds value k of the slabs in slab order; lane 0 solves A x = b by LDL^T with compile-time
//                indices (nothing goes to scratch).  Failure: a pivot D_j <= 0 or non-finite.  (ICP's absolute |det| < 1e-15 test is
//                the reference's, for that problem's scaling; it is not taken over.)
//   dof          6: rigid, x = (w, t_inc).  3: translation only -- the lower-right 3 x 3 block, w = 0 (symmetric objects: a sphere's
//                rotation is unobservable).
//   update       Tinc = (Rodrigues(w), t_inc); pose = Tinc pose in fp64, rounded to float
//   stop         after the update: |w| < eps_rot and |t_inc| < eps_trans -> status = 0x20000 | iterations done (an eps of 0 never
//                triggers).  Failure: status = 0x10000 | iteration, the pose of the iteration before stays.  Status 0: every iteration ran.
//                Every later launch of THIS file sees status != 0 and exits at once; the mesh-distance launches in between still run,
//                on the stale list s: harmless (their output is not read again), and that file stays as it is.
//   trace        optional, 4 floats per iteration: inliers, sqrt(sum r r / inliers) (0 without inliers), |w|, |t_inc| (both 0 on the failed
//                iteration).  Entries of iterations that did not run are not written.
#include "sobfu_hip.h"
#include "sobfu_mesh.hpp"
#include "sobfu_normal_eq.hpp"

using namespace sobfu_hip;

namespace {

constexpr int kMaxIters = 1000;

__global__ void __launch_bounds__(kThreads) align_transform_kernel(const float* __restrict__ pose, const int* __restrict__ status,
                                                                   const float4* __restrict__ src, int n, float4* __restrict__ s) {
    if (status && *status != 0) return;
    float P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = pose[k];
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float4 p = src[i];
        s[i] = make_float4(((P[0] * p.x + P[1] * p.y) + P[2] * p.z) + P[3], ((P[4] * p.x + P[5] * p.y) + P[6] * p.z) + P[7],
                           ((P[8] * p.x + P[9] * p.y) + P[10] * p.z) + P[11], 1.f);
    }
}

__global__ void __launch_bounds__(kThreads) align_sums_kernel(const int* __restrict__ status, const float4* __restrict__ src,
                                                              const float4* __restrict__ s4, const int* __restrict__ tri,
                                                              const float4* __restrict__ closest, const float4* __restrict__ verts,
                                                              const int* __restrict__ faces, int n_triangles, int n, double* __restrict__ parts) {
    __shared__ double lds[4][kSums];
    if (status && *status != 0) return;  // uniform: the whole grid exits before any barrier
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const float4 p = src[i];
        const int t = tri[i];
        if (!finite3(p) || t < 0 || t >= n_triangles) continue;
        const auto [a, b, c2] = corners_of(Mesh{verts, faces, n_triangles}, t);
        const double ux = (double) b.x - (double) a.x, uy = (double) b.y - (double) a.y, uz = (double) b.z - (double) a.z;
        const double vx = (double) c2.x - (double) a.x, vy = (double) c2.y - (double) a.y, vz = (double) c2.z - (double) a.z;
        const double mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
        const double len = sqrt((mx * mx + my * my) + mz * mz);
        if (!(len > 0.0)) continue;
        const double nx = mx / len, ny = my / len, nz = mz / len;
        const float4 sf = s4[i], cf = closest[i];
        const double sx = sf.x, sy = sf.y, sz = sf.z;
        const double r = (nx * ((double) cf.x - sx) + ny * ((double) cf.y - sy)) + nz * ((double) cf.z - sz);
        const double row[6] = {sy * nz - sz * ny, sz * nx - sx * nz, sx * ny - sy * nx, nx, ny, nz};
        add_row(acc, row, r);
    }
    block_sum<double, kSums>(acc, lds);
    if (threadIdx.x == 0) {
        double* o = parts + (size_t) blockIdx.x * kSlab;
#pragma unroll
        for (int k = 0; k < kSums; ++k) o[k] = acc[k];
    }
}

// The solve of iteration `it` (or, with sums_out, the sums alone: sobfu_hip_mesh_align_step).  nparts = 0: no points, no inliers.
__global__ void __launch_bounds__(64) align_solve_kernel(const double* __restrict__ parts, int nparts, float* __restrict__ pose,
                                                         int* __restrict__ status, int it, int dof, float eps_rot, float eps_trans,
                                                         float* __restrict__ trace, double* __restrict__ sums_out) {
    __shared__ double total[kSlab];
    if (status && *status != 0) return;
    if (threadIdx.x < kSums) {
        double v = 0.0;
        for (int j = 0; j < nparts; ++j) v += parts[(size_t) j * kSlab + threadIdx.x];
        total[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = total[k];
    if (sums_out) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums_out[k] = acc[k];
        return;
    }
    if (trace) {
        trace[0] = (float) acc[27];
        trace[1] = acc[27] > 0.0 ? (float) sqrt(acc[28] / acc[27]) : 0.f;
        trace[2] = 0.f;
        trace[3] = 0.f;
    }
    double w[3] = {0.0, 0.0, 0.0}, tinc[3];
    bool ok;
    if (dof == 6) {
        double A[6][6], b[6], x[6];
        unpack_sums(acc, A, b);
        Ldlt<6> f;
        ldlt_factor<6>(A, f);
        ok = ldlt_ok(f);
        ldlt_solve<6>(f, b, x);
        w[0] = x[0], w[1] = x[1], w[2] = x[2], tinc[0] = x[3], tinc[1] = x[4], tinc[2] = x[5];
    } else {  // the translation block: sums 15 16 17 / 18 19 / 20 and b 24 25 26
        double A[3][3] = {{acc[15], acc[16], acc[17]}, {acc[16], acc[18], acc[19]}, {acc[17], acc[19], acc[20]}};
        double b[3] = {acc[24], acc[25], acc[26]};
        Ldlt<3> f;
        ldlt_factor<3>(A, f);
        ok = ldlt_ok(f);
        ldlt_solve<3>(f, b, tinc);
    }
    if (!ok) {
        *status = 0x10000 | it;
        return;
    }
    const double tn = sqrt((tinc[0] * tinc[0] + tinc[1] * tinc[1]) + tinc[2] * tinc[2]);
    const double th = apply_increment(w, tinc, pose);
    if (trace) {
        trace[2] = (float) th;
        trace[3] = (float) tn;
    }
    if (th < (double) eps_rot && tn < (double) eps_trans) *status = 0x20000 | (it + 1);
}

int parts_of(int n) {
    const int p = (int) (((long long) n + kThreads - 1) / kThreads);
    return p < 1 ? 1 : p > kMaxParts ? kMaxParts : p;
}
size_t round4(size_t n) { return (n + 3) & ~(size_t) 3; }

// the caller's workspace: slabs | s (n float4) | closest (n float4) | dist | tri | unresolved (n rounded up to 4, 4 bytes each)
struct Workspace {
    double* parts;
    float4 *s, *closest;
    float* dist;
    int *tri, *unresolved;
};
size_t workspace_bytes_of(int n) { return (size_t) kMaxParts * kSlab * sizeof(double) + 32 * (size_t) n + 12 * round4((size_t) n); }
Workspace carve(void* ws, int n) {
    Workspace w;
    char* p = (char*) ws;
    w.parts = (double*) p, p += (size_t) kMaxParts * kSlab * sizeof(double);
    w.s = (float4*) p, p += 16 * (size_t) n;
    w.closest = (float4*) p, p += 16 * (size_t) n;
    w.dist = (float*) p, p += 4 * round4((size_t) n);
    w.tri = (int*) p, p += 4 * round4((size_t) n);
    w.unresolved = (int*) p;
    return w;
}

struct Target {
    MeshTarget m;
    float max_dist;
    int mode, ring_cap;
};
int query(const Target& t, const Workspace& w, int n, hipStream_t s) {
    const Grid& g = t.m.grid;
    const float origin[3] = {g.ox, g.oy, g.oz};
    const int dims[3] = {g.dx, g.dy, g.dz};
    return sobfu_hip_mesh_distance(g.hdr, t.m.ws_bytes, (const float*) t.m.mesh.verts, t.m.n_vertices, t.m.mesh.faces, t.m.mesh.n_triangles, origin, g.h,
                                   dims, (const float*) w.s, n, t.max_dist, t.mode, t.ring_cap, w.dist, w.tri, (float*) w.closest, w.unresolved, (void*) s);
}
// every check of both entry points after mesh_target's; the query's own arguments are sobfu_hip_mesh_distance's to judge, asked with no
// points (it launches nothing then)
bool args_ok(const Target& t, const float* d_points, int n, const float* d_pose, void* ws, size_t ws_bytes) {
    if (!(d_pose && aligned(d_pose, 0, 4) && n >= 0 && ws && aligned(ws, 0, 16) && ws_bytes >= workspace_bytes_of(n))) return false;
    if (!(d_points && aligned(d_points, 0, 16))) return false;
    const Workspace w = carve(ws, n);
    return query(t, w, 0, nullptr) == 0;
}
// transform + query + sums at the pose in d_pose, into the slabs
int enqueue_pass(const Target& t, const Workspace& w, const float* d_points, int n, const float* d_pose, const int* d_status, hipStream_t s) {
    const dim3 grid((unsigned) parts_of(n));
    hipLaunchKernelGGL(align_transform_kernel, grid, dim3(kThreads), 0, s, d_pose, d_status, (const float4*) d_points, n, w.s);
    SOBFU_HIP_TRY(hipGetLastError());
    SOBFU_TRY(query(t, w, n, s));
    hipLaunchKernelGGL(align_sums_kernel, grid, dim3(kThreads), 0, s, d_status, (const float4*) d_points, (const float4*) w.s, (const int*) w.tri,
                       (const float4*) w.closest, t.m.mesh.verts, t.m.mesh.faces, t.m.mesh.n_triangles, n, w.parts);
    return (int) hipGetLastError();
}

}  // namespace

extern "C" {

size_t sobfu_hip_mesh_align_workspace_bytes(int n) { return n < 0 ? 0 : workspace_bytes_of(n); }

int sobfu_hip_mesh_align_step(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                              int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist, int mode,
                              int ring_cap, const float* d_pose, void* d_workspace, size_t workspace_bytes, double* d_sums, void* stream) {
    Target t{{}, max_dist, mode, ring_cap};
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &t.m));
    SOBFU_CHECK_ARGS(d_sums && aligned(d_sums, 0, 8) && args_ok(t, d_points, n, d_pose, d_workspace, workspace_bytes));
    if (n == 0) return 0;
    const Workspace w = carve(d_workspace, n);
    SOBFU_TRY(enqueue_pass(t, w, d_points, n, d_pose, nullptr, (hipStream_t) stream));
    hipLaunchKernelGGL(align_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t) stream, (const double*) w.parts, parts_of(n), nullptr, nullptr, 0, 6, 0.f,
                       0.f, nullptr, d_sums);
    return (int) hipGetLastError();
}

int sobfu_hip_mesh_align_estimate(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                                  int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist,
                                  int mode, int ring_cap, int iters, int dof, float eps_rot, float eps_trans, void* d_workspace, size_t workspace_bytes,
                                  float* d_pose, int* d_status, float* d_trace, void* stream) {
    Target t{{}, max_dist, mode, ring_cap};
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &t.m));
    SOBFU_CHECK_ARGS(d_status && aligned(d_status, 0, 4) && aligned(d_trace, 0, 4) && (dof == 3 || dof == 6) && iters >= 0 && iters <= kMaxIters);
    SOBFU_CHECK_ARGS(eps_rot >= 0.f && eps_trans >= 0.f && std::isfinite(eps_rot) && std::isfinite(eps_trans));
    SOBFU_CHECK_ARGS(args_ok(t, d_points, n, d_pose, d_workspace, workspace_bytes));
    if (n == 0) return 0;
    const hipStream_t s = (hipStream_t) stream;
    const Workspace w = carve(d_workspace, n);
    SOBFU_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int), s));
    for (int it = 0; it < iters; ++it) {
        SOBFU_TRY(enqueue_pass(t, w, d_points, n, d_pose, d_status, s));
        hipLaunchKernelGGL(align_solve_kernel, dim3(1), dim3(64), 0, s, (const double*) w.parts, parts_of(n), d_pose, d_status, it, dof, eps_rot,
                           eps_trans, d_trace ? d_trace + 4 * it : nullptr, nullptr);
        SOBFU_HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
