// Area-weighted samples of an indexed triangle mesh on gfx950, and the counts behind precision, recall and F-score.  The
// reference has no such step; the rule is this project's (sobfu_mesh_sample.hpp, restated by tests/mesh_sample_reference.py): the samples
// depend on the mesh, the density and the seed alone -- not on the launch shape, the workgroup size or the run.
//
//   count     one lane per triangle: its fp64 area, its count (floor(area density) plus one Philox coin for the fraction), stored clamped
//             to INT32_MAX; the 64-bit total by one integer atomic per workgroup; a face index outside [0, n_vertices) or a non-finite corner
//             counts 0 and raises the header's flag
//   scan      scan_exclusive (sobfu_scan.hpp) over n_triangles + 1 counts, the last one 0: offset[n_triangles] = the total
//   generate  one lane per SAMPLE, so that a 12-triangle box spreads its samples over the whole chip: an upper-bound binary search of
//             the lane's index in offset[0 .. n_triangles] (runs of equal offsets -- triangles without samples -- are stepped over), then
//             the point of (triangle, k).  The plain per-lane search in global memory is the one kept: profiles/mesh_sample.md
//   score     n distances against K <= 16 thresholds: per lane counts over a grid-stride loop, summed across the wave, then across the
//             workgroup's waves through LDS, one 64-bit integer atomic per threshold and workgroup.  NaN and +Inf are never within
// workspace (ints): a header of 16 | count[T + 1] | offset[T + 1] | the scan's block sums.
#include "sobfu_hip.h"
#include "sobfu_mesh.hpp"
#include "sobfu_mesh_sample.hpp"
#include "sobfu_scan.hpp"

using namespace sobfu_hip;

namespace {

// header (ints): 0 bad-input flag, 1 a triangle alone exceeds INT32_MAX, 2-3 the total (64 bit), 5 counted marker, 6 the triangles counted
constexpr int kSmpBad = 0, kSmpHuge = 1, kSmpTotal = 2, kSmpCounted = 5, kSmpTriangles = 6;
constexpr int kMaxThresholds = 16;

struct SampleWs {
    int* hdr;
    int* count;   // T + 1, the last one 0
    int* offset;  // T + 1: the exclusive scan; offset[T] = the total
    int* blk;
};
size_t sample_ints(int n_triangles) {
    const size_t nc = (size_t) n_triangles + 1, nb = (nc + kChunk - 1) / kChunk;
    return kHdrInts + 2 * nc + nb + 1;
}
SampleWs sample_ws(void* ws, int n_triangles) {
    const size_t nc = (size_t) n_triangles + 1;
    SampleWs w;
    w.hdr = (int*) ws, w.count = w.hdr + kHdrInts, w.offset = w.count + nc, w.blk = w.offset + nc;
    return w;
}

SOBFU_DEV bool face_ok(const int3& f, int n_vertices) {
    return f.x >= 0 && f.x < n_vertices && f.y >= 0 && f.y < n_vertices && f.z >= 0 && f.z < n_vertices;
}

__global__ void __launch_bounds__(256) sample_count_kernel(SampleWs w, const float4* __restrict__ verts, int n_vertices, const int* __restrict__ faces,
                                                           int n_triangles, double density, uint64_t seed, double* __restrict__ areas) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    unsigned long long mine = 0;
    if (t < n_triangles) {
        const Mesh m{verts, faces, n_triangles};
        const int3 f = face_of(m, t);
        bool ok      = face_ok(f, n_vertices);
        double area  = 0.0;
        if (ok) {
            const Corners c = corners_of(m, f);
            ok              = finite3(c.a) && finite3(c.b) && finite3(c.c);
            if (ok) {
                area = triangle_area(p3(c.a), p3(c.b), p3(c.c));
                mine = (unsigned long long) sample_count(area, density, seed, t);
            }
        }
        if (!ok) atomicOr(w.hdr + kSmpBad, 1);
        if (mine > (unsigned long long) INT_MAX) atomicOr(w.hdr + kSmpHuge, 1);
        w.count[t] = (int) (mine > (unsigned long long) INT_MAX ? (unsigned long long) INT_MAX : mine);
        if (areas) areas[t] = area;
    }
    // the total: a wave sum, the four wave sums through LDS, one atomic per workgroup (thousands of atomics on one address serialise:
    // one per wave cost 30 us on 175 632 triangles, profiles/mesh_sample.md)
    __shared__ unsigned long long s_wave[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (sum) atomicAdd((unsigned long long*) (w.hdr + kSmpTotal), sum);
    }
}

struct Generate {
    const float4* verts;
    int n_vertices;
    const int* faces;
    int n_triangles;
    uint64_t seed;
    const int* offset;  // n_triangles + 1
    int total;
    float4* points;
    int* tri;      // may be null
    float2* bary;  // may be null
};

__global__ void __launch_bounds__(256) sample_generate_kernel(Generate g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.total) return;
    // the first index in [0, T] whose offset exceeds i: offset[T] = total > i, so it exists, and offset[0] = 0 <= i, so it is >= 1
    int lo = 0, hi = g.n_triangles;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (g.offset[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    const int t = lo - 1, k = i - g.offset[t];
    const Mesh m{g.verts, g.faces, g.n_triangles};
    const int3 f = face_of(m, t);
    MeshSample s{P3{0.f, 0.f, 0.f}, 0.f, 0.f};
    if (face_ok(f, g.n_vertices)) {  // always, with the arrays the count call saw: a triangle that fails this has no samples
        const Corners c = corners_of(m, f);
        s               = sample_point(p3(c.a), p3(c.b), p3(c.c), g.seed, t, k);
    }
    g.points[i] = make_float4(s.p.x, s.p.y, s.p.z, 1.f);
    if (g.tri) g.tri[i] = t;
    if (g.bary) g.bary[i] = make_float2(s.r1, s.r2);
}

struct Thresholds {
    float tau[kMaxThresholds];
    int k;
};

// counts[0 .. k - 1]: d finite and d <= tau; counts[k]: d finite
__global__ void __launch_bounds__(256) distance_score_kernel(const float* __restrict__ dist, int n, Thresholds th, unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_part[4][kMaxThresholds + 1];
    unsigned mine[kMaxThresholds + 1];
#pragma unroll
    for (int k = 0; k <= kMaxThresholds; ++k) mine[k] = 0;
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < (size_t) n; i += (size_t) gridDim.x * 256) {
        const float d     = dist[i];
        const bool finite = fabsf(d) < INFINITY;
#pragma unroll
        for (int k = 0; k < kMaxThresholds; ++k) mine[k] += (k < th.k && finite && d <= th.tau[k]) ? 1u : 0u;
        mine[kMaxThresholds] += finite ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= kMaxThresholds; ++k) {
        unsigned v = mine[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < th.k || k == kMaxThresholds) {
        const unsigned long long sum = (unsigned long long) s_part[0][k] + s_part[1][k] + s_part[2][k] + s_part[3][k];
        if (sum) atomicAdd(counts + (k == kMaxThresholds ? th.k : k), sum);
    }
}

bool mesh_args_ok(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles) {
    return n_vertices >= 0 && n_triangles >= 0 && (n_triangles == 0 || (d_vertices && d_faces)) && aligned(d_vertices, 0, 16) && aligned(d_faces, 0, 4);
}

}  // namespace

extern "C" {

size_t sobfu_hip_mesh_sample_workspace_bytes(int n_triangles) { return n_triangles < 0 ? 0 : sample_ints(n_triangles) * sizeof(int); }

int sobfu_hip_mesh_sample_count(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, double density, uint64_t seed,
                                void* d_workspace, size_t workspace_bytes, double* d_areas, long long* h_samples, void* stream) {
    SOBFU_CHECK_ARGS(h_samples && mesh_args_ok(d_vertices, n_vertices, d_faces, n_triangles) && std::isfinite(density) && density >= 0.0);
    SOBFU_CHECK_ARGS(d_workspace && aligned(d_workspace, 0, 16) && workspace_bytes >= sample_ints(n_triangles) * sizeof(int) && aligned(d_areas, 0, 8));
    hipStream_t st   = (hipStream_t) stream;
    const SampleWs w = sample_ws(d_workspace, n_triangles);
    const int nc     = n_triangles + 1;
    *h_samples       = 0;
    SOBFU_HIP_TRY(hipMemsetAsync(w.hdr, 0, (size_t) (kHdrInts + nc) * sizeof(int), st));  // the header and the counts, the last one included
    if (n_triangles > 0) {
        const dim3 blocks((unsigned) (((long long) n_triangles + 255) / 256));
        hipLaunchKernelGGL(sample_count_kernel, blocks, dim3(256), 0, st, w, (const float4*) d_vertices, n_vertices, d_faces, n_triangles, density, seed,
                           d_areas);
        SOBFU_HIP_TRY(hipGetLastError());
    }
    int hdr[4];
    SOBFU_HIP_TRY(hipMemcpyAsync(hdr, w.hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    if (hdr[kSmpBad]) return SOBFU_E_BADARG;
    unsigned long long total;
    std::memcpy(&total, hdr + kSmpTotal, sizeof total);
    *h_samples = (long long) (total > (unsigned long long) LLONG_MAX ? (unsigned long long) LLONG_MAX : total);
    if (hdr[kSmpHuge] || total > (unsigned long long) INT_MAX) return SOBFU_E_UNSUPPORTED;  // int offsets: nothing is scanned, generate is refused
    SOBFU_TRY(scan_exclusive(w.count, nc, w.offset, w.blk, st));
    SOBFU_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) (w.hdr + kSmpTriangles), n_triangles, 1, st));
    return (int) hipMemsetD32Async((hipDeviceptr_t) (w.hdr + kSmpCounted), 1, 1, st);
}

int sobfu_hip_mesh_sample_generate(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, uint64_t seed, void* d_workspace,
                                   size_t workspace_bytes, float* d_points, int* d_tri, float* d_bary, int max_samples, void* stream) {
    SOBFU_CHECK_ARGS(mesh_args_ok(d_vertices, n_vertices, d_faces, n_triangles) && max_samples >= 0 && (max_samples == 0 || d_points));
    SOBFU_CHECK_ARGS(d_workspace && aligned(d_workspace, 0, 16) && workspace_bytes >= sample_ints(n_triangles) * sizeof(int));
    SOBFU_CHECK_ARGS(aligned(d_points, 0, 16) && aligned(d_tri, 0, 4) && aligned(d_bary, 0, 8));
    hipStream_t st   = (hipStream_t) stream;
    const SampleWs w = sample_ws(d_workspace, n_triangles);
    int hdr[8];  // the count call's verdict and total: never truncate
    SOBFU_HIP_TRY(hipMemcpyAsync(hdr, w.hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    unsigned long long total;
    std::memcpy(&total, hdr + kSmpTotal, sizeof total);
    SOBFU_CHECK_ARGS(hdr[kSmpCounted] == 1 && hdr[kSmpTriangles] == n_triangles && !hdr[kSmpBad] && !hdr[kSmpHuge] && total <= (unsigned long long) max_samples);
    if (total == 0) return 0;
    SOBFU_CHECK_ARGS(d_points);
    const Generate g{(const float4*) d_vertices, n_vertices, d_faces, n_triangles, seed, w.offset, (int) total, (float4*) d_points, d_tri, (float2*) d_bary};
    hipLaunchKernelGGL(sample_generate_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, g);
    return (int) hipGetLastError();
}

int sobfu_hip_distance_score(const float* d_dist, int n, const float* h_thresholds, int n_thresholds, long long* d_counts, void* stream) {
    SOBFU_CHECK_ARGS(n >= 0 && (n == 0 || d_dist) && aligned(d_dist, 0, 4) && h_thresholds && n_thresholds >= 1 && n_thresholds <= kMaxThresholds &&
                     d_counts && aligned(d_counts, 0, 8));
    hipStream_t st = (hipStream_t) stream;
    Thresholds th;
    for (int k = 0; k < kMaxThresholds; ++k) th.tau[k] = k < n_thresholds ? h_thresholds[k] : 0.f;
    th.k = n_thresholds;
    SOBFU_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t) (n_thresholds + 1) * sizeof(long long), st));
    if (n == 0) return 0;
    const long long blocks = ((long long) n + 255) / 256;
    hipLaunchKernelGGL(distance_score_kernel, dim3((unsigned) (blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, d_dist, n, th,
                       (unsigned long long*) d_counts);
    return (int) hipGetLastError();
}

}  // extern "C"
