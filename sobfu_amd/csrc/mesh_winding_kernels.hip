// Generalised winding numbers of open, doubled or inconsistently oriented triangle meshes on gfx950, and the sign bits of their TSDF volumes
// (DESIGN.md 4.14).  The reference has no such step; the rule is this project's (sobfu_mesh_winding.hpp, restated by
// tests/mesh_winding_reference.py): w(p) = N(p) + the solid angles of the strips from the boundary edges to infinity along -x, over 4 pi.
// The kernels read the grid of sobfu_hip_mesh_grid_build through the walk that mesh_voxel_kernels.hip uses (sobfu_mesh_rows.hpp: the
// row's one cell column, every triangle counted in the first cell in x of its cell range); the boundary list is the caller's
// (sobfu_hip_mesh_boundary: two float4 per edge, u = (x, y, z, k) and v = (x, y, z, .)).
//
//   rows     one wave per volume row (j, k), up to X = 512: lanes stride over the column's references; each crossing adds its sign, an
//            LDS integer atomic, to the counter of the first voxel whose centre is not below X (counter X: beyond the last voxel).  Integer
//            sums are order-independent.  Nothing is decided on the counters before the barrier; then every lane sums its own nine
//            counters, the lanes' sums are scanned with shuffles, and counter i becomes the sum at counters >= i: N(voxel i) = counter i + 1.
//            A row whose total is odd is open (a sum of +-1 has the parity of their number): one integer atomic, for information.
//   strips   the boundary goes through LDS 64 edges at a time, in index order: lane e turns edge e into what it is to this row (StripRow:
//            |W|, its sign times k, the y-z parts of the lengths and of the dot product, the seam test), once per row; then every lane
//            adds, for each of its up to 8 voxels, the staged edges in order (broadcast LDS reads): only the x part, two square roots and
//            one atan2, is per voxel.  fp64, one accumulator per voxel, edge order: the same bits run after run, whatever the walk.
//   seams    a voxel whose centre lies below (in x) a boundary vertex with the row's y and z takes the definition: its index goes to a
//            compact list (an integer atomic; the order of the list changes no output), its bit stays 0, and winding_sum_kernel, launched
//            over the list without a synchronisation (the count is read on the device), sets the bit and writes w.
//   sum      the definition for a point list or the seam list: one lane per point, triangles staged through LDS 256 at a time in index
//            order, van Oosterom and Strackee in fp64.
//   points   one lane per point: the column walk of mesh_inside_kernel with signs and all boundary edges (staged through LDS 256 at a
//            time); a point on a seam is flagged with a NaN, and winding_sum_kernel, launched behind it over the same points, gives the
//            flagged ones the definition (a workgroup without one skips the triangles).  The same functions in the same order as the
//            rows: a voxel centre gets the same bits from both.
//   nothing  an unbuilt or refused grid, or no triangles: w = 0 everywhere, no bit set; the mesh and the boundary are not read.
#include <vector>

#include "sobfu_hip.h"
#include "sobfu_device.hpp"
#include "sobfu_mesh_boundary.hpp"
#include "sobfu_mesh_rows.hpp"
#include "sobfu_mesh_winding.hpp"

using namespace sobfu_hip;

namespace {

constexpr int kPerLane    = 9;               // counters a lane sums: 64 x 9 = 576 >= kMaxX + 1
constexpr int kCounters   = 64 * kPerLane;
constexpr int kVoxPerLane = kMaxX / 64;      // voxels of a row a lane accumulates
constexpr int kEdgeStage  = 64;              // boundary edges a wave stages at a time (56 B each)
constexpr int kSumBlocks  = 1024;            // workgroups of the seam pass: they stride over the list

struct RowArgs {
    Mesh mesh;
    int brute;
    Dims d;
    float vsx, vsy, vsz;
    const float4* boundary;  // 2 per edge
    int n_boundary;
    unsigned* bits;  // Y Z rows of nw words
    int nw;
    float* winding;  // X Y Z, may be NULL
    int* open_rows;
    int* seam_count;
    int* seam_list;  // voxel indices x + X (y + Y z)
};

__global__ void __launch_bounds__(256) row_winding_kernel(Grid g, RowArgs a) {
    __shared__ int cnt[4][kCounters];
    __shared__ unsigned obits[4][kMaxX / 32];
    __shared__ double e_w[4][kEdgeStage], e_qa[4][kEdgeStage], e_qb[4][kEdgeStage], e_dyz[4][kEdgeStage], e_ux[4][kEdgeStage], e_vx[4][kEdgeStage],
        e_ks[4][kEdgeStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = (long long) a.d.y * a.d.z, row_raw = (long long) blockIdx.x * 4 + wave;
    const bool valid    = row_raw < rows;
    const long long row = valid ? row_raw : rows - 1;  // a wave past the end works on the last row and writes nothing: the barriers stay uniform
    for (int i = lane; i < kCounters; i += 64) cnt[wave][i] = 0;
    if (lane < kMaxX / 32) obits[wave][lane] = 0u;
    __syncthreads();
    const bool built = g.hdr[kHdrBuilt] == 1 && a.mesh.n_triangles > 0;  // uniform
    const float py = centre((int) (row % a.d.y), a.vsy), pz = centre((int) (row / a.d.y), a.vsz);
    if (valid && built)
        walk_row_wave(g, a.mesh, a.brute, py, pz, lane, [&](const SignedCrossing& c) { atomicAdd(&cnt[wave][first_not_below(c.X, a.vsx, a.d.x)], c.sign); });
    __syncthreads();  // every addition has landed: from here on the counters are only read and rewritten by their own lane
    {
        int v[kPerLane], own = 0;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) v[j] = cnt[wave][kPerLane * lane + j], own += v[j];
        int incl = own;  // this lane's counters and those of every higher lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_down(incl, d, 64);
            if (lane + d < 64) incl += t;
        }
        int above = incl - own;
#pragma unroll
        for (int j = kPerLane - 1; j >= 0; --j) above += v[j], cnt[wave][kPerLane * lane + j] = above;
    }
    __syncthreads();
    double acc[kVoxPerLane];
#pragma unroll
    for (int j = 0; j < kVoxPerLane; ++j) acc[j] = 0.0;
    float seam_x = -INFINITY;  // the largest x of a boundary vertex with this row's y and z
    if (built) {
        for (int e0 = 0; e0 < a.n_boundary; e0 += kEdgeStage) {
            __syncthreads();  // the previous stage has been read
            if (e0 + lane < a.n_boundary) {
                const float4 u = a.boundary[2 * (size_t) (e0 + lane)], v = a.boundary[2 * (size_t) (e0 + lane) + 1];
                const StripRow r = strip_row(u.y, u.z, v.y, v.z, py, pz);
                e_w[wave][lane] = r.absW, e_qa[wave][lane] = r.qa, e_qb[wave][lane] = r.qb, e_dyz[wave][lane] = r.dyz;
                e_ux[wave][lane] = (double) u.x, e_vx[wave][lane] = (double) v.x, e_ks[wave][lane] = (double) r.sign * (double) u.w;
                if (r.seam_u) seam_x = fmaxf(seam_x, u.x);
                if (r.seam_v) seam_x = fmaxf(seam_x, v.x);
            }
            __syncthreads();
            const int m = min(kEdgeStage, a.n_boundary - e0);
            for (int k = 0; k < m; ++k) {
                const double ks = e_ks[wave][k];
                if (ks == 0.0) continue;  // no projected length on this row: uniform over the wave
                const StripRow r{e_w[wave][k], e_qa[wave][k], e_qb[wave][k], e_dyz[wave][k], 0, false, false};
                const double ux = e_ux[wave][k], vx = e_vx[wave][k];
#pragma unroll
                for (int j = 0; j < kVoxPerLane; ++j) {
                    const int i = lane + 64 * j;
                    if (i < a.d.x) {
                        const double px = (double) centre(i, a.vsx);
                        acc[j] += ks * strip_magnitude(r, ux - px, vx - px);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) seam_x = fmaxf(seam_x, __shfl_xor(seam_x, d, 64));
#pragma unroll
    for (int j = 0; j < kVoxPerLane; ++j) {
        const int i = lane + 64 * j;
        if (valid && i < a.d.x) {
            const size_t voxel = (size_t) row * a.d.x + i;
            if (centre(i, a.vsx) < seam_x) {
                a.seam_list[atomicAdd(a.seam_count, 1)] = (int) voxel;
            } else {
                const double w = (double) cnt[wave][i + 1] + acc[j] / kFourPi;
                if (w > 0.5) atomicOr(&obits[wave][i >> 5], 1u << (i & 31));
                if (a.winding) a.winding[voxel] = (float) w;
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    if (lane < a.nw) a.bits[(size_t) row * a.nw + lane] = obits[wave][lane];
    if (lane == 0 && (cnt[wave][0] & 1)) atomicAdd(a.open_rows, 1);
}

struct SumArgs {
    Mesh mesh;
    const float4* points;  // or
    const int* list;       // voxel indices, *count of them
    const int* count;
    int n;
    Dims d;
    float vsx, vsy, vsz;
    int flagged;     // points: only those whose w is NaN (mesh_winding_kernel's seam points)
    float* w;        // per point, or per voxel (may be NULL for the list)
    unsigned* bits;  // the list's
    int nw;
};

__global__ void __launch_bounds__(256) winding_sum_kernel(Grid g, SumArgs a) {
    __shared__ float4 sa[256], sb[256], sc[256];
    const int n      = a.list ? *a.count : a.n;  // uniform
    const bool built = g.hdr[kHdrBuilt] == 1;
    for (long long base = (long long) blockIdx.x * 256; base < n; base += (long long) gridDim.x * 256) {  // uniform over the workgroup
        const long long i = base + threadIdx.x;
        const bool have   = i < n;
        P3 p{0.f, 0.f, 0.f};
        int voxel = 0, x = 0;
        if (have) {
            if (a.list) {
                voxel = a.list[i];
                x     = voxel % a.d.x;
                p     = P3{centre(x, a.vsx), centre((voxel / a.d.x) % a.d.y, a.vsy), centre(voxel / a.d.x / a.d.y, a.vsz)};
            } else {
                p = p3(a.points[i]);
            }
        }
        const bool need = have && (!a.flagged || a.w[i] != a.w[i]);
        if (a.flagged && !__syncthreads_or(need)) continue;  // uniform: no lane of this workgroup has a seam point
        double acc = 0.0;
        if (built)
            for (int t0 = 0; t0 < a.mesh.n_triangles; t0 += 256) {
                __syncthreads();  // the previous chunk has been read
                stage_triangles(a.mesh, t0, sa, sb, sc);
                __syncthreads();
                const int m = min(256, a.mesh.n_triangles - t0);
                if (need)
                    for (int k = 0; k < m; ++k) acc += triangle_angle(from(p3(sa[k]), p), from(p3(sb[k]), p), from(p3(sc[k]), p));
            }
        if (need) {
            const double w = acc / kFourPi;
            if (a.list) {
                if (a.w) a.w[voxel] = (float) w;
                if (w > 0.5) atomicOr(&a.bits[(size_t) (voxel / a.d.x) * a.nw + (x >> 5)], 1u << (x & 31));
            } else {
                a.w[i] = (float) w;
            }
        }
    }
}

struct PointArgs {
    Mesh mesh;
    int brute;
    const float4* boundary;
    int n_boundary;
    const float4* points;
    int n;
    float* w;
};

// Every loop stays rolled, the walk's (sobfu_mesh_rows.hpp) included: left to the unroller this kernel took 314 VGPRs and spilled two
// (tests/test_no_scratch.py); rolled, 84.
__global__ void __launch_bounds__(256) mesh_winding_kernel(Grid g, PointArgs a) {
    __shared__ float4 s_u[256], s_v[256];
    const long long i = (long long) blockIdx.x * 256 + threadIdx.x;
    const bool have   = i < a.n;
    const bool built  = g.hdr[kHdrBuilt] == 1 && a.mesh.n_triangles > 0;  // uniform
    const float4 q    = have ? a.points[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const P3 p{q.x, q.y, q.z};
    const double px = (double) p.x;
    int N = 0;
    if (have && built)
        walk_row_lane(g, a.mesh, a.brute, p.y, p.z, [&](const SignedCrossing& c) {
            if (c.X > px) N += c.sign;
        });
    double acc = 0.0;
    bool seam  = false;
    if (built)
#pragma unroll 1
        for (int e0 = 0; e0 < a.n_boundary; e0 += 256) {
            __syncthreads();  // the previous stage has been read
            if (e0 + (int) threadIdx.x < a.n_boundary) {
                s_u[threadIdx.x] = a.boundary[2 * (size_t) (e0 + threadIdx.x)];
                s_v[threadIdx.x] = a.boundary[2 * (size_t) (e0 + threadIdx.x) + 1];
            }
            __syncthreads();
            const int m = min(256, a.n_boundary - e0);
            if (have)
#pragma unroll 1
                for (int k = 0; k < m; ++k) {
                    const float4 u = s_u[k], v = s_v[k];
                    const StripRow r = strip_row(u.y, u.z, v.y, v.z, p.y, p.z);
                    seam = seam || (r.seam_u && u.x > p.x) || (r.seam_v && v.x > p.x);
                    const double ks = (double) r.sign * (double) u.w;
                    if (ks != 0.0) acc += ks * strip_magnitude(r, (double) u.x - px, (double) v.x - px);
                }
        }
    if (!have) return;
    // a seam point takes the definition: flagged with a NaN for winding_sum_kernel, which the launch below sends after this kernel
    const double w = seam ? (double) NAN : (double) N + acc / kFourPi;
    a.w[i] = (float) w;
}

bool boundary_ok(const float* d_boundary, int n_boundary) { return n_boundary >= 0 && (n_boundary == 0 || d_boundary) && aligned(d_boundary, 0, 16); }

}  // namespace

extern "C" {

int sobfu_hip_mesh_boundary(const int* h_faces, int n_triangles, int n_vertices, int* h_edges, int capacity, int* h_count) {
    SOBFU_CHECK_ARGS(h_count && n_triangles >= 0 && n_vertices >= 0 && (n_triangles == 0 || h_faces) && capacity >= 0 && (capacity == 0 || h_edges));
    std::vector<BoundaryEdge> edges;
    SOBFU_CHECK_ARGS(mesh_boundary(h_faces, n_triangles, n_vertices, &edges));
    *h_count = (int) edges.size();
    if (!h_edges) return 0;
    if ((size_t) capacity < edges.size()) return SOBFU_E_UNSUPPORTED;
    for (size_t i = 0; i < edges.size(); ++i) h_edges[3 * i] = edges[i].u, h_edges[3 * i + 1] = edges[i].v, h_edges[3 * i + 2] = edges[i].k;
    return 0;
}

int sobfu_hip_mesh_winding(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                           int n_triangles, const float origin[3], float h, const int dims[3], const float* d_boundary, int n_boundary,
                           const float* d_points, int n, float* d_w, int mode, int walk, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(boundary_ok(d_boundary, n_boundary) && d_points && d_w && n >= 0 && aligned(d_points, 0, 16) && aligned(d_w, 0, 4) && mode_ok(walk) &&
                     (mode == SOBFU_MESH_WINDING_BOUNDARY || mode == SOBFU_MESH_WINDING_SUM));
    if (n == 0) return 0;
    const dim3 blocks((unsigned) (((long long) n + 255) / 256));
    if (mode == SOBFU_MESH_WINDING_SUM) {
        const SumArgs a{tg.mesh, (const float4*) d_points, nullptr, nullptr, n, {1, 1, 1}, 0.f, 0.f, 0.f, 0, d_w, nullptr, 0};
        hipLaunchKernelGGL(winding_sum_kernel, blocks, dim3(256), 0, (hipStream_t) stream, tg.grid, a);
    } else {
        const PointArgs a{tg.mesh, is_brute(walk, n_triangles), (const float4*) d_boundary, n_boundary, (const float4*) d_points, n, d_w};
        hipLaunchKernelGGL(mesh_winding_kernel, blocks, dim3(256), 0, (hipStream_t) stream, tg.grid, a);
        if (n_boundary > 0 && n_triangles > 0) {  // only a boundary makes seams
            SOBFU_HIP_TRY(hipGetLastError());
            const SumArgs s{tg.mesh, (const float4*) d_points, nullptr, nullptr, n, {1, 1, 1}, 0.f, 0.f, 0.f, 1, d_w, nullptr, 0};
            hipLaunchKernelGGL(winding_sum_kernel, blocks, dim3(256), 0, (hipStream_t) stream, tg.grid, s);
        }
    }
    return (int) hipGetLastError();
}

size_t sobfu_hip_mesh_voxelise_winding_workspace_bytes(int X, int Y, int Z) {
    if (!rows_ok(X, Y, Z) || (long long) X * Y * Z > INT_MAX) return 0;
    return bits_bytes(X, Y, Z) + 16 + (size_t) X * Y * Z * sizeof(int);
}

int sobfu_hip_mesh_voxelise_winding(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                                    int n_triangles, const float origin[3], float h, const int dims[3], const float* d_boundary, int n_boundary,
                                    float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc, float eta, int mode, void* d_workspace,
                                    size_t workspace_bytes, int* d_open_rows, float* d_winding, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(boundary_ok(d_boundary, n_boundary) && aligned(d_winding, 0, 4) && (long long) X * Y * Z <= INT_MAX &&
                     rows_volume_ok(d_vol, X, Y, Z, voxel_size, trunc, eta, mode, d_workspace, workspace_bytes,
                                    sobfu_hip_mesh_voxelise_winding_workspace_bytes(X, Y, Z), d_open_rows));
    hipStream_t st    = (hipStream_t) stream;
    char* ws          = (char*) d_workspace;
    int* seam_count   = (int*) (ws + bits_bytes(X, Y, Z));
    const RowArgs a{tg.mesh, is_brute(mode, n_triangles), {X, Y, Z}, voxel_size[0], voxel_size[1], voxel_size[2], (const float4*) d_boundary,
                    n_triangles > 0 ? n_boundary : 0, (unsigned*) d_workspace, words_per_row(X), d_winding, d_open_rows, seam_count, seam_count + 4};
    SOBFU_HIP_TRY(hipMemsetAsync(d_open_rows, 0, sizeof(int), st));
    SOBFU_HIP_TRY(hipMemsetAsync(seam_count, 0, sizeof(int), st));
    hipLaunchKernelGGL(row_winding_kernel, dim3((unsigned) (((long long) Y * Z + 3) / 4)), dim3(256), 0, st, tg.grid, a);
    SOBFU_HIP_TRY(hipGetLastError());
    if (a.n_boundary > 0) {  // only a boundary makes seams
        const SumArgs s{tg.mesh, nullptr, a.seam_list, seam_count, 0, {X, Y, Z}, voxel_size[0], voxel_size[1], voxel_size[2], 0, d_winding, a.bits, a.nw};
        hipLaunchKernelGGL(winding_sum_kernel, dim3(kSumBlocks), dim3(256), 0, st, tg.grid, s);
        SOBFU_HIP_TRY(hipGetLastError());
    }
    return mesh_voxel_bricks(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, d_vol, X, Y, Z,
                             voxel_size, trunc, eta, mode, d_workspace, d_open_rows, stream);
}

}  // extern "C"
