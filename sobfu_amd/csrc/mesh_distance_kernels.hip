// Exact point-to-mesh distances on gfx950: for every query point the nearest triangle of an indexed mesh, its distance and its closest
// point.  The reference has no such step; the rules are this project's, and tests/mesh_distance_reference.py restates
// them (the point-triangle rule operation by operation: sobfu_mesh_distance.hpp).
//
//   answer   per point: min over all triangles of d2 (closest_on_triangle), the LOWEST triangle index attaining it, that triangle's
//            closest point; dist = sqrt(min d2).  With max_dist: dist > max_dist -> (+Inf, -1, (0, 0, 0, 0)).  No triangles: the same.
//            The answer does not depend on the path that finds it: grid and brute force agree bit for bit, run after run.
//   grid     a uniform grid of cubic cells over the mesh's box (the plan: sobfu_mesh_grid.hpp; the workspace's layout, the mesh record and
//            all else the ray and voxel kernels share: sobfu_mesh.hpp).  A triangle is referenced from every cell its axis-aligned box
//            overlaps (cells_of).  build: count per cell (integer atomics) -> exclusive scan (sobfu_scan.hpp) -> fill
//            (cursors: the counts, counted back down).  The order of the references inside a cell varies from run to run; the answer
//            does not (the tie rule).  The count pass also raises a flag for a face index outside [0, n_vertices) or a non-finite
//            corner: build then returns SOBFU_E_BADARG and the workspace stays unmarked -- every query through it answers (+Inf, -1).
//   query    one lane per point (marching-cubes vertex order is spatially coherent: the lanes of a wave walk neighbouring cells).
//            Shells of Chebyshev radius r = 0, 1, 2, ... around the point's cell (the nearest cell for a point outside the box).  After
//            shell r every unvisited triangle is at least r h away, so the walk stops when min(best, max_dist) + margin <= r h, or when
//            the shells have covered the grid.  margin = kMeshMargin L, L = the largest coordinate magnitude of the box and the point:
//            an absolute bound on the fp32 error of one point-triangle distance (measured <= 3.0e-7 L, tests/test_mesh_distance_cpu.py),
//            so an unvisited triangle can neither beat nor tie the best one and pruning never depends on last bits.
//   ring cap a point still unresolved after shell ring_cap (default kMeshGridRingCap) is appended to a list (one integer atomic) and
//            finished by the brute-force kernel: a far-off point must not walk millions of empty cells.
//   brute    a 256-lane workgroup per 256 points, the triangles staged through LDS 256 at a time (48 B each), every lane testing the
//            same triangle (a broadcast LDS read) in ascending index order.  Also the whole call for mode brute and for tiny meshes.
#include "sobfu_hip.h"
#include "sobfu_mesh.hpp"
#include "sobfu_scan.hpp"

using namespace sobfu_hip;

namespace {

// one lane per triangle: FILL = false counts the cells its box overlaps (and checks it), FILL = true writes the references
template <bool FILL>
__global__ void __launch_bounds__(256) bin_triangles_kernel(Grid g, const float4* __restrict__ verts, int n_vertices, const int* __restrict__ faces,
                                                            int n_triangles) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long cells = 0;
    if (i < n_triangles) {
        const Mesh m{verts, faces, n_triangles};
        const int3 f = face_of(m, i);
        bool ok = f.x >= 0 && f.x < n_vertices && f.y >= 0 && f.y < n_vertices && f.z >= 0 && f.z < n_vertices;
        Corners t{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
        if (ok) {
            t  = corners_of(m, f);
            ok = finite3(t.a) && finite3(t.b) && finite3(t.c);
        }
        if (!ok) {
            if (!FILL) atomicOr(g.hdr + kHdrBad, 1);
        } else {
            const CellRange r = cells_of(g, t);
            cells = (unsigned long long) (r.x1 - r.x0 + 1) * (unsigned long long) (r.y1 - r.y0 + 1) * (unsigned long long) (r.z1 - r.z0 + 1);
            for (int z = r.z0; z <= r.z1; ++z)
                for (int y = r.y0; y <= r.y1; ++y)
                    for (int x = r.x0; x <= r.x1; ++x) {
                        const int cell = x + g.dx * (y + g.dy * z);
                        if (!FILL) {
                            atomicAdd(g.count + cell, 1);
                        } else {
                            const int pos = g.start[cell] + atomicSub(g.count + cell, 1) - 1;
                            if (pos >= 0 && pos < g.max_refs) g.refs[pos] = i;
                        }
                    }
        }
    }
    if (!FILL) {  // the number of references, in 64 bits: one atomic per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cells += __shfl_down(cells, o, 64);
        if ((threadIdx.x & 63) == 0 && cells) atomicAdd((unsigned long long*) (g.hdr + kHdrRefs), cells);
    }
}

struct Query {
    Mesh mesh;
    const float4* points;
    int n;
    float max_dist;  // +Inf: unlimited
    float box_l;     // the largest coordinate magnitude of the grid's box
    int ring_cap;
    float* dist;
    int* tri;
    float4* closest;  // may be null
    int* list;        // unresolved points
};

struct Best {
    float d2;
    int tri;
    P3 q;
};

SOBFU_DEV void write_answer(const Query& a, int i, const Best& b) {
    const float d   = __builtin_sqrtf(b.d2);
    const bool hit  = b.tri >= 0 && !(d > a.max_dist);
    a.dist[i]       = hit ? d : INFINITY;
    a.tri[i]        = hit ? b.tri : -1;
    if (a.closest) a.closest[i] = hit ? make_float4(b.q.x, b.q.y, b.q.z, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

SOBFU_DEV void visit_cell(const Grid& g, const Query& a, const P3& p, int cell, Best& best) {
    const int end = g.start[cell + 1];
    for (int k = g.start[cell]; k < end; ++k) {
        const int t = g.refs[k];
        const Corners v = corners_of(a.mesh, t);
        const Closest c = closest_on_triangle(p, p3(v.a), p3(v.b), p3(v.c));
        if (c.d2 < best.d2 || (c.d2 == best.d2 && t < best.tri)) best = Best{c.d2, t, c.q};
    }
}

__global__ void __launch_bounds__(256) grid_query_kernel(Grid g, Query a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    Best best{INFINITY, -1, P3{0.f, 0.f, 0.f}};
    if (g.hdr[kHdrBuilt] != 1) {  // a grid whose build was refused
        write_answer(a, i, best);
        return;
    }
    const float4 p4 = a.points[i];
    const P3 p      = p3(p4);
    const float L      = fmaxf(fmaxf(a.box_l, fabsf(p.x)), fmaxf(fabsf(p.y), fabsf(p.z)));
    const float margin = kMeshMargin * L;
    const int cx = cell_of(p.x, g.ox, g.h, g.dx), cy = cell_of(p.y, g.oy, g.h, g.dy), cz = cell_of(p.z, g.oz, g.h, g.dz);
    bool resolved = false;
    for (int r = 0;; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.dy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int row = g.dx * (y + g.dy * z);
                if (abs(z - cz) == r || abs(y - cy) == r) {  // a face of the shell: the whole row
                    for (int x = x0; x <= x1; ++x) visit_cell(g, a, p, row + x, best);
                } else {  // inside in y and z: the two end cells
                    if (cx - r >= 0) visit_cell(g, a, p, row + cx - r, best);
                    if (r > 0 && cx + r < g.dx) visit_cell(g, a, p, row + cx + r, best);
                }
            }
        const bool covered = cx - r <= 0 && cx + r >= g.dx - 1 && cy - r <= 0 && cy + r >= g.dy - 1 && cz - r <= 0 && cz + r >= g.dz - 1;
        if (covered || fminf(__builtin_sqrtf(best.d2), a.max_dist) + margin <= (float) r * g.h) {
            resolved = true;
            break;
        }
        if (r >= a.ring_cap) break;
    }
    if (resolved) write_answer(a, i, best);
    else a.list[atomicAdd(g.hdr + kHdrUnresolved, 1)] = i;
}

// LIST: the points of a.list (their number: the header's counter), else all n points
template <bool LIST>
__global__ void __launch_bounds__(256) brute_force_kernel(const int* __restrict__ hdr, Query a) {
    __shared__ float4 sa[256], sb[256], sc[256];
    const int count = LIST ? hdr[kHdrUnresolved] : a.n;
    const int slot  = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= count) return;  // the whole workgroup
    const bool active = slot < count;
    const int i       = active ? (LIST ? a.list[slot] : slot) : 0;
    const bool built  = hdr[kHdrBuilt] == 1;
    const P3 p        = p3(a.points[i]);
    Best best{INFINITY, -1, P3{0.f, 0.f, 0.f}};
    for (int t0 = 0; built && t0 < a.mesh.n_triangles; t0 += 256) {
        __syncthreads();  // the previous chunk has been read
        stage_triangles(a.mesh, t0, sa, sb, sc);
        __syncthreads();
        const int m = min(256, a.mesh.n_triangles - t0);
        for (int k = 0; k < m; ++k) {
            const Closest c = closest_on_triangle(p, p3(sa[k]), p3(sb[k]), p3(sc[k]));
            if (c.d2 < best.d2) best = Best{c.d2, t0 + k, c.q};  // ascending index: the first minimum is the lowest
        }
    }
    if (active) write_answer(a, i, best);
}

}  // namespace

extern "C" {

int sobfu_hip_mesh_grid_plan(const float bbox[6], int n_triangles, float cell, float origin[3], float* h, int dims[3]) {
    SOBFU_CHECK_ARGS(bbox && origin && h && dims);
    MeshGridPlan p;
    SOBFU_CHECK_ARGS(mesh_grid_plan(bbox, n_triangles, cell, &p));
    for (int i = 0; i < 3; ++i) origin[i] = p.origin[i], dims[i] = p.dims[i];
    *h = p.h;
    return 0;
}

size_t sobfu_hip_mesh_grid_workspace_bytes(const int dims[3], int max_refs) {
    if (!dims || max_refs < 0) return 0;
    for (int i = 0; i < 3; ++i)
        if (dims[i] < 1 || dims[i] > kMeshGridMaxDim) return 0;
    return grid_ints(dims, max_refs) * sizeof(int);
}

int sobfu_hip_mesh_grid_build(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, const float origin[3], float h,
                              const int dims[3], void* d_workspace, size_t workspace_bytes, int max_refs, int* h_refs, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(h_refs && mesh_target(d_workspace, workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, max_refs, &tg));
    hipStream_t st = (hipStream_t) stream;
    const Grid& g  = tg.grid;
    const int nc   = (int) ncells_of(dims) + 1;
    const dim3 blocks((unsigned) (((long long) n_triangles + 255) / 256));
    SOBFU_HIP_TRY(hipMemsetAsync(g.hdr, 0, (size_t) (kHdrInts + nc) * sizeof(int), st));
    if (n_triangles > 0) {
        hipLaunchKernelGGL(bin_triangles_kernel<false>, blocks, dim3(256), 0, st, g, tg.mesh.verts, n_vertices, d_faces, n_triangles);
        SOBFU_HIP_TRY(hipGetLastError());
    }
    SOBFU_TRY(scan_exclusive(g.count, nc, g.start, g.blk, st));
    int hdr[4];
    SOBFU_HIP_TRY(hipMemcpyAsync(hdr, g.hdr, sizeof hdr, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    if (hdr[kHdrBad]) return SOBFU_E_BADARG;
    unsigned long long total;
    std::memcpy(&total, hdr + kHdrRefs, sizeof total);
    if (total > (unsigned long long) INT_MAX) return SOBFU_E_UNSUPPORTED;
    *h_refs = (int) total;
    if ((int) total > max_refs) return SOBFU_E_UNSUPPORTED;  // the caller enlarges the workspace to *h_refs and builds again
    if (n_triangles > 0) {
        hipLaunchKernelGGL(bin_triangles_kernel<true>, blocks, dim3(256), 0, st, g, tg.mesh.verts, n_vertices, d_faces, n_triangles);
        SOBFU_HIP_TRY(hipGetLastError());
    }
    return (int) hipMemsetD32Async((hipDeviceptr_t) (g.hdr + kHdrBuilt), 1, 1, st);
}

int sobfu_hip_mesh_distance(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                            const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist, int mode,
                            int ring_cap, float* d_dist, int* d_tri, float* d_closest, int* d_unresolved, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_workspace, workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(d_points && d_dist && d_tri && n >= 0 && aligned(d_points, 0, 16) && aligned(d_dist, 0, 4) && aligned(d_tri, 0, 4) &&
                     aligned(d_closest, 0, 16) && aligned(d_unresolved, 0, 4));
    SOBFU_CHECK_ARGS(!std::isnan(max_dist) && mode_ok(mode) && ring_cap >= 0 && (mode == SOBFU_MESH_DISTANCE_BRUTE || d_unresolved));
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    const Grid& g  = tg.grid;
    const Query q{tg.mesh, (const float4*) d_points, n, max_dist > 0.f ? max_dist : INFINITY, tg.box_l, ring_cap > 0 ? ring_cap : kMeshGridRingCap,
                  d_dist, d_tri, (float4*) d_closest, d_unresolved};
    const dim3 blocks((unsigned) (((long long) n + 255) / 256));
    SOBFU_HIP_TRY(hipMemsetAsync(g.hdr + kHdrUnresolved, 0, sizeof(int), st));
    if (is_brute(mode, n_triangles)) {
        hipLaunchKernelGGL(brute_force_kernel<false>, blocks, dim3(256), 0, st, (const int*) g.hdr, q);
        return (int) hipGetLastError();
    }
    hipLaunchKernelGGL(grid_query_kernel, blocks, dim3(256), 0, st, g, q);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(brute_force_kernel<true>, blocks, dim3(256), 0, st, (const int*) g.hdr, q);
    return (int) hipGetLastError();
}

int sobfu_hip_mesh_distance_unresolved(const void* d_workspace, int* h_count, void* stream) {
    SOBFU_CHECK_ARGS(d_workspace && h_count && aligned(d_workspace, 0, 16));
    SOBFU_HIP_TRY(hipMemcpyAsync(h_count, (const int*) d_workspace + kHdrUnresolved, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t) stream));
    return (int) hipStreamSynchronize((hipStream_t) stream);
}

}  // extern "C"
