// Closed triangle meshes into signed TSDF volumes on gfx950, and the inside / outside test behind them.  The reference
// has no such step; the rules are this project's, and tests/mesh_parity_reference.py restates them (the row-crossing rule operation by
// operation: sobfu_mesh_parity.hpp; the distance: sobfu_mesh_distance.hpp).  The kernels only read the grid that
// sobfu_hip_mesh_grid_build made for the distance query; the grid's view, the mesh record, the corner loads, the cell range the rows and
// points ask for, the margin, the mode and the check of the leading arguments are shared (sobfu_mesh.hpp), and so are the rows: the walk
// of a row's cell column, the voxel centres and the format of the sign bits (sobfu_mesh_rows.hpp).  Vertices are in the volume's frame.
//
//   centres  voxel i of an axis has its centre at i vs + vs / 2, in fp32
//   rows     one wave per volume row (j, k), up to X = 512: lanes stride over the column's references; each crossing flips, in an LDS mask,
//            the bit of the first voxel whose centre is not below X (bit X: beyond the last voxel).  XOR is order-independent.  Voxel i
//            is inside iff the flips at bits above i are odd in number: a suffix parity, written as ceil(X / 32) words per row.  A
//            row whose flips are odd in number altogether is open: one integer atomic on the counter.
//   points   one lane per point walks its whole column and counts the crossings with X > p.x, and all of them (open).
//   volume   d = the exact minimum distance over ALL triangles (closest_on_triangle), s = inside ? -d : d, the voxel
//            pack_tsdf(s, trunc, s > -eta ? 1 : 0).  |s| at or beyond max(trunc, eta) packs to (+-1, weight by sign alone), so only
//            triangles nearer than that matter.  One 512-lane workgroup per 8 x 8 x 8 brick (ragged at the edges): the box of its voxel
//            centres grown by max(trunc, eta) + kMeshMargin L (L = the largest coordinate magnitude of the grid's box and the brick: the
//            bound on the fp32 error of one distance, as in mesh_distance_kernels.hip); the triangles referenced by the cells that
//            overlap it are gathered into LDS, each once (taken in the first overlapping cell of its own cell range), kStage at a
//            time; every lane tests every staged triangle (broadcast LDS reads).  A brick that gathers none stores +-1 from its sign bits.
//            The reach is not gathered at once: first the cells within one cell edge of the brick's box, then -- while some voxel's best
//            distance (or the saturating distance) is not below the gathered radius rho by the margin -- the cells out to that largest best
//            distance, or to 2 rho while some voxel has found nothing, less the cells already visited.  A triangle not yet gathered keeps
//            its box clear of the brick's box grown by rho, so it is farther than rho from every voxel and cannot change a bit.
//            min d2 does not depend on order: the volume is the brute-force volume bit for bit, run after run.
//   nothing  an unbuilt or refused grid, or no triangles: every voxel is (1, 1), empty space, and every point outside; the mesh is
//            not read.
#include "sobfu_hip.h"
#include "sobfu_device.hpp"
#include "sobfu_mesh_rows.hpp"

using namespace sobfu_hip;

namespace {

constexpr int kMaskWords = kMaxX / 32 + 1;  // bit X of a row: crossings beyond the last voxel
constexpr int kStage     = 1024;            // triangles staged in LDS at a time (48 B each)

struct VoxArgs {
    Mesh mesh;
    int brute;
    Dims d;
    float vsx, vsy, vsz, trunc, eta;
    float box_l;  // the largest coordinate magnitude of the grid's box
    float2* vol;
    unsigned* bits;  // Y Z rows of nw words
    int nw;
    int* open_rows;
};

__global__ void __launch_bounds__(256) row_parity_kernel(Grid g, VoxArgs a) {
    __shared__ unsigned mask[4][kMaskWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long) blockIdx.x * 4 + wave;
    const bool valid    = row < (long long) a.d.y * a.d.z;
    if (lane < kMaskWords) mask[wave][lane] = 0u;
    __syncthreads();
    if (valid && g.hdr[kHdrBuilt] == 1) {
        const float py = centre((int) (row % a.d.y), a.vsy), pz = centre((int) (row / a.d.y), a.vsz);
        walk_row_wave(g, a.mesh, a.brute, py, pz, lane, [&](const SignedCrossing& c) {
            const int i = first_not_below(c.X, a.vsx, a.d.x);
            atomicXor(&mask[wave][i >> 5], 1u << (i & 31));
        });
    }
    __syncthreads();
    if (!valid) return;
    const int nmask = a.d.x / 32 + 1;
    if (lane < a.nw) {
        unsigned s = mask[wave][lane];  // bit i: the parity of the flips at bits >= i of this word
        s ^= s >> 1, s ^= s >> 2, s ^= s >> 4, s ^= s >> 8, s ^= s >> 16;
        unsigned above = 0u;
        for (int w = lane + 1; w < nmask; ++w) above ^= mask[wave][w];
        unsigned inside = (s >> 1) ^ ((__popc(above) & 1) ? 0xffffffffu : 0u);
        if (lane == a.nw - 1 && (a.d.x & 31)) inside &= (1u << (a.d.x & 31)) - 1u;
        a.bits[(size_t) row * a.nw + lane] = inside;
    }
    if (lane == 0) {
        unsigned all = 0u;
        for (int w = 0; w < nmask; ++w) all ^= mask[wave][w];
        if (__popc(all) & 1) atomicAdd(a.open_rows, 1);
    }
}

struct InsideArgs {
    Mesh mesh;
    int brute;
    const float4* points;
    int n;
    unsigned char* inside;
    unsigned char* open;
};

__global__ void __launch_bounds__(256) mesh_inside_kernel(Grid g, InsideArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    unsigned beyond = 0u, total = 0u;
    if (g.hdr[kHdrBuilt] == 1) {
        const float4 p  = a.points[i];
        const double px = (double) p.x;
        walk_row_lane(g, a.mesh, a.brute, p.y, p.z, [&](const SignedCrossing& c) { ++total, beyond += c.X > px ? 1u : 0u; });
    }
    a.inside[i] = (unsigned char) (beyond & 1u);
    a.open[i]   = (unsigned char) (total & 1u);
}

__global__ void __launch_bounds__(512) brick_kernel(Grid g, VoxArgs a) {
    __shared__ float4 sa[kStage], sb[kStage], sc[kStage];
    __shared__ int s_count, s_reach;
    const int tid = threadIdx.x;
    const int x = blockIdx.x * kBrick + (tid & 7), y = blockIdx.y * kBrick + ((tid >> 3) & 7), z = blockIdx.z * kBrick + (tid >> 6);
    const P3 p{centre(x, a.vsx), centre(y, a.vsy), centre(z, a.vsz)};
    float best = INFINITY;
    const Mesh& m = a.mesh;
    auto test = [&](int count) {
        for (int k = 0; k < count; ++k) best = fminf(best, closest_on_triangle(p, p3(sa[k]), p3(sb[k]), p3(sc[k])).d2);
    };
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (g.hdr[kHdrBuilt] == 1 && m.n_triangles > 0) {  // uniform over the workgroup, like every loop bound below
        if (a.brute) {
            for (int t0 = 0; t0 < m.n_triangles; t0 += kStage) {
                __syncthreads();  // the previous chunk has been read
                for (int s = tid; s < kStage && t0 + s < m.n_triangles; s += 512) {
                    const Corners v = corners_of(m, t0 + s);
                    sa[s] = v.a, sb[s] = v.b, sc[s] = v.c;
                }
                __syncthreads();
                test(min(kStage, m.n_triangles - t0));
            }
        } else {
            const float lx = centre(blockIdx.x * kBrick, a.vsx), hx = centre(min((int) blockIdx.x * kBrick + kBrick, a.d.x) - 1, a.vsx);
            const float ly = centre(blockIdx.y * kBrick, a.vsy), hy = centre(min((int) blockIdx.y * kBrick + kBrick, a.d.y) - 1, a.vsy);
            const float lz = centre(blockIdx.z * kBrick, a.vsz), hz = centre(min((int) blockIdx.z * kBrick + kBrick, a.d.z) - 1, a.vsz);
            const float L = fmaxf(fmaxf(a.box_l, fmaxf(fabsf(lx), fabsf(hx))), fmaxf(fmaxf(fabsf(ly), fabsf(hy)), fmaxf(fabsf(lz), fabsf(hz))));
            const float margin = kMeshMargin * L, cap = fmaxf(a.trunc, a.eta), r = cap + margin;
            const bool in_volume = x < a.d.x && y < a.d.y && z < a.d.z;
            // the cells visited so far (p): none; plain ints, selected one by one: a select between two structs goes through the stack
            int px0 = 1, px1 = 0, py0 = 1, py1 = 0, pz0 = 1, pz1 = 0;
            int examined = 0;  // references looked at since the stage was last emptied: at least the triangles staged
            for (float rho = fminf(g.h, r);;) {
                // the cells that overlap the brick's box grown by rho (n), less those of the radius before
                const bool near = hx + rho >= g.ox && lx - rho <= g.ox + (float) g.dx * g.h && hy + rho >= g.oy && ly - rho <= g.oy + (float) g.dy * g.h &&
                                  hz + rho >= g.oz && lz - rho <= g.oz + (float) g.dz * g.h;
                const int nx0 = near ? cell_of(lx - rho, g.ox, g.h, g.dx) : px0, nx1 = near ? cell_of(hx + rho, g.ox, g.h, g.dx) : px1;
                const int ny0 = near ? cell_of(ly - rho, g.oy, g.h, g.dy) : py0, ny1 = near ? cell_of(hy + rho, g.oy, g.h, g.dy) : py1;
                const int nz0 = near ? cell_of(lz - rho, g.oz, g.h, g.dz) : pz0, nz1 = near ? cell_of(hz + rho, g.oz, g.h, g.dz) : pz1;
                const bool had = px0 <= px1;
                for (int cz = nz0; cz <= nz1; ++cz)
                    for (int cy = ny0; cy <= ny1; ++cy) {
                        const int* start  = g.start + g.dx * (cy + g.dy * cz);
                        const bool inner  = had && cz >= pz0 && cz <= pz1 && cy >= py0 && cy <= py1;  // this row's middle is done
                        for (int part = 0; part < (inner ? 2 : 1); ++part) {
                            const int xa = inner && part == 1 ? px1 + 1 : nx0, xb = inner && part == 0 ? px0 - 1 : nx1;
                            if (xa > xb) continue;
                            const int k1 = start[xb + 1];
                            for (int kb = start[xa]; kb < k1; kb += 512) {
                                // room for a whole pass?  Decided on the references examined, not on s_count: a wave ahead may already
                                // be adding to that, and every lane has to take the same branch to the barriers
                                if (examined + 512 > kStage) {
                                    test(s_count);
                                    __syncthreads();
                                    if (tid == 0) s_count = 0;
                                    __syncthreads();
                                    examined = 0;
                                }
                                examined += min(512, k1 - kb);
                                const int k = kb + tid;
                                if (k < k1) {
                                    const auto [va, vb, vc] = corners_of(m, g.refs[k]);
                                    // the cell range, written out as cells_of (sobfu_mesh.hpp) has it: through cells_of, and with another form
                                    // of the staging loop above, this kernel measured 0.8 % and 4.4 % slower (profiles/mesh_side_home.md)
                                    const int tx0 = cell_of(fminf(fminf(va.x, vb.x), vc.x), g.ox, g.h, g.dx), tx1 = cell_of(fmaxf(fmaxf(va.x, vb.x), vc.x), g.ox, g.h, g.dx);
                                    const int ty0 = cell_of(fminf(fminf(va.y, vb.y), vc.y), g.oy, g.h, g.dy), ty1 = cell_of(fmaxf(fmaxf(va.y, vb.y), vc.y), g.oy, g.h, g.dy);
                                    const int tz0 = cell_of(fminf(fminf(va.z, vb.z), vc.z), g.oz, g.h, g.dz), tz1 = cell_of(fmaxf(fmaxf(va.z, vb.z), vc.z), g.oz, g.h, g.dz);
                                    // taken at an earlier radius: its cells met those visited then
                                    const bool seen = had && tx0 <= px1 && tx1 >= px0 && ty0 <= py1 && ty1 >= py0 && tz0 <= pz1 && tz1 >= pz0;
                                    // else once, in the first of its cells inside the range
                                    if (!seen && max(ty0, ny0) == cy && max(tz0, nz0) == cz && max(tx0, nx0) == cell_of_reference(start, xa, xb, k)) {
                                        const int slot = atomicAdd(&s_count, 1);
                                        sa[slot] = va, sb[slot] = vb, sc[slot] = vc;
                                    }
                                }
                                __syncthreads();
                            }
                        }
                    }
                test(s_count);
                if (!(rho < r)) break;  // the whole reach has been gathered
                // Every triangle not yet seen keeps its box clear of the brick's box grown by rho: it is farther than rho from every voxel.
                // Once every voxel's best distance -- or the cap beyond which the voxel saturates whatever the distance -- is below rho by
                // the margin, none of them can change a bit.
                __syncthreads();
                if (tid == 0) s_count = 0, s_reach = 0;
                examined = 0;
                __syncthreads();
                if (in_volume) atomicMax(&s_reach, __float_as_int(fminf(__builtin_sqrtf(best), cap)));  // non-negative floats order as their bits
                __syncthreads();
                const float reach = __int_as_float(s_reach);
                if (reach + margin <= rho) break;
                px0 = nx0, px1 = nx1, py0 = ny0, py1 = ny1, pz0 = nz0, pz1 = nz1;
                // every voxel has a triangle within reach < cap: nothing beyond reach matters, and the next round is the last (best only
                // falls).  Else some voxel has found nothing yet: twice as far
                rho = fminf(reach < cap ? reach + margin : 2.f * rho, r);
            }
        }
    }
    if (x >= a.d.x || y >= a.d.y || z >= a.d.z) return;
    const bool inside = (a.bits[((size_t) z * a.d.y + y) * a.nw + (x >> 5)] >> (x & 31)) & 1u;
    const float d = __builtin_sqrtf(best), s = inside ? -d : d;
    a.vol[vidx(a.d, x, y, z)] = pack_tsdf(s, a.trunc, s > -a.eta ? 1.f : 0.f);
}

}  // namespace

namespace sobfu_hip {

// declared, with what it takes, in sobfu_mesh_rows.hpp
int mesh_voxel_bricks(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                      const float origin[3], float h, const int dims[3], float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc,
                      float eta, int mode, void* d_bits, int* d_open_rows, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    const VoxArgs a{tg.mesh, is_brute(mode, n_triangles), {X, Y, Z}, voxel_size[0], voxel_size[1], voxel_size[2], trunc, eta, tg.box_l, (float2*) d_vol,
                    (unsigned*) d_bits, words_per_row(X), d_open_rows};
    const dim3 bricks((unsigned) ((X + kBrick - 1) / kBrick), (unsigned) ((Y + kBrick - 1) / kBrick), (unsigned) ((Z + kBrick - 1) / kBrick));
    hipLaunchKernelGGL(brick_kernel, bricks, dim3(512), 0, (hipStream_t) stream, tg.grid, a);
    return (int) hipGetLastError();
}

}  // namespace sobfu_hip

extern "C" {

size_t sobfu_hip_mesh_voxelise_workspace_bytes(int X, int Y, int Z) {
    if (!rows_ok(X, Y, Z) || (long long) Y * Z > INT_MAX) return 0;
    return bits_bytes(X, Y, Z);
}

int sobfu_hip_mesh_voxelise(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                            int n_triangles, const float origin[3], float h, const int dims[3], float* d_vol, int X, int Y, int Z,
                            const float voxel_size[3], float trunc, float eta, int mode, void* d_workspace, size_t workspace_bytes,
                            int* d_open_rows, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(rows_volume_ok(d_vol, X, Y, Z, voxel_size, trunc, eta, mode, d_workspace, workspace_bytes, bits_bytes(X, Y, Z), d_open_rows) &&
                     (long long) Y * Z <= INT_MAX);
    hipStream_t st = (hipStream_t) stream;
    const VoxArgs a{tg.mesh, is_brute(mode, n_triangles), {X, Y, Z}, voxel_size[0], voxel_size[1], voxel_size[2], trunc, eta, tg.box_l, (float2*) d_vol,
                    (unsigned*) d_workspace, words_per_row(X), d_open_rows};
    SOBFU_HIP_TRY(hipMemsetAsync(d_open_rows, 0, sizeof(int), st));
    hipLaunchKernelGGL(row_parity_kernel, dim3((unsigned) (((long long) Y * Z + 3) / 4)), dim3(256), 0, st, tg.grid, a);
    SOBFU_HIP_TRY(hipGetLastError());
    return mesh_voxel_bricks(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, d_vol, X, Y, Z,
                             voxel_size, trunc, eta, mode, d_workspace, d_open_rows, stream);
}

int sobfu_hip_mesh_inside(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                          int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, uint8_t* d_inside,
                          uint8_t* d_open, int mode, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_grid_workspace, grid_workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(d_points && d_inside && d_open && n >= 0 && aligned(d_points, 0, 16) && mode_ok(mode));
    if (n == 0) return 0;
    const InsideArgs a{tg.mesh, is_brute(mode, n_triangles), (const float4*) d_points, n, d_inside, d_open};
    hipLaunchKernelGGL(mesh_inside_kernel, dim3((unsigned) (((long long) n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, tg.grid, a);
    return (int) hipGetLastError();
}

}  // extern "C"
