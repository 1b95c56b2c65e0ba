// Marching cubes over a TSDF volume on gfx950 -- counterpart of src/kfusion/cuda/marching_cubes.cu + the host wrapper
// src/kfusion/marching_cubes.cpp.  Not on the solver's hot path: once per extracted mesh.
//
// The reference compacts active cells with a global atomic counter, so its voxel (and therefore triangle) ORDER differs
// from run to run.  Here the order is deterministic -- ascending voxel index, the canonical member of that family -- by
// compacting with a three-kernel exclusive scan (per-block sums -> one-block scan of the sums -> per-block scatter)
// instead of atomics; the same scan then turns the per-voxel vertex counts into vertex offsets (the reference uses
// thrust::exclusive_scan).  Classification is one lane per cell with x fastest: the 8 corner reads of a wave are 4 pairs
// of neighbouring 512-byte row segments, served by L1/L2.
//
// Arithmetic conventions: see oracle/sobfu_oracle.c (marching-cubes block) -- IEEE / and sqrt, no contraction, fma only in
// dot() and pose * vertex.
//
// The indexed (welded) path below reuses classify_kernel and the scans: an edge-mask pass, a vertex pass and a face pass.
#include <cstdlib>

#include "sobfu_device.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_scan.hpp"

using namespace sobfu_hip;

namespace {

__device__ const uint64_t kTri[256] = {
#include "mc_table.inc"
};

SOBFU_DEV int tri_edge(uint64_t row, int k) { return (int) ((row >> (4 * k)) & 15u); }
SOBFU_DEV int num_verts(uint64_t row) {  // entries before the first 0xF nibble (numVertsTable)
    // a nibble is 0xF iff all four bits are set: AND the four bit planes, find the first set nibble
    uint64_t m = row & (row >> 1) & (row >> 2) & (row >> 3) & 0x1111111111111111ull;
    return m ? (int) (__builtin_ctzll(m) >> 2) : 16;
}

// CubeIndexEstimator::computeCubeIndex (marching_cubes.cu:38-79), isoValue = 0
SOBFU_DEV int cube_index(const float2* __restrict__ vol, const Dims& d, int x, int y, int z, float f[8]) {
    const size_t sy = (size_t) d.x, sz = (size_t) d.x * d.y, o = vidx(d, x, y, z);
    const size_t off[8] = {o, o + 1, o + 1 + sy, o + sy, o + sz, o + 1 + sz, o + 1 + sy + sz, o + sy + sz};
    bool seen = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float2 v = vol[off[c]];
        f[c]     = v.x;
        seen     = seen && v.y != 0.f;
    }
    if (!seen) return 0;
    int cube = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cube += (f[c] < 0.f) << c;
    return cube;
}

// pass 1: vertex count of every cell (uint8 scratch) + per-workgroup number of active cells
__global__ void __launch_bounds__(kBlock) classify_kernel(const float2* __restrict__ vol, Dims d, uint8_t* __restrict__ nv_out,
                                                          int* __restrict__ block_cnt) {
    __shared__ int s_wave[kBlock / 64 + 1];
    const size_t N = (size_t) d.x * d.y * d.z, base = (size_t) blockIdx.x * kChunk;
    int active = 0;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const size_t i = base + (size_t) it * kBlock + threadIdx.x;
        int nv = 0;
        if (i < N) {
            const int x = (int) (i % d.x), y = (int) ((i / d.x) % d.y), z = (int) (i / ((size_t) d.x * d.y));
            if (x + 1 < d.x && y + 1 < d.y && z + 1 < d.z) {
                float f[8];
                const int cube = cube_index(vol, d, x, y, z, f);
                nv = (cube == 0 || cube == 255) ? 0 : num_verts(kTri[cube]);
            }
            nv_out[i] = (uint8_t) nv;
        }
        active += nv > 0;
    }
    int total;
    block_exclusive(active, &total, s_wave);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

// the indexed path's three per-workgroup arrays (consecutive, n ints each; totals consecutive): one workgroup per array
__global__ void __launch_bounds__(1024) scan_blocks3_kernel(int* __restrict__ v, int n, int* __restrict__ totals) {
    scan_blocks(v + (size_t) blockIdx.x * n, n, totals + blockIdx.x);
}

// pass 3: scatter the active cells of each workgroup in ascending index order
__global__ void __launch_bounds__(kBlock) compact_kernel(const uint8_t* __restrict__ nv_in, size_t N, const int* __restrict__ block_off,
                                                         int* __restrict__ voxel_idx, int* __restrict__ voxel_nv, int max_size) {
    __shared__ int s_wave[kBlock / 64 + 1];
    const size_t base = (size_t) blockIdx.x * kChunk;
    int run = block_off[blockIdx.x];
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const size_t i = base + (size_t) it * kBlock + threadIdx.x;
        const int nv = i < N ? nv_in[i] : 0;
        int total;
        const int pos = run + block_exclusive(nv > 0, &total, s_wave);
        if (nv > 0 && pos < max_size) {
            voxel_idx[pos] = (int) i;
            voxel_nv[pos]  = nv;
        }
        run += total;
    }
}

struct Pose {
    float R[9], t[3];
};

SOBFU_DEV void interp(const float p0[3], const float p1[3], float f0, float f1, float out[3]) {  // vertex_interp :193-199
    const float t = (0.f - f0) / (f1 - f0 + 1e-15f);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = p0[k] + t * (p1[k] - p0[k]);
}

// TrianglesGenerator::operator() (marching_cubes.cu:201-268): one lane per active cell
__global__ void __launch_bounds__(256) triangles_kernel(const float2* __restrict__ vol, Dims d, const int* __restrict__ voxel_idx,
                                                        const int* __restrict__ vertex_off, int count, float csx, float csy, float csz,
                                                        Pose pose, float4* __restrict__ out_v, float4* __restrict__ out_n, int max_vertices) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const int voxel = voxel_idx[idx];
    const int z = voxel / (d.x * d.y), y = (voxel - z * d.x * d.y) / d.x, x = (voxel - z * d.x * d.y) - y * d.x;
    float f[8];
    const int cube = cube_index(vol, d, x, y, z, f);
    const uint64_t row = kTri[cube];
    const int nv = num_verts(row), first = vertex_off[idx];
    const float cx[2] = {((float) x + 0.5f) * csx, ((float) (x + 1) + 0.5f) * csx};  // get_node_coo :183-191
    const float cy[2] = {((float) y + 0.5f) * csy, ((float) (y + 1) + 0.5f) * csy};
    const float cz[2] = {((float) z + 0.5f) * csz, ((float) (z + 1) + 0.5f) * csz};
    for (int i = 0; i < nv; i += 3) {
        if (first + i + 3 > max_vertices) break;
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // edge e joins corners (ea, eb): 0-3 bottom ring, 4-7 top ring, 8-11 verticals (:232-243)
            const int e = tri_edge(row, i + k);
            const int ea = e < 8 ? e : e - 8, eb = e < 8 ? ((e & 3) == 3 ? e - 3 : e + 1) : e - 4;
            // corner c: x offset = ((c & 3) == 1 || (c & 3) == 2), y offset = (c & 3) >= 2, z offset = c >> 2
            const float a[3] = {cx[((ea & 3) == 1) | ((ea & 3) == 2)], cy[(ea & 3) >> 1], cz[ea >> 2]};
            const float b[3] = {cx[((eb & 3) == 1) | ((eb & 3) == 2)], cy[(eb & 3) >> 1], cz[eb >> 2]};
            float fa = 0.f, fb = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {  // select without dynamic indexing of f[] (keeps it in registers)
                fa = c == ea ? f[c] : fa;
                fb = c == eb ? f[c] : fb;
            }
            interp(a, b, fa, fb, p[k]);
        }
        // normalized(cross(v3 - v1, v2 - v1)) (:258), one normal per triangle
        const float ax = p[2][0] - p[0][0], ay = p[2][1] - p[0][1], az = p[2][2] - p[0][2];
        const float bx = p[1][0] - p[0][0], by = p[1][1] - p[0][1], bz = p[1][2] - p[0][2];
        const float c[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
        const float inv  = 1.f / __builtin_sqrtf(dot3(c, c[0], c[1], c[2]));
        const float4 n   = make_float4(c[0] * inv, -(c[1] * inv), -(c[2] * inv), 1.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // pose * vertex, store_point (:260-273)
            const float wx = dot3(pose.R + 0, p[k][0], p[k][1], p[k][2]) + pose.t[0];
            const float wy = dot3(pose.R + 3, p[k][0], p[k][1], p[k][2]) + pose.t[1];
            const float wz = dot3(pose.R + 6, p[k][0], p[k][1], p[k][2]) + pose.t[2];
            out_v[first + i + k] = make_float4(wx, -wy, -wz, 1.f);
            out_n[first + i + k] = n;
        }
    }
}

// ---- indexed (welded) meshes: one vertex per cut grid edge, shared by every triangle that uses it ----------------------------------
// Voxel v owns the grid edges leaving its corner in +x, +y, +z (bits 0, 1, 2 of its edge mask).  An owned edge carries a vertex iff it is
// cut ((f_v < 0) != (f_{v+axis} < 0), cube_index's sign rule) and one of the <= 4 cells sharing it is active (classify_kernel's vertex
// count != 0) -- the case table triangulates exactly the edges a case cuts, so that is "referenced by some triangle".  Vertices come in
// ascending owner index, then axis; vertex index = base[owner] + popcount(mask[owner] & ((1 << axis) - 1)), base = exclusive scan of
// popcount(mask).  Face k is soup triangle k with corners 1 and 2 swapped (counter-clockwise seen from outside).

// table edge e -> (owner offset, axis): 5-bit fields dx | dy << 1 | dz << 2 | axis << 3 (a shift instead of an indexed array: no scratch)
constexpr uint64_t kEdgeOwner = (0ull << 0) | (9ull << 5) | (2ull << 10) | (8ull << 15) | (4ull << 20) | (13ull << 25) | (6ull << 30) |
                                (12ull << 35) | (16ull << 40) | (17ull << 45) | (19ull << 50) | (18ull << 55);

// x, y, z of voxel i < 2^31 with 32-bit divisions (the indexed entry points refuse larger volumes)
SOBFU_DEV void coords32(size_t i, const Dims& d, int& x, int& y, int& z) {
    const unsigned u = (unsigned) i, r = u / (unsigned) d.x;
    x = (int) (u - r * (unsigned) d.x);
    z = (int) (r / (unsigned) d.y);
    y = (int) (r - (unsigned) z * (unsigned) d.y);
}

// pass 2 of the indexed path: per-voxel edge mask + per-workgroup sums of the soup vertex counts (nv) and of the welded vertices
__global__ void __launch_bounds__(kBlock) edge_mask_kernel(const float2* __restrict__ vol, Dims d, const uint8_t* __restrict__ nv,
                                                           uint8_t* __restrict__ mask_out, int* __restrict__ blk_tri, int* __restrict__ blk_vert) {
    __shared__ int s_wave[kBlock / 64 + 1];
    const size_t N = (size_t) d.x * d.y * d.z, base = (size_t) blockIdx.x * kChunk, sy = (size_t) d.x, sz = (size_t) d.x * d.y;
    int tri = 0, vert = 0;
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const size_t i = base + (size_t) it * kBlock + threadIdx.x;
        if (i >= N) break;
        int x, y, z;
        coords32(i, d, x, y, z);
        const bool neg = vol[i].x < 0.f;
        int m = 0;
        // x edge: cells (x, y - dy, z - dz); y edge: (x - dx, y, z - dz); z edge: (x - dx, y - dy, z).  nv is 0 on the upper faces.
        if (x + 1 < d.x && (vol[i + 1].x < 0.f) != neg) {
            const bool a = nv[i] || (y > 0 && nv[i - sy]) || (z > 0 && nv[i - sz]) || (y > 0 && z > 0 && nv[i - sy - sz]);
            m |= a ? 1 : 0;
        }
        if (y + 1 < d.y && (vol[i + sy].x < 0.f) != neg) {
            const bool a = nv[i] || (x > 0 && nv[i - 1]) || (z > 0 && nv[i - sz]) || (x > 0 && z > 0 && nv[i - 1 - sz]);
            m |= a ? 2 : 0;
        }
        if (z + 1 < d.z && (vol[i + sz].x < 0.f) != neg) {
            const bool a = nv[i] || (x > 0 && nv[i - 1]) || (y > 0 && nv[i - sy]) || (x > 0 && y > 0 && nv[i - 1 - sy]);
            m |= a ? 4 : 0;
        }
        mask_out[i] = (uint8_t) m;
        tri += nv[i];
        vert += __builtin_popcount(m);
    }
    int total;
    block_exclusive(tri, &total, s_wave);
    if (threadIdx.x == 0) blk_tri[blockIdx.x] = total;
    block_exclusive(vert, &total, s_wave);
    if (threadIdx.x == 0) blk_vert[blockIdx.x] = total;
}

// TSDF gradient component along one axis at coordinate c of n: central difference / (2 cs), one-sided / cs on a face, no weight test
SOBFU_DEV float grad1(const float2* __restrict__ vol, size_t i, size_t stride, int c, int n, float cs) {
    const int lo = c > 0 ? c - 1 : c, hi = c + 1 < n ? c + 1 : c;
    if (hi == lo) return 0.f;
    const float fl = vol[i - (size_t) (c - lo) * stride].x, fh = vol[i + (size_t) (hi - c) * stride].x;
    return (fh - fl) / ((float) (hi - lo) * cs);
}

// pass 4: base[] of the voxels with a non-zero mask (scan of popcount(mask) within the workgroup + its offset) and their vertices
__global__ void __launch_bounds__(kBlock) indexed_vertices_kernel(const float2* __restrict__ vol, Dims d, const uint8_t* __restrict__ mask,
                                                                  const int* __restrict__ blk_vert_off, int* __restrict__ vbase, float csx,
                                                                  float csy, float csz, Pose pose, float4* __restrict__ out_v,
                                                                  float4* __restrict__ out_n, int max_vertices) {
    __shared__ int s_wave[kBlock / 64 + 1];
    const size_t N = (size_t) d.x * d.y * d.z, sy = (size_t) d.x, sz = (size_t) d.x * d.y;
    int run = blk_vert_off[blockIdx.x];
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const size_t i = (size_t) blockIdx.x * kChunk + (size_t) it * kBlock + threadIdx.x;
        const int m = i < N ? mask[i] : 0;
        int total;
        int pos = run + block_exclusive(__builtin_popcount(m), &total, s_wave);
        run += total;
        if (m == 0) continue;
        vbase[i] = pos;
        int x, y, z;
        coords32(i, d, x, y, z);
        const float fa = vol[i].x;
        const float ga[3] = {grad1(vol, i, 1, x, d.x, csx), grad1(vol, i, sy, y, d.y, csy), grad1(vol, i, sz, z, d.z, csz)};
        const float a[3] = {((float) x + 0.5f) * csx, ((float) y + 0.5f) * csy, ((float) z + 0.5f) * csz};  // get_node_coo
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            if (!((m >> axis) & 1)) continue;
            const size_t step = axis == 0 ? 1 : axis == 1 ? sy : sz;
            const int bx = x + (axis == 0), by = y + (axis == 1), bz = z + (axis == 2);
            const float b[3] = {((float) bx + 0.5f) * csx, ((float) by + 0.5f) * csy, ((float) bz + 0.5f) * csz};
            const float fb = vol[i + step].x;
            const float t  = (0.f - fa) / (fb - fa + 1e-15f);  // interp, from the owner corner up
            float p[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = a[k] + t * (b[k] - a[k]);
            const size_t j   = i + step;
            const float gb[3] = {grad1(vol, j, 1, bx, d.x, csx), grad1(vol, j, sy, by, d.y, csy), grad1(vol, j, sz, bz, d.z, csz)};
            float g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = ga[k] + t * (gb[k] - ga[k]);
            const float len2 = dot3(g, g[0], g[1], g[2]);
            float n[3] = {0.f, 0.f, 0.f};
            if (len2 > 0.f) {
                const float inv = 1.f / __builtin_sqrtf(len2);
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = g[k] * inv;
            }
            if (pos < max_vertices) {
                const float wx = dot3(pose.R + 0, p[0], p[1], p[2]) + pose.t[0];
                const float wy = dot3(pose.R + 3, p[0], p[1], p[2]) + pose.t[1];
                const float wz = dot3(pose.R + 6, p[0], p[1], p[2]) + pose.t[2];
                out_v[pos] = make_float4(wx, -wy, -wz, 1.f);
                const float nx = dot3(pose.R + 0, n[0], n[1], n[2]), ny = dot3(pose.R + 3, n[0], n[1], n[2]), nz = dot3(pose.R + 6, n[0], n[1], n[2]);
                out_n[pos] = make_float4(nx, -ny, -nz, 1.f);
            }
            ++pos;
        }
    }
}

// pass 5: the faces of every active cell; its first soup vertex = scan of nv within the workgroup + the workgroup's offset
__global__ void __launch_bounds__(kBlock) indexed_faces_kernel(const float2* __restrict__ vol, Dims d, const uint8_t* __restrict__ nv_in,
                                                               const uint8_t* __restrict__ mask, const int* __restrict__ vbase,
                                                               const int* __restrict__ blk_tri_off, int* __restrict__ faces, int max_triangles) {
    __shared__ int s_wave[kBlock / 64 + 1];
    const size_t N = (size_t) d.x * d.y * d.z, sy = (size_t) d.x, sz = (size_t) d.x * d.y;
    int run = blk_tri_off[blockIdx.x];
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const size_t i = (size_t) blockIdx.x * kChunk + (size_t) it * kBlock + threadIdx.x;
        const int nv = i < N ? nv_in[i] : 0;
        int total;
        const int first = run + block_exclusive(nv, &total, s_wave);
        run += total;
        if (nv == 0) continue;
        int x, y, z;
        coords32(i, d, x, y, z);
        float f[8];
        const uint64_t row = kTri[cube_index(vol, d, x, y, z, f)];
        for (int k = 0; k < nv; k += 3) {
            const int tri = (first + k) / 3;
            if (tri >= max_triangles) break;
            int idx[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = tri_edge(row, k + c), o = (int) ((kEdgeOwner >> (5 * e)) & 31u), axis = o >> 3;
                const size_t ow = i + (size_t) (o & 1) + (size_t) ((o >> 1) & 1) * sy + (size_t) ((o >> 2) & 1) * sz;
                idx[c] = vbase[ow] + __builtin_popcount(mask[ow] & ((1u << axis) - 1u));
            }
            faces[3 * (size_t) tri + 0] = idx[0];  // corners 1 and 2 swapped: counter-clockwise from outside
            faces[3 * (size_t) tri + 1] = idx[2];
            faces[3 * (size_t) tri + 2] = idx[1];
        }
    }
}

}  // namespace

extern "C" {

// Scratch of the two scan-based steps: one vertex-count byte per voxel + one int per 1024-voxel chunk (+ the total).
// A caller-provided workspace (sobfu_hip_mc_workspace_bytes) avoids the hipMalloc / hipFree pair -- two implicit device
// synchronisations -- per call; without one (NULL / too small) the scratch is allocated for the call.
static size_t nv_bytes(size_t N) { return (N + 255) / 256 * 256; }

size_t sobfu_hip_mc_workspace_bytes(int X, int Y, int Z) {
    if (X <= 0 || Y <= 0 || Z <= 0) return 0;
    const size_t N = (size_t) X * Y * Z;
    return nv_bytes(N) + ((N + kChunk - 1) / kChunk + 1) * sizeof(int);
}

int sobfu_hip_mc_occupied_voxels(void* stream, const float* d_vol, int X, int Y, int Z, int* d_occupied, int stride, int max_size,
                                 int* h_count, void* d_workspace, size_t workspace_bytes) {
    SOBFU_CHECK_ARGS(d_vol && d_occupied && h_count && X > 0 && Y > 0 && Z > 0 && max_size > 0 && stride >= max_size);
    const size_t N = (size_t) X * Y * Z;
    if (N > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;  // int32 voxel indices in `occupied`, like the reference
    hipStream_t st = (hipStream_t) stream;
    const int nb = (int) ((N + kChunk - 1) / kChunk);
    const bool own = !d_workspace || workspace_bytes < sobfu_hip_mc_workspace_bytes(X, Y, Z);
    uint8_t* d_nv = (uint8_t*) d_workspace;
    if (own) SOBFU_HIP_TRY(hipMalloc((void**) &d_nv, sobfu_hip_mc_workspace_bytes(X, Y, Z)));
    int* d_blk = (int*) (d_nv + nv_bytes(N));  // nb block counts + 1 total
    hipLaunchKernelGGL(classify_kernel, dim3(nb), dim3(kBlock), 0, st, (const float2*) d_vol, Dims{X, Y, Z}, d_nv, d_blk);
    int rc = (int) hipGetLastError();
    if (rc == 0) rc = scan_in_place_sums(d_blk, nb, d_blk + nb, st);
    if (rc == 0) {
        hipLaunchKernelGGL(compact_kernel, dim3(nb), dim3(kBlock), 0, st, d_nv, N, d_blk, d_occupied, d_occupied + stride, max_size);
        rc = (int) hipGetLastError();
    }
    int found = 0;
    if (rc == 0) rc = (int) hipMemcpyAsync(&found, d_blk + nb, sizeof(int), hipMemcpyDeviceToHost, st);
    if (rc == 0) rc = (int) hipStreamSynchronize(st);
    if (own) (void) hipFree(d_nv);
    if (rc == 0) *h_count = found < max_size ? found : max_size;
    return rc;
}

int sobfu_hip_mc_offsets(void* stream, int* d_occupied, int stride, int count, int* h_total_vertices, void* d_workspace,
                         size_t workspace_bytes) {
    SOBFU_CHECK_ARGS(d_occupied && h_total_vertices && count >= 0 && stride >= count);
    if (count == 0) { *h_total_vertices = 0; return 0; }
    hipStream_t st = (hipStream_t) stream;
    const int nb = (count + kChunk - 1) / kChunk;
    const bool own = !d_workspace || workspace_bytes < (size_t) (nb + 1) * sizeof(int);
    int* d_blk = (int*) d_workspace;
    if (own) SOBFU_HIP_TRY(hipMalloc((void**) &d_blk, (size_t) (nb + 1) * sizeof(int)));
    hipLaunchKernelGGL(chunk_sum_kernel, dim3(nb), dim3(kBlock), 0, st, d_occupied + stride, count, d_blk);
    int rc = (int) hipGetLastError();
    if (rc == 0) rc = scan_in_place_sums(d_blk, nb, d_blk + nb, st);
    if (rc == 0) {
        hipLaunchKernelGGL(chunk_scan_kernel, dim3(nb), dim3(kBlock), 0, st, d_occupied + stride, count, d_blk, d_occupied + 2 * (size_t) stride);
        rc = (int) hipGetLastError();
    }
    if (rc == 0) rc = (int) hipMemcpyAsync(h_total_vertices, d_blk + nb, sizeof(int), hipMemcpyDeviceToHost, st);
    if (rc == 0) rc = (int) hipStreamSynchronize(st);
    if (own) (void) hipFree(d_blk);
    return rc;
}

int sobfu_hip_mc_generate_triangles(void* stream, const float* d_vol, int X, int Y, int Z, const int* d_occupied, int stride, int count,
                                    float size_x, float size_y, float size_z, const float R[9], const float t[3], float* d_vertices,
                                    float* d_normals, int max_vertices) {
    SOBFU_CHECK_ARGS(d_vol && d_occupied && R && t && d_vertices && d_normals && X > 0 && Y > 0 && Z > 0 && count >= 0 && stride >= count &&
                     max_vertices >= 0);
    if (count == 0) return 0;
    Pose p;
    for (int i = 0; i < 9; ++i) p.R[i] = R[i];
    for (int i = 0; i < 3; ++i) p.t[i] = t[i];
    hipLaunchKernelGGL(triangles_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t) stream, (const float2*) d_vol, Dims{X, Y, Z},
                       d_occupied, d_occupied + 2 * (size_t) stride, count, size_x / X, size_y / Y, size_z / Z, p, (float4*) d_vertices,
                       (float4*) d_normals, max_vertices);
    return (int) hipGetLastError();
}

// Indexed path.  Workspace: nv and mask bytes, base ints per voxel (6 B), then three per-workgroup int arrays (active cells, soup vertices,
// welded vertices: scanned in place) and their three totals.  The count call leaves all of it for the generate call.
struct IndexedLayout {
    size_t N, nb;
    uint8_t *nv, *mask;
    int *base, *blk_active, *blk_tri, *blk_vert, *totals;
};
static size_t indexed_bytes(size_t N) {
    const size_t nb = (N + kChunk - 1) / kChunk;
    return 6 * nv_bytes(N) + (3 * nb + 4) * sizeof(int);
}
static IndexedLayout indexed_layout(void* ws, size_t N) {
    IndexedLayout L;
    L.N = N;
    L.nb = (N + kChunk - 1) / kChunk;
    L.nv = (uint8_t*) ws;
    L.mask = L.nv + nv_bytes(N);
    L.base = (int*) (L.mask + nv_bytes(N));
    L.blk_active = (int*) ((uint8_t*) L.base + 4 * nv_bytes(N));
    L.blk_tri = L.blk_active + L.nb;
    L.blk_vert = L.blk_tri + L.nb;
    L.totals = L.blk_vert + L.nb;  // active cells, soup vertices, welded vertices
    return L;
}

size_t sobfu_hip_mc_indexed_workspace_bytes(int X, int Y, int Z) {
    if (X <= 0 || Y <= 0 || Z <= 0) return 0;
    return indexed_bytes((size_t) X * Y * Z);
}

int sobfu_hip_mc_indexed_count(void* stream, const float* d_vol, int X, int Y, int Z, void* d_workspace, size_t workspace_bytes,
                               int* h_active_cells, int* h_vertices, int* h_triangles) {
    SOBFU_CHECK_ARGS(d_vol && d_workspace && h_active_cells && h_vertices && h_triangles && X > 0 && Y > 0 && Z > 0);
    const size_t N = (size_t) X * Y * Z;
    if (N > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    SOBFU_CHECK_ARGS(workspace_bytes >= indexed_bytes(N));
    hipStream_t st = (hipStream_t) stream;
    const IndexedLayout L = indexed_layout(d_workspace, N);
    const int nb = (int) L.nb;
    const Dims d{X, Y, Z};
    hipLaunchKernelGGL(classify_kernel, dim3(nb), dim3(kBlock), 0, st, (const float2*) d_vol, d, L.nv, L.blk_active);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(edge_mask_kernel, dim3(nb), dim3(kBlock), 0, st, (const float2*) d_vol, d, (const uint8_t*) L.nv, L.mask, L.blk_tri,
                       L.blk_vert);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scan_blocks3_kernel, dim3(3), dim3(1024), 0, st, L.blk_active, nb, L.totals);  // blk_active, blk_tri, blk_vert
    SOBFU_HIP_TRY(hipGetLastError());
    int h[3];
    SOBFU_HIP_TRY(hipMemcpyAsync(h, L.totals, sizeof h, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    *h_active_cells = h[0];
    *h_vertices     = h[2];
    *h_triangles    = h[1] / 3;
    return 0;
}

int sobfu_hip_mc_indexed_generate(void* stream, const float* d_vol, int X, int Y, int Z, float size_x, float size_y, float size_z,
                                  const float R[9], const float t[3], void* d_workspace, size_t workspace_bytes, float* d_vertices,
                                  float* d_normals, int max_vertices, int* d_faces, int max_triangles) {
    SOBFU_CHECK_ARGS(d_vol && R && t && d_workspace && d_vertices && d_normals && d_faces && X > 0 && Y > 0 && Z > 0 && max_vertices >= 0 &&
                     max_triangles >= 0);
    const size_t N = (size_t) X * Y * Z;
    if (N > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    SOBFU_CHECK_ARGS(workspace_bytes >= indexed_bytes(N));
    hipStream_t st = (hipStream_t) stream;
    const IndexedLayout L = indexed_layout(d_workspace, N);
    int h[3];  // the count call's totals: never truncate (a dropped face or vertex would leave dangling indices)
    SOBFU_HIP_TRY(hipMemcpyAsync(h, L.totals, sizeof h, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    if (h[2] > max_vertices || h[1] / 3 > max_triangles) return SOBFU_E_BADARG;
    if (h[1] == 0) return 0;
    Pose p;
    for (int i = 0; i < 9; ++i) p.R[i] = R[i];
    for (int i = 0; i < 3; ++i) p.t[i] = t[i];
    const int nb = (int) L.nb;
    const Dims d{X, Y, Z};
    hipLaunchKernelGGL(indexed_vertices_kernel, dim3(nb), dim3(kBlock), 0, st, (const float2*) d_vol, d, (const uint8_t*) L.mask,
                       (const int*) L.blk_vert, L.base, size_x / X, size_y / Y, size_z / Z, p, (float4*) d_vertices, (float4*) d_normals,
                       max_vertices);
    SOBFU_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(indexed_faces_kernel, dim3(nb), dim3(kBlock), 0, st, (const float2*) d_vol, d, (const uint8_t*) L.nv,
                       (const uint8_t*) L.mask, (const int*) L.base, (const int*) L.blk_tri, d_faces, max_triangles);
    return (int) hipGetLastError();
}

}  // extern "C"
