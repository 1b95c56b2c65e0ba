// Rows along +x through a mesh's grid: what mesh_voxel_kernels.hip (parities) and mesh_winding_kernels.hip (signed counts) share beyond
// sobfu_mesh.hpp -- the voxel centres, where a crossing lands in a row, the walk of a row's cell column in its two forms, the format of
// the sign bits that brick_kernel reads, and the check of the volume-side arguments of the two voxelise entry points.  The crossing rule
// itself is sobfu_mesh_parity.hpp's.  Internal linkage, no kernels, like sobfu_mesh.hpp.
//
//   column   a row is the line through (., py, pz) along +x.  A crossing triangle's box contains (py, pz) -- the fp32 translation of the
//            rule keeps signs -- so it is referenced from the row's one cell column (cell_of(py), cell_of(pz)), whose cells cx = 0 ..
//            dx - 1 hold one contiguous range of references.  A triangle referenced from several cells of the column counts only in
//            the first cell in x of its cell range (cells_of, which the build bins by).  The crossing rule is exact, so what is counted
//            depends neither on the cells, nor on the order of the references, nor on grid versus brute force (every triangle once).
//   bits     voxel i of row (j, k) is inside iff bit i & 31 of word (j + Y k) words_per_row(X) + (i >> 5) is set; X <= kMaxX
#pragma once

#include "sobfu_mesh.hpp"
#include "sobfu_mesh_parity.hpp"

namespace sobfu_hip {

// mesh_voxel_kernels.hip: the distance pass alone, over sign bits that a row kernel of either unit wrote into d_bits.  The arguments
// are sobfu_hip_mesh_voxelise's and have been checked by the caller (rows_volume_ok).
int mesh_voxel_bricks(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                      const float origin[3], float h, const int dims[3], float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc,
                      float eta, int mode, void* d_bits, int* d_open_rows, void* stream);

namespace {

constexpr int kMaxX  = 512;  // the longest row a wave takes
constexpr int kBrick = 8;    // mesh_voxel_bricks: one workgroup per 8 x 8 x 8 voxels, one brick of z per blockIdx.z

SOBFU_DEV float centre(int i, float vs) { return (float) i * vs + vs / 2.f; }

// the first i in [0, n] whose centre is not below X (n: none is)
SOBFU_DEV int first_not_below(double X, float vs, int n) {
    const double e = ceil((X - (double) (vs / 2.f)) / (double) vs);
    int i = (int) fmax(fmin(e, (double) n), 0.0);
    while (i > 0 && (double) centre(i - 1, vs) >= X) --i;
    while (i < n && (double) centre(i, vs) < X) ++i;
    return i;
}

SOBFU_DEV SignedCrossing cross_triangle(const Corners& t, float py, float pz) { return signed_row_crossing(p3(t.a), p3(t.b), p3(t.c), py, pz); }

// the cell c in [c0, c1] of a row of cells (start: that row's entries) whose references hold position k: the largest c with start[c] <= k
SOBFU_DEV int cell_of_reference(const int* __restrict__ start, int c0, int c1, int k) {
    int lo = c0, hi = c1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the entries of the cell column of the row (., py, pz)
SOBFU_DEV const int* column_of(const Grid& g, float py, float pz) {
    return g.start + g.dx * (cell_of(py, g.oy, g.h, g.dy) + g.dy * cell_of(pz, g.oz, g.h, g.dz));
}

// The walk, a wave to a row: the lanes stride over the column's references (brute: over all triangles) and find a reference's cell by
// bisection; crossed(c) runs once for every triangle the row crosses, in no particular order.
template <class Crossed> SOBFU_DEV void walk_row_wave(const Grid& g, const Mesh& m, int brute, float py, float pz, int lane, Crossed crossed) {
    if (brute) {
        for (int t = lane; t < m.n_triangles; t += 64) {
            const SignedCrossing c = cross_triangle(corners_of(m, t), py, pz);
            if (c.sign != 0) crossed(c);
        }
    } else {
        const int* start = column_of(g, py, pz);
        const int k1     = start[g.dx];
        for (int k = start[0] + lane; k < k1; k += 64) {
            const Corners t        = corners_of(m, g.refs[k]);
            const SignedCrossing c = cross_triangle(t, py, pz);
            if (c.sign != 0 && cells_of(g, t).x0 == cell_of_reference(start, 0, g.dx - 1, k)) crossed(c);
        }
    }
}

// The walk, a lane to a row: the column's cells in order, so a reference's cell is known.  Every loop stays rolled: left to the unroller
// the point kernels took over 300 VGPRs and mesh_winding_kernel spilled two (tests/test_no_scratch.py, profiles/mesh_rows_home.md).
template <class Crossed> SOBFU_DEV void walk_row_lane(const Grid& g, const Mesh& m, int brute, float py, float pz, Crossed crossed) {
    if (brute) {
#pragma unroll 1
        for (int t = 0; t < m.n_triangles; ++t) {
            const SignedCrossing c = cross_triangle(corners_of(m, t), py, pz);
            if (c.sign != 0) crossed(c);
        }
    } else {
        const int* start = column_of(g, py, pz);
#pragma unroll 1
        for (int cx = 0; cx < g.dx; ++cx)
#pragma unroll 1
            for (int k = start[cx]; k < start[cx + 1]; ++k) {
                const Corners t        = corners_of(m, g.refs[k]);
                const SignedCrossing c = cross_triangle(t, py, pz);
                if (c.sign != 0 && cells_of(g, t).x0 == cx) crossed(c);
            }
    }
}

int words_per_row(int X) { return (X + 31) / 32; }
size_t bits_bytes(int X, int Y, int Z) { return ((size_t) Y * Z * words_per_row(X) * sizeof(unsigned) + 15) / 16 * 16; }
bool rows_ok(int X, int Y, int Z) { return X >= 1 && X <= kMaxX && Y >= 1 && Z >= 1; }

// The volume-side arguments the two voxelise entry points share; workspace_needed is the entry point's own, and so is its limit on the
// number of rows or voxels, which it checks beside this.
bool rows_volume_ok(const float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc, float eta, int mode, const void* d_workspace,
                    size_t workspace_bytes, size_t workspace_needed, const int* d_open_rows) {
    return d_vol && aligned(d_vol, 0, 8) && rows_ok(X, Y, Z) && volume_ok(X, Y, Z, kGridZ * kBrick) && voxel_size && positive_finite(voxel_size[0]) &&
           positive_finite(voxel_size[1]) && positive_finite(voxel_size[2]) && positive_finite(trunc) && std::isfinite(eta) && mode_ok(mode) && d_workspace &&
           aligned(d_workspace, 0, 16) && workspace_bytes >= workspace_needed && d_open_rows && aligned(d_open_rows, 0, 4);
}

}  // namespace
}  // namespace sobfu_hip
