// The workspace of the uniform triangle grid as the kernels see it: mesh_distance_kernels.hip builds it and queries it with points,
// mesh_ray_kernels.hip only reads it, with rays.  The plan (origin, cell edge, dims) is sobfu_mesh_grid.hpp's.  Internal linkage, like
// sobfu_scan.hpp.
#pragma once

#include "sobfu_host.hpp"
#include "sobfu_mesh_distance.hpp"
#include "sobfu_mesh_grid.hpp"
#include "sobfu_scan.hpp"

namespace sobfu_hip {
namespace {

// workspace header (ints): 0 bad-input flag, 1 unresolved points of the last query, 2-3 references counted (64 bit), 5 built marker
constexpr int kHdrInts = 16, kHdrBad = 0, kHdrUnresolved = 1, kHdrRefs = 2, kHdrBuilt = 5;

struct Grid {
    int* hdr;
    int* count;  // ncells + 1: the build's cursors (all 0 afterwards)
    int* start;  // ncells + 1: exclusive scan of the counts; start[ncells] = the number of references
    int* blk;    // the scan's per-block sums
    int* refs;
    float ox, oy, oz, h;
    int dx, dy, dz;
    int max_refs;
};

size_t ncells_of(const int dims[3]) { return (size_t) dims[0] * dims[1] * dims[2]; }
size_t grid_ints(const int dims[3], int max_refs) {
    const size_t nc = ncells_of(dims) + 1, nb = (nc + kChunk - 1) / kChunk;
    return kHdrInts + 2 * nc + nb + 1 + (size_t) max_refs;
}
Grid grid_of(void* ws, const float origin[3], float h, const int dims[3], int max_refs) {
    const size_t nc = ncells_of(dims) + 1, nb = (nc + kChunk - 1) / kChunk;
    Grid g;
    g.hdr = (int*) ws, g.count = g.hdr + kHdrInts, g.start = g.count + nc, g.blk = g.start + nc, g.refs = g.blk + nb + 1;
    g.ox = origin[0], g.oy = origin[1], g.oz = origin[2], g.h = h;
    g.dx = dims[0], g.dy = dims[1], g.dz = dims[2], g.max_refs = max_refs;
    return g;
}
// the largest coordinate magnitude of the grid's box
float grid_box_l(const float origin[3], float h, const int dims[3]) {
    float l = 0.f;
    for (int i = 0; i < 3; ++i) l = std::fmax(l, std::fmax(std::fabs(origin[i]), std::fabs(origin[i] + (float) dims[i] * h)));
    return l;
}

// the cell of coordinate x along an axis of `dim` cells from o, clamped into the grid (a NaN lands in cell 0)
SOBFU_DEV int cell_of(float x, float o, float h, int dim) { return (int) fminf(fmaxf(floorf((x - o) / h), 0.f), (float) (dim - 1)); }
SOBFU_DEV P3 p3(const float4& v) { return P3{v.x, v.y, v.z}; }
SOBFU_DEV bool finite3(const float4& v) { return fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY && fabsf(v.z) < INFINITY; }

bool grid_args_ok(const void* ws, size_t ws_bytes, const float origin[3], float h, const int dims[3], int max_refs) {
    return ws && aligned(ws, 0, 16) && max_refs >= 0 && mesh_grid_plan_ok(origin, h, dims) && ws_bytes >= grid_ints(dims, max_refs) * sizeof(int);
}
bool mesh_args_ok(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles) {
    return n_vertices >= 0 && n_triangles >= 0 && (n_triangles == 0 || (d_vertices && d_faces)) && aligned(d_vertices, 0, 16) &&
           aligned(d_faces, 0, 4);
}

}  // namespace
}  // namespace sobfu_hip
