// The mesh side's home: what the units that work on "an indexed triangle mesh plus its uniform grid" share -- mesh_distance_kernels.hip
// (builds the grid, queries it with points), mesh_ray_kernels.hip (rays), mesh_voxel_kernels.hip (rows, bricks), mesh_winding_kernels.hip
// (rows and points with winding numbers), mesh_align_kernels.hip.
// The grid's workspace as the kernels see it, the mesh record and its corner loads, a triangle's cell range, the LDS staging loads of the
// 256-lane brute-force loops, the margin, the mode, and the one check of the nine arguments every mesh entry point of the C ABI starts with.  The
// plan (origin, cell edge, dims) is sobfu_mesh_grid.hpp's.  What only the rows along +x share -- the crossing walk, the voxel centres, the
// sign bits -- is sobfu_mesh_rows.hpp's, on top of this.  Internal linkage, no kernels: the scan is compiled where it is launched.
#pragma once

#include "sobfu_device.hpp"
#include "sobfu_host.hpp"
#include "sobfu_mesh_distance.hpp"
#include "sobfu_mesh_grid.hpp"
#include "sobfu_scan_layout.hpp"

namespace sobfu_hip {
namespace {

constexpr float kMeshMargin = 1e-4f;  // bounds the fp32 error of one point-triangle distance, in units of L (mesh_distance_kernels.hip)
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

struct Mesh {
    const float4* verts;
    const int* faces;
    int n_triangles;
};
struct Corners { float4 a, b, c; };
// the vertex indices of triangle t, and its corners (from the indices where the caller has to look at those first)
SOBFU_DEV int3 face_of(const Mesh& m, int t) { return make_int3(m.faces[3 * (size_t) t], m.faces[3 * (size_t) t + 1], m.faces[3 * (size_t) t + 2]); }
SOBFU_DEV Corners corners_of(const Mesh& m, const int3& f) { return Corners{m.verts[f.x], m.verts[f.y], m.verts[f.z]}; }
SOBFU_DEV Corners corners_of(const Mesh& m, int t) { return corners_of(m, face_of(m, t)); }

// the inclusive range of cells a triangle's box overlaps: the build references the triangle from exactly these, and whoever has to know
// where a reference came from (the x-minimum of the row counts and of the point test) asks here; brick_kernel writes the same lines out
struct CellRange { int x0, x1, y0, y1, z0, z1; };
SOBFU_DEV CellRange cells_of(const Grid& g, const Corners& t) {
    const float4 &a = t.a, &b = t.b, &c = t.c;
    return CellRange{cell_of(fminf(fminf(a.x, b.x), c.x), g.ox, g.h, g.dx), cell_of(fmaxf(fmaxf(a.x, b.x), c.x), g.ox, g.h, g.dx),
                     cell_of(fminf(fminf(a.y, b.y), c.y), g.oy, g.h, g.dy), cell_of(fmaxf(fmaxf(a.y, b.y), c.y), g.oy, g.h, g.dy),
                     cell_of(fminf(fminf(a.z, b.z), c.z), g.oz, g.h, g.dz), cell_of(fmaxf(fmaxf(a.z, b.z), c.z), g.oz, g.h, g.dz)};
}

// the loads of one staging pass of a brute-force loop whose workgroup stages one triangle per lane: lane s takes triangle t0 + s, if
// there is one, into slot s.  The barriers before and after are the kernel's.  (brick_kernel stages two per lane, in a loop of its own.)
SOBFU_DEV void stage_triangles(const Mesh& m, int t0, float4* sa, float4* sb, float4* sc) {
    const int s = threadIdx.x;
    if (t0 + s < m.n_triangles) {
        const Corners t = corners_of(m, t0 + s);
        sa[s] = t.a, sb[s] = t.b, sc[s] = t.c;
    }
}

bool mode_ok(int mode) { return mode >= SOBFU_MESH_DISTANCE_AUTO && mode <= SOBFU_MESH_DISTANCE_BRUTE; }
int is_brute(int mode, int n_triangles) { return mode == SOBFU_MESH_DISTANCE_BRUTE || (mode == SOBFU_MESH_DISTANCE_AUTO && n_triangles <= kMeshGridTinyMesh); }

// The nine arguments every mesh entry point of the C ABI starts with (and max_refs, 0 for all but the build), checked and turned into
// what the kernels take.  ws_bytes and n_vertices are kept for the unit that passes the target on through the C ABI (mesh alignment).
struct MeshTarget {
    Grid grid;
    Mesh mesh;
    float box_l;  // the largest coordinate magnitude of the grid's box
    size_t ws_bytes;
    int n_vertices;
};
bool mesh_target(void* ws, size_t ws_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, const float origin[3],
                 float h, const int dims[3], int max_refs, MeshTarget* out) {
    const bool grid_ok = ws && aligned(ws, 0, 16) && max_refs >= 0 && mesh_grid_plan_ok(origin, h, dims) && ws_bytes >= grid_ints(dims, max_refs) * sizeof(int);
    const bool mesh_ok = n_vertices >= 0 && n_triangles >= 0 && (n_triangles == 0 || (d_vertices && d_faces)) && aligned(d_vertices, 0, 16) && aligned(d_faces, 0, 4);
    if (grid_ok && mesh_ok)
        *out = MeshTarget{grid_of(ws, origin, h, dims, max_refs), Mesh{(const float4*) d_vertices, d_faces, n_triangles}, grid_box_l(origin, h, dims), ws_bytes, n_vertices};
    return grid_ok && mesh_ok;
}

}  // namespace
}  // namespace sobfu_hip
