// The plan of the uniform grid over a triangle mesh (mesh_distance_kernels.hip): bounding box + triangle count (+ a cell edge given by the
// caller) -> origin, cell edge h and dims.  Host-only, no HIP: sobfu_hip_mesh_grid_plan and the CPU tests call it.
//
//   cells    cubic, edge h, the first at the box's lower corner
//   default  cells along the longest extent = clamp(ceil(sqrt(n_triangles) / kMeshGridDivisor), 1, kMeshGridMaxDim); h = that extent / cells,
//            rounded up to a float that still covers it
//   given    h = the caller's cell, enlarged to longest extent / kMeshGridMaxDim where it would give more cells than that
//   others   every axis gets ceil(extent / h) cells, at least 1; a zero extent gives one cell, a point-like box one cell of edge 1 (or the
//            caller's cell)
// dims[i] * h >= extent[i] on every axis: the box is always covered.
#pragma once

#include <cmath>

namespace sobfu_hip {

constexpr int kMeshGridMaxDim   = 128;
constexpr int kMeshGridDivisor  = 4;   // cells along the longest extent = sqrt(n_triangles) / this (profiles/mesh_distance.md)
constexpr int kMeshGridRingCap  = 8;   // shells a query visits before the point goes to the brute-force pass
constexpr int kMeshGridTinyMesh = 64;  // mode auto: at most this many triangles are not worth a grid walk

struct MeshGridPlan {
    float origin[3];
    float h;
    int dims[3];
};

// false: a non-finite or inverted box, a negative count, a negative or non-finite cell
inline bool mesh_grid_plan(const float bbox[6], int n_triangles, float cell, MeshGridPlan* out) {
    if (n_triangles < 0 || !std::isfinite(cell) || cell < 0.f) return false;
    double ext[3], longest = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(bbox[i]) || !std::isfinite(bbox[3 + i]) || bbox[3 + i] < bbox[i]) return false;
        ext[i] = (double) bbox[3 + i] - (double) bbox[i];
        if (!std::isfinite((float) ext[i])) return false;
        longest = ext[i] > longest ? ext[i] : longest;
        out->origin[i] = bbox[i];
    }
    float h;
    if (cell > 0.f) {
        h = cell;
        if ((double) h * kMeshGridMaxDim < longest) h = (float) (longest / kMeshGridMaxDim);
        while ((double) h * kMeshGridMaxDim < longest) h = std::nextafterf(h, INFINITY);
    } else if (longest == 0.0) {
        h = 1.f;
    } else {
        int cells = (int) std::ceil(std::sqrt((double) n_triangles) / kMeshGridDivisor);
        cells     = cells < 1 ? 1 : cells > kMeshGridMaxDim ? kMeshGridMaxDim : cells;
        h         = (float) (longest / cells);
        while ((double) h * cells < longest) h = std::nextafterf(h, INFINITY);
        if (!(h > 0.f)) h = std::nextafterf(0.f, 1.f);
    }
    if (!std::isfinite(h) || !(h > 0.f)) return false;
    out->h = h;
    for (int i = 0; i < 3; ++i) {
        double c = std::ceil(ext[i] / (double) h);
        out->dims[i] = c < 1.0 ? 1 : c > kMeshGridMaxDim ? kMeshGridMaxDim : (int) c;
    }
    return true;
}

inline bool mesh_grid_plan_ok(const float origin[3], float h, const int dims[3]) {
    if (!origin || !dims || !std::isfinite(h) || !(h > 0.f)) return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(origin[i]) || dims[i] < 1 || dims[i] > kMeshGridMaxDim) return false;
    return true;
}

}  // namespace sobfu_hip
