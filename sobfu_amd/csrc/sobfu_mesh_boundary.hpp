// The boundary chain of an indexed triangle mesh: for every undirected edge {u < v} the coefficient
// k = (#triangles that run u -> v) - (#triangles that run v -> u); the edges with k != 0, sorted by (u, v).  An interior edge of a
// consistently oriented mesh has k = 0 and vanishes; a triangle listed twice gives |k| = 2, two neighbours with opposite orientation
// |k| = 2 on the edge they share, and a closed mesh nothing.  64-bit edge keys are sorted -- no hashing -- so the list is deterministic.
// An edge from a vertex to itself has no direction and is skipped.  Host-only, no HIP: sobfu_hip_mesh_boundary and the CPU tests call it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace sobfu_hip {

struct BoundaryEdge {
    int u, v, k;
};

// false: an index outside [0, n_vertices)
inline bool mesh_boundary(const int* faces, int n_triangles, int n_vertices, std::vector<BoundaryEdge>* out) {
    std::vector<uint64_t> keys;  // (u << 33) | (v << 1) | (1 where the triangle runs v -> u)
    keys.reserve(3 * (size_t) (n_triangles > 0 ? n_triangles : 0));
    for (int t = 0; t < n_triangles; ++t)
        for (int e = 0; e < 3; ++e) {
            const int p = faces[3 * (size_t) t + e], q = faces[3 * (size_t) t + (e + 1) % 3];
            if (p < 0 || q < 0 || p >= n_vertices || q >= n_vertices) return false;
            if (p == q) continue;
            const uint64_t lo = (uint64_t) (p < q ? p : q), hi = (uint64_t) (p < q ? q : p);
            keys.push_back((lo << 33) | (hi << 1) | (p < q ? 0u : 1u));
        }
    std::sort(keys.begin(), keys.end());
    out->clear();
    for (size_t i = 0; i < keys.size();) {
        const uint64_t edge = keys[i] >> 1;
        long long k = 0;
        for (; i < keys.size() && (keys[i] >> 1) == edge; ++i) k += (keys[i] & 1u) ? -1 : 1;
        if (k != 0) out->push_back(BoundaryEdge{(int) (edge >> 32), (int) (edge & 0xffffffffu), (int) k});
    }
    return true;
}

}  // namespace sobfu_hip
