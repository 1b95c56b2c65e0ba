// Area-weighted samples of a triangle mesh: the rule of mesh_sample_kernels.hip, shared by its count and generate kernels
// and taken by a host compiler too.  tests/mesh_sample_reference.py restates it operation by operation (every TU is built with
// -ffp-contract=off; there is no fused operation here): the order of the floating-point operations below is part of the contract.  Plain
// floats, doubles and integers, no HIP types.  The draws are Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32) (sobfu_random.hpp).
//
//   area     of the triangle a, b, c (fp32 corners), in fp64: e1 = (double) b - (double) a, e2 = (double) c - (double) a,
//            n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x), area = 0.5 sqrt((n.x n.x + n.y n.y) + n.z n.z)
//   count    of triangle t at `density` samples per unit area: x = area density, fl = floor(x), frac = x - fl,
//            u = (double) uniform_variate(w[0]) of the draw with counter (t, 0, 0, 0); count = fl + (u < frac ? 1 : 0).  Its expectation is
//            x, and it is never more than one sample from it; a triangle without area gets 0.  (x beyond 2^62 counts as 2^62.)
//   sample   k of triangle t: the draw with counter (t, k, 0, 1); m1 = w[0] >> 8, m2 = w[1] >> 8; when m1 + m2 > 2^24 both are reflected,
//            m = 2^24 - m -- on the integers, so the fold is exact and r1 + r2 <= 1 holds exactly; r1 = (float) m1 2^-24, r2 likewise;
//            ab = b - a, ac = c - a in fp32; p = (a + ab r1) + ac r2 (md_along twice).  (r1, r2) are the weights of b and c.
#pragma once

#include <cmath>
#include <cstdint>

#include "sobfu_mesh_distance.hpp"
#include "sobfu_random.hpp"

namespace sobfu_hip {

constexpr uint32_t kSampleCountStream = 0, kSamplePointStream = 1;  // the counter's last word

struct MeshSample {
    P3 p;
    float r1, r2;
};

SOBFU_MD_FN double triangle_area(const P3& a, const P3& b, const P3& c) {
    const double e1x = (double) b.x - (double) a.x, e1y = (double) b.y - (double) a.y, e1z = (double) b.z - (double) a.z;
    const double e2x = (double) c.x - (double) a.x, e2y = (double) c.y - (double) a.y, e2z = (double) c.z - (double) a.z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    return 0.5 * __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
}

// area and density finite and >= 0
SOBFU_MD_FN long long sample_count(double area, double density, uint64_t seed, int t) {
    const double x = area * density;
    if (!(x < 0x1p62)) return 1LL << 62;  // also an overflow to +Inf
    const double fl = __builtin_floor(x), frac = x - fl;
    const Philox w = philox4x32_10((uint32_t) t, 0u, 0u, kSampleCountStream, (uint32_t) (seed & 0xffffffffu), (uint32_t) (seed >> 32));
    const double u = (double) uniform_variate(w.w[0]);
    return (long long) fl + (u < frac ? 1 : 0);
}

SOBFU_MD_FN MeshSample sample_point(const P3& a, const P3& b, const P3& c, uint64_t seed, int t, int k) {
    const Philox w = philox4x32_10((uint32_t) t, (uint32_t) k, 0u, kSamplePointStream, (uint32_t) (seed & 0xffffffffu), (uint32_t) (seed >> 32));
    uint32_t m1 = w.w[0] >> 8, m2 = w.w[1] >> 8;
    if (m1 + m2 > (1u << 24)) m1 = (1u << 24) - m1, m2 = (1u << 24) - m2;
    const float r1 = (float) m1 * 0x1p-24f, r2 = (float) m2 * 0x1p-24f;
    const P3 ab = md_sub(b, a), ac = md_sub(c, a);
    return MeshSample{md_along(md_along(a, ab, r1), ac, r2), r1, r2};
}

}  // namespace sobfu_hip
