// The closest point of a triangle to a point, in fp32: the rule of mesh_distance_kernels.hip, shared by its grid and brute-force kernels.
// tests/mesh_distance_reference.py restates it operation by operation (every TU is built with -ffp-contract=off; there is no fused
// operation here): the order of the floating-point operations below is part of the contract.  Plain floats, no HIP types: a host
// compiler takes this header too.
//
//   dot(u, v)   (u.x v.x + u.y v.y) + u.z v.z
//   setup       ab = b - a, ac = c - a, bc = c - b, ap = p - a, bp = p - b, cp = p - c; d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp,
//               d5 = ab.cp, d6 = ac.cp; vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4; sum = (va + vb) + vc
//               (in exact arithmetic sum = |ab x ac|^2, whatever p is)
//   regions     Voronoi regions in Ericson's order (Real-Time Collision Detection 5.1.5), the first that holds:
//                 vertex a   d1 <= 0 and d2 <= 0                          q = a
//                 vertex b   d3 >= 0 and d4 <= d3                         q = b
//                 edge ab    vc <= 0, d1 >= 0, d3 <= 0                    q = a + ab (d1 / (d1 - d3))
//                 vertex c   d6 >= 0 and d5 <= d6                         q = c
//                 edge ac    vb <= 0, d2 >= 0, d6 <= 0                    q = a + ac (d2 / (d2 - d6))
//                 edge bc    va <= 0, e1 = d4 - d3 >= 0, e2 = d5 - d6 >= 0  q = b + bc (e1 / (e1 + e2))
//                 interior                                                q = (a + ab (vb / sum)) + ac (vc / sum)
//               an edge parameter whose denominator is not > 0 is 0
//   degenerate  when sum is not > kMeshDegenerate E2 m, with E2 = max(ab.ab, ac.ac, bc.bc) and m = max(ap.ap, bp.bp, cp.cp) -- two or three
//               equal corners, collinear corners, or a sliver whose area is within the rounding noise of va, vb, vc (about 2^-24 |ab| |ac| m:
//               below the threshold their signs and ratios mean nothing) -- the regions are not consulted: the answer is the nearest of the
//               segments ab, bc, ac in that order (a later one wins only when strictly nearer), each q = u + e clamp((e . (p - u)) / (e . e),
//               0, 1) from its first corner u, a zero-length segment (e . e not > 0) being that corner.  A triangle that falls under the
//               rule is lower than 2^-8 of the point's distance to its farthest corner, so its edges stand in for it within
//               that height.  No division has a zero denominator: nothing here makes a NaN or Inf from finite input whose squares do not
//               overflow.
//   distance    d2 = dot(p - q, p - q)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define SOBFU_MD_FN __host__ __device__ __forceinline__
#else
#define SOBFU_MD_FN inline
#endif

namespace sobfu_hip {

constexpr float kMeshDegenerate = 1.52587890625e-05f;  // 2^-16 = 256 * 2^-24

struct P3 {
    float x, y, z;
};
struct Closest {
    P3 q;
    float d2;
};

SOBFU_MD_FN P3 md_sub(const P3& u, const P3& v) { return P3{u.x - v.x, u.y - v.y, u.z - v.z}; }
SOBFU_MD_FN float md_dot(const P3& u, const P3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
SOBFU_MD_FN P3 md_along(const P3& u, const P3& e, float s) { return P3{u.x + e.x * s, u.y + e.y * s, u.z + e.z * s}; }
SOBFU_MD_FN float md_ratio(float num, float den) { return den > 0.f ? num / den : 0.f; }
SOBFU_MD_FN Closest md_at(const P3& p, const P3& q) {
    const P3 d = md_sub(p, q);
    return Closest{q, md_dot(d, d)};
}

// the segment from u along e
SOBFU_MD_FN Closest closest_on_segment(const P3& p, const P3& u, const P3& e) {
    const float l2 = md_dot(e, e), t = md_dot(e, md_sub(p, u));
    const float s = l2 > 0.f ? fminf(fmaxf(t / l2, 0.f), 1.f) : 0.f;
    return md_at(p, md_along(u, e, s));
}

SOBFU_MD_FN Closest closest_on_triangle(const P3& p, const P3& a, const P3& b, const P3& c) {
    const P3 ab = md_sub(b, a), ac = md_sub(c, a), bc = md_sub(c, b);
    const P3 ap = md_sub(p, a), bp = md_sub(p, b), cp = md_sub(p, c);
    const float d1 = md_dot(ab, ap), d2 = md_dot(ac, ap), d3 = md_dot(ab, bp), d4 = md_dot(ac, bp), d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float sum = (va + vb) + vc;
    const float E2 = fmaxf(fmaxf(md_dot(ab, ab), md_dot(ac, ac)), md_dot(bc, bc));
    const float m  = fmaxf(fmaxf(md_dot(ap, ap), md_dot(bp, bp)), md_dot(cp, cp));
    if (!(sum > (kMeshDegenerate * E2) * m)) {
        Closest r = closest_on_segment(p, a, ab);
        const Closest s = closest_on_segment(p, b, bc), t = closest_on_segment(p, a, ac);
        if (s.d2 < r.d2) r = s;
        if (t.d2 < r.d2) r = t;
        return r;
    }
    if (d1 <= 0.f && d2 <= 0.f) return md_at(p, a);
    if (d3 >= 0.f && d4 <= d3) return md_at(p, b);
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) return md_at(p, md_along(a, ab, md_ratio(d1, d1 - d3)));
    if (d6 >= 0.f && d5 <= d6) return md_at(p, c);
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) return md_at(p, md_along(a, ac, md_ratio(d2, d2 - d6)));
    const float e1 = d4 - d3, e2 = d5 - d6;
    if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) return md_at(p, md_along(b, bc, md_ratio(e1, e1 + e2)));
    return md_at(p, md_along(md_along(a, ab, vb / sum), ac, vc / sum));
}

}  // namespace sobfu_hip
