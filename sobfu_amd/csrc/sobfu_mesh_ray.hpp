// A ray against a triangle, in fp32: the rule of mesh_ray_kernels.hip, shared by its grid walk, its brute-force kernel and the camera
// entry.  It is the watertight test of Woop, Benthin and Wald ("Watertight Ray/Triangle Intersection", JCGT 2(1), 2013) with a division
// at the end.  tests/mesh_ray_reference.py restates it operation by operation (every TU is built with -ffp-contract=off; there is no
// fused operation here): the order of the floating-point operations below is part of the contract.  Plain floats and P3, no HIP types:
// a host compiler takes this header too.
//
//   per ray (origin o, direction d, not normalised)
//     kz          the axis of the largest |d| (of equal ones the lowest axis); kx = kz + 1, ky = kz + 2 (mod 3), swapped when d[kz] < 0
//     Sx, Sy, Sz  d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
//     valid       o and d finite, d != 0 and Sz finite; any other ray misses everything and reads no memory
//   per triangle (a, b, c)
//     translate   A = a - o, B = b - o, C = c - o, per component
//     shear       Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz]; B and C likewise
//     edges       U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax: each the difference of two rounded products.  When any of
//                 the three is exactly 0, all three are recomputed from the same fp32 Ax .. Cy in fp64 (products exact, one rounding of
//                 the difference, so the sign is exact) and rounded to fp32
//     inside      U, V, W all >= 0 or all <= 0; det = (U + V) + W != 0
//     distance    Az = Sz A[kz], Bz = Sz B[kz], Cz = Sz C[kz]; T = (U Az + V Bz) + W Cz; t = T / det; a hit needs t_min < t <= t_max
//     answer      t, barycentrics (u, v) = (V / det, W / det) -- the weights of b and c, a has (1 - u) - v -- and side = +1 (det > 0: the
//                 ray meets the face whose corners run counter-clockwise as seen from the origin, the front) or -1 (the back)
// Two triangles that share an edge compute its edge function from the same two sheared corners: the two values are exact negatives of
// each other, in fp32 and in the fp64 recomputation alike, so a ray cannot slip between them, and a ray through a shared corner or edge
// hits both.  Do not reorder the operations.  A degenerate triangle (two or three equal corners, collinear corners) has det == 0 and is a
// miss.  Every comparison is written so that a NaN fails it: input whose products overflow gives a miss, never a NaN answer.
// The ray parameter t of a hit is a mix of Az, Bz, Cz with weights in [0, 1]: it never leaves the triangle's extent along kz.
#pragma once

#include <cmath>

#include "sobfu_mesh_distance.hpp"  // P3

namespace sobfu_hip {

struct Ray {
    P3 o;
    int kx, ky, kz;
    float Sx, Sy, Sz;
    bool valid;
};
struct RayHit {
    float t;  // +Inf: a miss
    float u, v;
    int side;  // +1 front, -1 back, 0 miss
};

SOBFU_MD_FN float mr_pick(const P3& p, int k) { return k == 0 ? p.x : k == 1 ? p.y : p.z; }
SOBFU_MD_FN bool mr_finite(float x) { return fabsf(x) < INFINITY; }

SOBFU_MD_FN Ray ray_setup(const P3& o, const P3& d) {
    Ray r;
    r.o = o;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int kz = 0;
    if (ay > ax) kz = 1;
    if (az > fmaxf(ax, ay)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = mr_pick(d, kz);
    if (dz < 0.f) {
        const int s = kx;
        kx = ky, ky = s;
    }
    r.kx = kx, r.ky = ky, r.kz = kz;
    r.Sx = mr_pick(d, kx) / dz, r.Sy = mr_pick(d, ky) / dz, r.Sz = 1.f / dz;
    r.valid = mr_finite(o.x) && mr_finite(o.y) && mr_finite(o.z) && mr_finite(d.x) && mr_finite(d.y) && mr_finite(d.z) && fmaxf(fmaxf(ax, ay), az) > 0.f &&
              mr_finite(r.Sz);
    return r;
}

SOBFU_MD_FN RayHit ray_miss() { return RayHit{INFINITY, 0.f, 0.f, 0}; }

SOBFU_MD_FN RayHit ray_triangle(const Ray& r, const P3& a, const P3& b, const P3& c, float t_min, float t_max) {
    const P3 A = md_sub(a, r.o), B = md_sub(b, r.o), C = md_sub(c, r.o);
    const float Akz = mr_pick(A, r.kz), Bkz = mr_pick(B, r.kz), Ckz = mr_pick(C, r.kz);
    const float Ax = mr_pick(A, r.kx) - r.Sx * Akz, Ay = mr_pick(A, r.ky) - r.Sy * Akz;
    const float Bx = mr_pick(B, r.kx) - r.Sx * Bkz, By = mr_pick(B, r.ky) - r.Sy * Bkz;
    const float Cx = mr_pick(C, r.kx) - r.Sx * Ckz, Cy = mr_pick(C, r.ky) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (U == 0.f || V == 0.f || W == 0.f) {
        U = (float) ((double) Cx * (double) By - (double) Cy * (double) Bx);
        V = (float) ((double) Ax * (double) Cy - (double) Ay * (double) Cx);
        W = (float) ((double) Bx * (double) Ay - (double) By * (double) Ax);
    }
    if (!((U >= 0.f && V >= 0.f && W >= 0.f) || (U <= 0.f && V <= 0.f && W <= 0.f))) return ray_miss();
    const float det = (U + V) + W;
    if (!(det != 0.f)) return ray_miss();
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float T = (U * Az + V * Bz) + W * Cz;
    const float t = T / det;
    if (!(t > t_min && t <= t_max)) return ray_miss();
    return RayHit{t, V / det, W / det, det > 0.f ? 1 : -1};
}

}  // namespace sobfu_hip
