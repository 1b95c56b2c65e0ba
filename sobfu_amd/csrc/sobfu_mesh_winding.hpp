// The generalised winding number of an oriented triangle soup from its boundary: the rule behind mesh_winding_kernels.hip (DESIGN.md
// 4.14).  Close the mesh with the strips that run from every boundary edge to infinity along -x: a row along +x never meets a strip, so
//
//   w(p) = N(p) + (1 / 4 pi) sum over boundary edges (u -> v, coefficient k) of k Omega_strip(p; u, v)
//
// with N the signed number of crossings of the row beyond p (the crossing rule of sobfu_mesh_parity.hpp, each crossing with the common
// sign of its edge functions) and Omega_strip the solid angle of the strip.  tests/mesh_winding_reference.py restates all of it.  Plain
// C++, no HIP types: a host compiler takes this header too (every TU is built with -ffp-contract=off).
//
//   crossing   signed_row_crossing of sobfu_mesh_parity.hpp, the one statement of the rule
//   strip      a = u - p, b = v - p: y and z translated in fp32 exactly as the crossing rule translates them, x in fp64.
//              W = a_y b_z - a_z b_y in fp64 (exact products, one rounding: the sign is exact); the strip's sign is -parity_sign(W, ...),
//              never the sign of a rounded determinant, so the strip flips exactly where N jumps; an edge without projected length
//              (sign 0) contributes nothing.  magnitude = 2 atan2(|W|, den),
//              den = ((|a| |b| + (a_x b_x + (a_y b_y + a_z b_z))) - b_x |a|) - a_x |b|, |a| = sqrt(a_x a_x + (a_y a_y + a_z a_z)), all fp64.
//              What depends on the row alone (StripRow) is split from what depends on x (strip_magnitude): the row kernel computes the
//              former once per row
//   triangle   van Oosterom and Strackee: 2 atan2(a . (b x c), |a| |b| |c| + (a . b) |c| + (b . c) |a| + (c . a) |b|) from the fp64
//              differences a = A - p ...: the definition w = sum of all triangles / 4 pi
//   seam       a boundary vertex v with (v.y - p.y) == 0 and (v.z - p.z) == 0 in fp32 and v.x > p.x: p lies on the ray where two
//              strips meet, each strip's angle there depends on the direction of approach, and the formula does not hold.  Such
//              points take the definition
//   inside     w > 1 / 2
#pragma once

#include "sobfu_mesh_parity.hpp"

namespace sobfu_hip {

constexpr double kFourPi = 12.566370614359172953850573533118;

// what the boundary edge u -> v is to the row (., py, pz)
struct StripRow {
    double absW, qa, qb, dyz;  // |W|, a_y a_y + a_z a_z, b_y b_y + b_z b_z, a_y b_y + a_z b_z
    int sign;                  // -parity_sign(W); 0: no projected length
    bool seam_u, seam_v;       // the endpoint has the row's y and z
};

SOBFU_MD_FN StripRow strip_row(float uy, float uz, float vy, float vz, float py, float pz) {
    const float Ay = uy - py, Az = uz - pz, By = vy - py, Bz = vz - pz;
    const double ay = (double) Ay, az = (double) Az, by = (double) By, bz = (double) Bz;
    const double W = ay * bz - az * by;
    return StripRow{fabs(W), ay * ay + az * az, by * by + bz * bz, ay * by + az * bz, -parity_sign(W, Ay, Az, By, Bz),
                    Ay == 0.f && Az == 0.f, By == 0.f && Bz == 0.f};
}

// 2 atan2(|W|, den) with ax = u.x - p.x, bx = v.x - p.x in fp64
SOBFU_MD_FN double strip_magnitude(const StripRow& r, double ax, double bx) {
    const double la = sqrt(ax * ax + r.qa), lb = sqrt(bx * bx + r.qb);
    const double den = ((la * lb + (ax * bx + r.dyz)) - bx * la) - ax * lb;
    return 2.0 * atan2(r.absW, den);
}

// the signed solid angle at p of the strip from the edge u -> v to infinity along -x
SOBFU_MD_FN double strip_angle(const P3& u, const P3& v, const P3& p) {
    const StripRow r = strip_row(u.y, u.z, v.y, v.z, p.y, p.z);
    if (r.sign == 0) return 0.0;
    return (double) r.sign * strip_magnitude(r, (double) u.x - (double) p.x, (double) v.x - (double) p.x);
}

struct D3 {
    double x, y, z;
};
SOBFU_MD_FN D3 from(const P3& v, const P3& p) { return D3{(double) v.x - (double) p.x, (double) v.y - (double) p.y, (double) v.z - (double) p.z}; }
SOBFU_MD_FN double ddot(const D3& u, const D3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

// the signed solid angle of the triangle whose corners, seen from the point, are a, b, c
SOBFU_MD_FN double triangle_angle(const D3& a, const D3& b, const D3& c) {
    const double la = sqrt(ddot(a, a)), lb = sqrt(ddot(b, b)), lc = sqrt(ddot(c, c));
    const D3 bc{b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x};
    const double num = ddot(a, bc);
    const double den = ((la * lb * lc + ddot(a, b) * lc) + ddot(b, c) * la) + ddot(c, a) * lb;
    return 2.0 * atan2(num, den);
}

// p lies on the seam ray of the boundary vertex v
SOBFU_MD_FN bool seam_point(const P3& v, const P3& p) { return v.y - p.y == 0.f && v.z - p.z == 0.f && v.x > p.x; }

}  // namespace sobfu_hip
