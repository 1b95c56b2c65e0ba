// Does the row through (., py, pz) along +x cross a triangle, and where: the counting rule behind the inside / outside test of
// mesh_voxel_kernels.hip.  The ray rule of sobfu_mesh_ray.hpp is watertight but does not count: a ray through a shared
// edge hits both triangles.  Here every row lies strictly on one side of every edge, so a closed mesh is crossed an even number of times
// and the parity of the crossings beyond x says inside or outside.  tests/mesh_parity_reference.py restates the rule operation by
// operation (every TU is built with -ffp-contract=off): the order of the operations below is part of the contract.  Plain C++, no HIP
// types: a host compiler takes this header too.
//
//   translate   Ay = a.y - py, Az = a.z - pz, likewise B and C, in fp32: the subtraction keeps the sign, and a corner shared by two
//               triangles becomes the same 2-D point in both
//   edges       in fp64 from those fp32 values: U = By Cz - Bz Cy (edge B -> C), V = Cy Az - Cz Ay (C -> A), W = Ay Bz - Az By (A -> B).
//               The products are exact and the difference is rounded once: the sign is exact
//   ties        an edge function of the ordered edge (P, Q) that is exactly 0 takes the sign it would have with the row moved by
//               (+e, +e^2) in (y, z): E + e (Pz - Qz) + e^2 (Qy - Py), so the sign of Pz - Qz, else that of Qy - Py, else none (an edge
//               without length: the triangle is no crossing).  Antisymmetric in (P, Q) and computed from the same values in both
//               triangles of a shared edge
//   crossing    the three signs are equal and det = (U + V) + W != 0 (a triangle seen edge-on never crosses); sign = their common
//               sign, 0 where the row does not cross
//   position    X = ((U a.x + V b.x) + W c.x) / det in fp64, absolute
//   inside      (x, py, pz) is inside iff the number of crossings with X > (double) x is odd
//   open rows   a row whose total number of crossings is odd: the mesh is not closed there
#pragma once

#include "sobfu_mesh_distance.hpp"

namespace sobfu_hip {

struct SignedCrossing {
    int sign;  // +1 / -1: the common sign of the three edge functions; 0: no crossing
    double X;
};

// the sign of the edge function e of the ordered edge (P, Q), never 0 for an edge with length
SOBFU_MD_FN int parity_sign(double e, float Py, float Pz, float Qy, float Qz) {
    if (e > 0.0) return 1;
    if (e < 0.0) return -1;
    if (Pz != Qz) return Pz > Qz ? 1 : -1;
    if (Qy != Py) return Qy > Py ? 1 : -1;
    return 0;
}

// the one statement of the rule: the parity test counts the crossings (sign != 0), the winding number of sobfu_mesh_winding.hpp adds the signs
SOBFU_MD_FN SignedCrossing signed_row_crossing(const P3& a, const P3& b, const P3& c, float py, float pz) {
    const float Ay = a.y - py, Az = a.z - pz, By = b.y - py, Bz = b.z - pz, Cy = c.y - py, Cz = c.z - pz;
    const double U = (double) By * (double) Cz - (double) Bz * (double) Cy;
    const double V = (double) Cy * (double) Az - (double) Cz * (double) Ay;
    const double W = (double) Ay * (double) Bz - (double) Az * (double) By;
    const int su = parity_sign(U, By, Bz, Cy, Cz), sv = parity_sign(V, Cy, Cz, Ay, Az), sw = parity_sign(W, Ay, Az, By, Bz);
    const double det = (U + V) + W;
    if (su == 0 || su != sv || su != sw || !(det != 0.0)) return SignedCrossing{0, 0.0};
    return SignedCrossing{su, ((U * (double) a.x + V * (double) b.x) + W * (double) c.x) / det};
}

}  // namespace sobfu_hip
