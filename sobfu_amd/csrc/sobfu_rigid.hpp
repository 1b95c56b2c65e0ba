// Small rigid-motion algebra in fp64, shared by the kernels that solve for a pose on the device (mesh_align_kernels.hip), by host tools
// (tests/cpp/rigid_solve_tool.cpp) and by the C++ shell (include/sobfu_amd/evaluate.hpp): the same lines everywhere, so the same bits.
// tests/mesh_align_reference.py restates every function operation by operation (every TU is built with -ffp-contract=off; there is no
// fused operation here): the order of the floating-point operations below is part of the contract.  Plain doubles and floats, no HIP
// types: a host compiler takes this header too.  Every loop has compile-time bounds and is fully unrolled, so in a kernel nothing
// goes to scratch.
//
//   LDL^T      A (symmetric N x N, only read at and below the diagonal) = L D L^T, column by column:
//                D_j = A_jj - sum_k<j (L_jk L_jk) D_k, L_ij = (A_ij - sum_k<j (L_ik L_jk) D_k) / D_j, the sums taken left to right by
//                repeated subtraction; det = ((((1 D_0) D_1) ...) D_N-1).  positive: every D_j > 0 (a NaN pivot is not); finite: every
//                D_j < +Inf.  ldlt_ok = positive and finite -- the rule of mesh alignment.  (Projective ICP has its own rule on top of
//                `positive`: |det| >= 1e-15, the reference's null-space check at that problem's scaling.)
//   solve      L y = b forwards (y_r = b_r - sum_k<r L_rk y_k), z_r = y_r / D_r, L^T x = z backwards (x_r = z_r - sum_k>r L_kr x_k)
//   Rodrigues  theta = sqrt((w0 w0 + w1 w1) + w2 w2); theta == 0 gives I exactly, else k = w / theta, c = cos, s = sin, c1 = 1 - c and
//                R = c I + c1 k k^T + s [k]x, each entry written as below ((c1 kx) ky - s kz, ...)
//   compose    pose (16 floats, row-major 4 x 4; rows 0..2 are read and written, row 3 is left alone) <- (R, t) pose:
//                out[r][c] = (float) ((R_r0 P_0c + R_r1 P_1c) + R_r2 P_2c), out[r][3] = (float) (((R_r0 P_03 + R_r1 P_13) + R_r2 P_23) + t_r)
//   inverse    of a rigid pose: out[r][c] = P[c][r], out[r][3] = (float) -((P_0r P_03 + P_1r P_13) + P_2r P_23) in fp64, row 3 = (0, 0, 0, 1)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define SOBFU_RIGID_FN __host__ __device__ __forceinline__
#define SOBFU_RIGID_UNROLL _Pragma("unroll")
#else
#define SOBFU_RIGID_FN inline
#define SOBFU_RIGID_UNROLL
#endif

namespace sobfu_hip {

template <int N>
struct Ldlt {
    double L[N][N];  // strictly below the diagonal
    double D[N];
    double det;
    bool positive, finite;
};

template <int N>
SOBFU_RIGID_FN bool ldlt_ok(const Ldlt<N>& f) {
    return f.positive && f.finite;
}

template <int N>
SOBFU_RIGID_FN void ldlt_factor(const double (&A)[N][N], Ldlt<N>& f) {
    f.det = 1.0;
    f.positive = true, f.finite = true;
    SOBFU_RIGID_UNROLL
    for (int c = 0; c < N; ++c) {
        double dc = A[c][c];
        SOBFU_RIGID_UNROLL
        for (int k = 0; k < c; ++k) dc -= f.L[c][k] * f.L[c][k] * f.D[k];
        f.D[c] = dc;
        f.det *= dc;
        f.positive = f.positive && dc > 0.0;
        f.finite = f.finite && dc < (double) INFINITY;
        SOBFU_RIGID_UNROLL
        for (int r = c + 1; r < N; ++r) {
            double a = A[r][c];
            SOBFU_RIGID_UNROLL
            for (int k = 0; k < c; ++k) a -= f.L[r][k] * f.L[c][k] * f.D[k];
            f.L[r][c] = a / dc;
        }
    }
}

template <int N>
SOBFU_RIGID_FN void ldlt_solve(const Ldlt<N>& f, const double (&b)[N], double (&x)[N]) {
    SOBFU_RIGID_UNROLL
    for (int r = 0; r < N; ++r) {  // L y = b
        double y = b[r];
        SOBFU_RIGID_UNROLL
        for (int k = 0; k < r; ++k) y -= f.L[r][k] * x[k];
        x[r] = y;
    }
    SOBFU_RIGID_UNROLL
    for (int r = 0; r < N; ++r) x[r] = x[r] / f.D[r];
    SOBFU_RIGID_UNROLL
    for (int r = N - 1; r >= 0; --r) {  // L^T x = z
        double y = x[r];
        SOBFU_RIGID_UNROLL
        for (int k = r + 1; k < N; ++k) y -= f.L[k][r] * x[k];
        x[r] = y;
    }
}

// the rotation of the rotation vector w (row-major 3 x 3) -> |w|
SOBFU_RIGID_FN double rodrigues(const double (&w)[3], double (&R)[9]) {
    R[0] = 1.0, R[1] = 0.0, R[2] = 0.0, R[3] = 0.0, R[4] = 1.0, R[5] = 0.0, R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    if (th > 0.0) {
        const double kx = w[0] / th, ky = w[1] / th, kz = w[2] / th, c = cos(th), s = sin(th), c1 = 1.0 - c;
        R[0] = c + c1 * kx * kx, R[1] = c1 * kx * ky - s * kz, R[2] = c1 * kx * kz + s * ky;
        R[3] = c1 * ky * kx + s * kz, R[4] = c + c1 * ky * ky, R[5] = c1 * ky * kz - s * kx;
        R[6] = c1 * kz * kx - s * ky, R[7] = c1 * kz * ky + s * kx, R[8] = c + c1 * kz * kz;
    }
    return th;
}

// pose <- (R, t) pose; rows 0..2 of the 4 x 4 (pose may not alias P)
SOBFU_RIGID_FN void pose_compose(const double (&R)[9], const double (&t)[3], const float (&P)[12], float* pose) {
    SOBFU_RIGID_UNROLL
    for (int r = 0; r < 3; ++r) {
        SOBFU_RIGID_UNROLL
        for (int c = 0; c < 3; ++c) pose[4 * r + c] = (float) ((R[3 * r] * P[c] + R[3 * r + 1] * P[4 + c]) + R[3 * r + 2] * P[8 + c]);
        pose[4 * r + 3] = (float) (((R[3 * r] * P[3] + R[3 * r + 1] * P[7]) + R[3 * r + 2] * P[11]) + t[r]);
    }
}

// the inverse of a rigid 4 x 4 (out may not alias P)
SOBFU_RIGID_FN void rigid_inverse(const float* P, float* out) {
    SOBFU_RIGID_UNROLL
    for (int r = 0; r < 3; ++r) {
        SOBFU_RIGID_UNROLL
        for (int c = 0; c < 3; ++c) out[4 * r + c] = P[4 * c + r];
        out[4 * r + 3] = (float) -(((double) P[r] * (double) P[3] + (double) P[4 + r] * (double) P[7]) + (double) P[8 + r] * (double) P[11]);
    }
    out[12] = 0.f, out[13] = 0.f, out[14] = 0.f, out[15] = 1.f;
}

}  // namespace sobfu_hip
