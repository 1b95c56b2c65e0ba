// The normal equations of a 6-dof point-to-plane step on the device, shared by projective ICP (icp_kernels.hip, fp32 sums) and mesh
// alignment (mesh_align_kernels.hip, fp64 sums): the 29 sums of a pass, their deterministic workgroup reduction into slabs, their unpacking
// into A x = b and the update of the pose.  tests/icp_reference.py and tests/mesh_align_reference.py restate these lines operation by
// operation.  What differs between the two solves -- how the slabs are added, when the system counts as singular, the 3-dof block, status
// and trace -- stays in their files; the LDL^T, Rodrigues and the pose composition are sobfu_rigid.hpp's.  Internal linkage.
#pragma once

#include "sobfu_device.hpp"
#include "sobfu_rigid.hpp"

namespace sobfu_hip {
namespace {

constexpr int kSums = 29;       // 21 products J_i J_j (i <= j < 6, row-major), 6 products J_i r, the inlier count, r r
constexpr int kSlab = 32;       // values per partial slab
constexpr int kMaxParts = 256;  // partial slabs of one pass
constexpr int kThreads = 256;

// workgroup sum of N values per thread (4 waves): a wave64 butterfly (every lane ends with the sum in the same, fixed association order),
// then wave 0 + 1 + 2 + 3 through LDS; valid in wave 0
template <class T, int N>
SOBFU_DEV void block_sum(T (&v)[N], T (*lds)[N]) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], h, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) lds[wave][k] = v[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
    }
}

// one inlier: the row J = [s x n, n] and the residual r into the 29 sums
template <class T>
SOBFU_DEV void add_row(T (&acc)[kSums], const T (&row)[6], T r) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += row[i] * row[j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += row[i] * r;
    acc[27] += (T) 1;
    acc[28] += r * r;
}

// the sums as the symmetric system A x = b
SOBFU_DEV void unpack_sums(const double (&acc)[kSums], double (&A)[6][6], double (&b)[6]) {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = acc[k++];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) b[r] = acc[21 + r];
}

// pose <- (Rodrigues(w), t) pose -> |w|
SOBFU_DEV double apply_increment(const double (&w)[3], const double (&t)[3], float* pose) {
    double R[9];
    const double th = rodrigues(w, R);
    float P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = pose[k];
    pose_compose(R, t, P, pose);
    return th;
}

}  // namespace
}  // namespace sobfu_hip
