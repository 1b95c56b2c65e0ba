/*
 * sobfu_hip.h -- C ABI of the MI355X-native SobolevFusion hot path (libsobfu_hip.so, gfx950).
 *
 * This is the drop-in boundary: one entry point per host-callable launcher of the reference's "L1 device
 * API" (include/sobfu/{solver,vector_fields,reductor}.hpp `namespace device`, include/kfusion/internal.hpp
 * :189-257), plus an opaque solver handle replacing sobfu::cuda::Solver's workspace + hot loop.  The C++
 * shells under include/sobfu_amd/ rebuild the reference's class surface on top of it; INTEGRATION.md shows
 * the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer marked `d_` is a DEVICE pointer the callee does not own;
 *  - volumes are dense, x fastest: idx = x + X*(y + Y*z) (reference: src/sobfu/cuda/vector_fields.cu:20-22);
 *    TSDF voxel = float2 {tsdf, weight} (8 B), vector-field voxel = float4 with w == 0 (16 B), Jacobian voxel
 *    = 4 x float4 (64 B, row 3 unused) -- the reference's layouts, unchanged;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Launches are asynchronous; nothing
 *    synchronises unless documented (the reference's per-call cudaDeviceSynchronize is NOT reproduced);
 *  - return value: 0 on success, otherwise a hipError_t (positive) or a SOBFU_E_* code (negative).  The
 *    reference prints and calls exit(0) on any CUDA error (src/kfusion/device_memory.cpp:7-10); the C++ shells
 *    keep that behaviour, the C ABI itself never exits.
 */
#ifndef SOBFU_HIP_H
#define SOBFU_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define SOBFU_HIP_ABI_VERSION 3

#define SOBFU_E_BADARG (-1)      /* null pointer, non-positive dims, ... */
#define SOBFU_E_FILTER (-2)      /* (s, lambda) not in the reference's Sobolev filter table */
#define SOBFU_E_UNSUPPORTED (-3) /* valid in the reference but outside this build's limits */

int sobfu_hip_abi_version(void);
/* Human-readable text for a return code of this library. */
const char* sobfu_hip_error_string(int code);

/* ------------------------------------------------------------------------------------------------------
 * TSDF volume  (kfusion::device::*, include/kfusion/internal.hpp:189-198, src/kfusion/cuda/tsdf_volume.cu)
 * ---------------------------------------------------------------------------------------------------- */
/* clear_volume (tsdf_volume.cu:23-46) */
int sobfu_hip_clear_volume(float* d_vol, int X, int Y, int Z, void* stream);
/* integrate(dists, volume, aff, proj) (tsdf_volume.cu:56-101,141-162).  d_dists: pitched float image
 * (step in bytes) of ray lengths in metres; R (row-major 3x3) and t: vol2cam = camera_pose^-1 * volume_pose
 * (src/kfusion/tsdf_volume.cpp:95-106); voxel_size[3]; trunc/eta in metres.  Voxels that project outside
 * the image, onto Dp <= 0 or behind the camera are left untouched.  A voxel's camera point is R * centre + t
 * for any rotation (the z march adds R * (0, 0, vs_z) per plane; the reference adds (0, 0, vs_z), which is
 * the same bits for the rotations it passes -- third column (0, 0, 1) -- and not the voxel otherwise). */
int sobfu_hip_integrate_depth(const float* d_dists, int dists_step_bytes, int rows, int cols, float* d_vol, int X,
                              int Y, int Z, const float voxel_size[3], float trunc_dist, float eta,
                              const float R[9], const float t[3], float fx, float fy, float cx, float cy,
                              void* stream);
/* integrate(phi_global, phi_n_psi) (tsdf_volume.cu:103-130,164-173): running weighted average fusion. */
int sobfu_hip_integrate_fuse(float* d_phi_global, const float* d_phi_n_psi, int X, int Y, int Z, float max_weight,
                             void* stream);
/* init_{sphere,box,ellipsoid,plane,torus} (tsdf_volume.cu:181-382): analytic truncated SDFs. */
int sobfu_hip_init_sphere(float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist, float eta,
                          const float centre[3], float radius, void* stream);
int sobfu_hip_init_box(float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                       const float b[3], void* stream);
int sobfu_hip_init_ellipsoid(float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                             const float r[3], void* stream);
int sobfu_hip_init_plane(float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist, float z,
                         void* stream);
int sobfu_hip_init_torus(float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                         const float t[2], void* stream);

/* ------------------------------------------------------------------------------------------------------
 * depth pre-steps  (include/kfusion/internal.hpp:236-239, src/kfusion/cuda/imgproc.cu:8-77,233-254)
 * ---------------------------------------------------------------------------------------------------- */
/* bilateralFilter: uint16 mm depth, sigma_depth in metres (scaled x1000 inside, imgproc.cu:43). */
int sobfu_hip_bilateral_filter(const uint16_t* d_src, int src_step_bytes, uint16_t* d_dst, int dst_step_bytes,
                               int rows, int cols, int kernel_size, float sigma_spatial, float sigma_depth,
                               void* stream);
/* truncateDepth: depth > max_dist_m*1000 -> 0, in place. */
int sobfu_hip_truncate_depth(uint16_t* d_depth, int step_bytes, int rows, int cols, float max_dist_m, void* stream);
/* compute_dists: uint16 mm depth -> ray length in metres. */
int sobfu_hip_compute_dists(const uint16_t* d_depth, int depth_step_bytes, float* d_dists, int dists_step_bytes,
                            int rows, int cols, float fx, float fy, float cx, float cy, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * vector fields  (sobfu::device::*, include/sobfu/vector_fields.hpp:140-241, src/sobfu/cuda/vector_fields.cu)
 * ---------------------------------------------------------------------------------------------------- */
int sobfu_hip_clear_field(float* d_field, int X, int Y, int Z, void* stream);   /* clear (:28-50) */
int sobfu_hip_init_identity(float* d_psi, int X, int Y, int Z, void* stream);   /* init_identity (:56-79) */
/* apply (:81-109): phi_warped(x) = trilinear phi(psi(x)), weight = nearest-floor weight. */
int sobfu_hip_apply(const float* d_phi, float* d_phi_warped, const float* d_psi, int X, int Y, int Z, void* stream);
/* estimate_inverse (:111-138): n_sweeps (reference: 48) in-place fixed-point sweeps on d_psi_inv. */
int sobfu_hip_estimate_inverse(const float* d_psi, float* d_psi_inv, int X, int Y, int Z, int n_sweeps,
                               void* stream);
/* The tail of Solver::estimate_psi fused (solver.cu:196-199): psi_inv <- identity, n_sweeps fixed-point sweeps, and
 * phi_warped = phi o psi_inv, in one pass (same values as init_identity + estimate_inverse + apply). */
int sobfu_hip_inverse_and_warp(const float* d_psi, float* d_psi_inv, const float* d_phi, float* d_phi_warped, int X, int Y, int Z,
                               int n_sweeps, void* stream);
/* TsdfDifferentiator::calculate (:144-208): central-difference gradient, exact 0 on boundary faces. */
int sobfu_hip_tsdf_gradient(const float* d_vol, float* d_grad, int X, int Y, int Z, void* stream);
/* SecondOrderDifferentiator::calculate (:278-337): NEGATIVE 7-point Laplacian of psi. */
int sobfu_hip_laplacian(const float* d_psi, float* d_L, int X, int Y, int Z, void* stream);
/* Differentiator::calculate (mode 0) / calculate_deformation_jacobian (mode 1) (:389-472). */
int sobfu_hip_jacobian(const float* d_psi, float* d_J, int X, int Y, int Z, int mode, void* stream);
int sobfu_hip_clear_jacobian(float* d_J, int X, int Y, int Z, void* stream);    /* clear(Jacobian&) (:353-383) */

/* ------------------------------------------------------------------------------------------------------
 * solver launchers  (include/sobfu/solver.hpp:109-136, src/sobfu/cuda/solver.cu)
 * ---------------------------------------------------------------------------------------------------- */
/* decompose_sobolev_filter (src/sobfu/solver.cpp:160-262): writes s normalised taps to host array out. */
int sobfu_hip_sobolev_filter(int s, float lambda, float* out);
/* calculate_potential_gradient (solver.cu:15-47) */
int sobfu_hip_potential_gradient(const float* d_phi_n_psi, const float* d_phi_global, const float* d_grad,
                                 const float* d_L, float* d_nabla_U, float w_reg, int X, int Y, int Z, void* stream);
/* convolution_{rows,columns,depth} (solver.cu:237-459): rows ASSIGNS dst = Sx*src, columns / depth ACCUMULATE
 * dst += S*src.  taps: 7 HOST floats (the reference's __constant__ S, solver.cu:229-234, passed by value so the
 * library holds no global state). */
int sobfu_hip_convolution_rows(float* d_dst, const float* d_src, const float taps[7], int w, int h, int d,
                               void* stream);
int sobfu_hip_convolution_columns(float* d_dst, const float* d_src, const float taps[7], int w, int h, int d,
                                  void* stream);
int sobfu_hip_convolution_depth(float* d_dst, const float* d_src, const float taps[7], int w, int h, int d,
                                void* stream);
/* update_psi (solver.cu:53-79): updates = alpha*nabla_U_S; psi -= updates. */
int sobfu_hip_update_psi(float* d_psi, const float* d_nabla_U_S, float* d_updates, float alpha, int X, int Y, int Z,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------
 * reductions  (sobfu::device::Reductor, include/sobfu/reductor.hpp:24-50, src/sobfu/reductor.cpp,
 * src/sobfu/cuda/reductor.cu, launch sizing src/sobfu/precomp.cpp:20-43)
 * ---------------------------------------------------------------------------------------------------- */
int sobfu_hip_reduce_config(int n, int* blocks, int* threads);
/* Each call runs the block reduction with the reference's tree shape, copies the block partials to the host
 * and finishes on the CPU exactly as final_reduce / final_reduce_max do; it SYNCHRONISES the stream.
 * d_scratch: device scratch of >= blocks*8 bytes. */
int sobfu_hip_data_energy(const float* d_phi_global, const float* d_phi_n, int n, void* d_scratch, float* out,
                          void* stream);
int sobfu_hip_reg_energy_sobolev(const float* d_J, int n, void* d_scratch, float* out, void* stream);
/* out[0] = max ||update|| (sqrt rounded down), out[1] = float-encoded linear index (reductor.cu:357-368). */
int sobfu_hip_max_update_norm(const float* d_updates, int n, void* d_scratch, float out[2], void* stream);
/* Same value as reg_energy_sobolev(J(psi, mode 1)) without materialising the 64 B/voxel Jacobian. */
int sobfu_hip_reg_energy_sobolev_from_psi(const float* d_psi, int X, int Y, int Z, void* d_scratch, float* out,
                                          void* stream);

/* ------------------------------------------------------------------------------------------------------
 * fused iteration kernels (MI355X-native decomposition of one pass of solver.cu:114-193; no reference
 * counterpart -- results are bit-identical to the launcher sequence above)
 * ---------------------------------------------------------------------------------------------------- */
/* pass A: nabla_U = (phi_n_psi - phi_global) * grad(phi_n_psi) + w_reg * (-Lap psi)   [a14 + a15 + a17] */
int sobfu_hip_fused_potential_gradient(const float* d_phi_n_psi, const float* d_phi_global, const float* d_psi,
                                       float* d_nabla_U, float w_reg, int X, int Y, int Z, void* stream);
/* pass B: u = alpha * (Sx + Sy + Sz)(nabla_U); psi -= u; phi_n_psi = phi_n o psi; max ||u||^2 folded into
 * d_max_sq_slots[256] with atomic max (uint32 view of non-negative floats)   [a18 + a19 + a12 + a20].
 * d_updates may be NULL (updates consumed in registers). */
int sobfu_hip_fused_smooth_update_apply(const float* d_nabla_U, float* d_psi, const float* d_phi_n,
                                        float* d_phi_n_psi, float* d_updates, uint32_t* d_max_sq_slots,
                                        const float taps[7], float alpha, int X, int Y, int Z, void* stream);

/* Compact-format conversions (n = number of voxels; the format the multi-GPU tile entry points below accept with compact != 0):
 * float4 <-> packed xyz (unpack leaves .w untouched) and float2 {tsdf, weight} -> tsdf. */
int sobfu_hip_pack_vec3(const float* d_src4, float* d_dst3, size_t n, void* stream);
int sobfu_hip_unpack_vec3(const float* d_src3, float* d_dst4, size_t n, void* stream);
int sobfu_hip_extract_tsdf(const float* d_src2, float* d_dst1, size_t n, void* stream);

/* Multi-GPU tiles (the 2x2x2 split of BASELINE config 4, z-slabs as 1x1xN): every field argument is a LOCAL
 * array (Lx, Ly, Lz) whose cell (0, 0, 0) is global cell (xb, yb, zb) of the (Xg, Yg, Zg) volume and that carries halo cells on every side that faces a neighbour tile;
 * d_phi_n / d_phi / the d_psi of estimate_inverse are WHOLE volumes.  `box` = (x0, x1, y0, y1, z0, z1): the cells a launch produces;
 * `own`: the cells that belong to this rank (they alone enter the max-norm).  thin != 0 evaluates the box DIRECTLY -- one lane per
 * cell, every tap read through the caches -- instead of by a z-march: for boxes a few cells thick (the one-cell shells of a tile,
 * halo faces), same results.  A thin pass-A launch is never gated (it writes scratch only).  Boundary rules apply at array edges, which are volume boundaries
 * exactly where a tile has no halo.  compact != 0: the field arguments are in the compact iteration format -- psi / nabla_U 12-byte
 * xyz triples, phi_n o psi / phi_global / phi_n tsdf-only floats.  d_prev_slots (may be NULL) and max_update_norm form the
 * device-side convergence gate (see the solver handle). */
int sobfu_hip_tile3_init_identity(float* d_psi, int Lx, int Ly, int Lz, int xb, int yb, int zb, void* stream);
int sobfu_hip_tile3_apply(const float* d_phi, int Xg, int Yg, int Zg, float* d_phi_warped, const float* d_psi, int Lx, int Ly, int Lz,
                          void* stream);
int sobfu_hip_tile3_estimate_inverse(const float* d_psi, int Xg, int Yg, int Zg, float* d_psi_inv, int Lx, int Ly, int Lz, int xb, int yb,
                                     int zb, int n_sweeps, void* stream);
/* The per-frame tail of a tile (reference src/sobfu/cuda/solver.cu:196-199; src/sobfu/cuda/vector_fields.cu:111-138) on a WINDOW of its
 * sources instead of the all-gathered volume: psi^-1(x), and every point its fixed-point iteration visits, lies within
 * r = max |psi - id| of x, so a tile needs psi / phi_global only on its owned cells widened by ceil(r) + 1 cells.
 * win = (Wx, Wy, Wz, wbx, wby, wbz): extents of the window array and the global cell of its cell (0, 0, 0); box = (x0, x1, y0, y1, z0, z1):
 * the LOCAL cells to produce (others are left untouched); clamps act on the global extents (Xg, Yg, Zg) as in the whole-volume kernels:
 * same bits.  *d_violation (zeroed by the caller) becomes 1 when a sample fell outside the window -- the results are then invalid and the
 * caller repeats the tail on all-gathered sources.  sobfu_hip_tile3_max_displacement folds max(|psi - id| components) over `box` into
 * *d_max_bits (atomicMax on the float's bit pattern; zero it first; NaN / inf count as 3e38). */
int sobfu_hip_tile3_estimate_inverse_window(const float* d_psi_win, const int win[6], int Xg, int Yg, int Zg, float* d_psi_inv, int Lx, int Ly, int Lz,
                                            int xb, int yb, int zb, const int box[6], int n_sweeps, int* d_violation, void* stream);
int sobfu_hip_tile3_apply_window(const float* d_phi_win, const int win[6], int Xg, int Yg, int Zg, float* d_phi_warped, const float* d_psi, int Lx,
                                 int Ly, int Lz, const int box[6], int* d_violation, void* stream);
int sobfu_hip_tile3_max_displacement(const float* d_psi, int Lx, int Ly, int Lz, int xb, int yb, int zb, const int box[6], uint32_t* d_max_bits,
                                     void* stream);
int sobfu_hip_tile3_integrate_depth(const float* d_dists, int dists_step_bytes, int rows, int cols, float* d_vol_local, int Lx, int Ly,
                                    int Lz, int xb, int yb, int zb, const float voxel_size[3], float trunc_dist, float eta,
                                    const float R[9], const float t[3], float fx, float fy, float cx, float cy, void* stream);
/* thin != 0 is a diagnostic entry (the native tile loop launches lists its handle owns): every call uploads its box list to a
 * stream-ordered allocation on `stream`, one small blocking host-to-device copy per call. */
int sobfu_hip_tile3_potential_gradient(const float* d_phi_n_psi, const float* d_phi_global, const float* d_psi, float* d_nabla_U,
                                       float w_reg, int Lx, int Ly, int Lz, const int box[6], int thin,
                                       const uint32_t* d_prev_slots, float max_update_norm, int compact, void* stream);
int sobfu_hip_tile3_smooth_update_apply(const float* d_nabla_U, float* d_psi, const float* d_phi_n, float* d_phi_n_psi, float* d_updates,
                                        uint32_t* d_max_sq_slots, const float taps[7], float alpha, int Lx, int Ly, int Lz, int Xg,
                                        int Yg, int Zg, const int own[6], const int box[6], int thin,
                                        const uint32_t* d_prev_slots, float max_update_norm, int compact, void* stream);
int sobfu_hip_tile3_apply_tsdf_only(const float* d_phi1, int Xg, int Yg, int Zg, float* d_out1, const float* d_psi3, int Lx, int Ly, int Lz,
                                    void* stream);
/* Halo messages: n_boxes boxes (6 ints each) of a 12-byte (compact) field <-> consecutive segments of d_buf, x fastest inside a
 * box -- the send side packs the cells a neighbour needs, the receive side scatters them into its halo cells (<= 18 boxes). */
int sobfu_hip_tile3_pack(const float* d_field3, int Lx, int Ly, int Lz, float* d_buf, const int* boxes, int n_boxes, void* stream);
int sobfu_hip_tile3_unpack(float* d_field3, int Lx, int Ly, int Lz, const float* d_buf, const int* boxes, int n_boxes, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * solver handle  (sobfu::cuda::Solver, include/sobfu/solver.hpp:52-101, src/sobfu/solver.cpp:7-101)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct sobfu_hip_solver sobfu_hip_solver; /* opaque */

typedef struct {
    int verbosity;         /* 0 quiet; 1 energies on iterations {1, k*50, max_iter}; 2 every iteration */
    int max_iter;
    int s;                 /* Sobolev filter length (only 7 taps reach the kernels, solver.cu:211-234) */
    float max_update_norm; /* convergence threshold: break when max ||update|| <= this (solver.cu:183) */
    float lambda;
    float alpha;
    float w_reg;
} sobfu_hip_solver_params; /* = SolverParams, include/sobfu/solver.hpp:16-19 */

typedef struct {
    int iterations;        /* iterations executed (iter at break, or max_iter) */
    int converged;         /* 1 if the max-update-norm test fired */
    float last_max_update_norm;
    float last_max_update_index; /* float-encoded linear voxel index of the last iteration, when that iteration reported (verbosity 2; 1, 50 k, max_iter at verbosity 1: solver.cu:173); else NaN */
    float last_e_data, last_e_reg; /* energies of the last reporting iteration (verbosity > 0), else NaN */
} sobfu_hip_solver_report;

/* Allocates the per-solver device workspace (the reference's SpatialGradients + Reductor, minus the fields
 * it never touches: nabla_phi_n, J_inv, L_o_psi_inv -- src/sobfu/vector_fields.cpp:152-161). */
int sobfu_hip_solver_create(sobfu_hip_solver** out, int X, int Y, int Z, const sobfu_hip_solver_params* params);
int sobfu_hip_solver_destroy(sobfu_hip_solver* s);
int sobfu_hip_solver_set_params(sobfu_hip_solver* s, const sobfu_hip_solver_params* params);
/* Bytes of device memory held by the handle. */
size_t sobfu_hip_solver_workspace_bytes(const sobfu_hip_solver* s);
/* Solver::estimate_psi (src/sobfu/solver.cpp:69-101 -> src/sobfu/cuda/solver.cu:85-205).  Mutates psi,
 * psi_inv, phi_n_psi, phi_global_psi_inv; reads phi_global, phi_n.  Synchronises `stream` before returning
 * (the reference synchronises every iteration).  per_iter_max_norm (host, may be NULL): max_iter floats. */
int sobfu_hip_solver_estimate_psi(sobfu_hip_solver* s, const float* d_phi_global, float* d_phi_global_psi_inv,
                                  const float* d_phi_n, float* d_phi_n_psi, float* d_psi, float* d_psi_inv,
                                  sobfu_hip_solver_report* report, float* per_iter_max_norm, void* stream);
/* Only the gradient-descent loop (solver.cu:106-193), no inverse / canonical warp: the unit bench.py times.
 * Always runs exactly n_iters iterations when max_update_norm < 0. */
int sobfu_hip_solver_iterate(sobfu_hip_solver* s, const float* d_phi_global, const float* d_phi_n,
                             float* d_phi_n_psi, float* d_psi, int n_iters, sobfu_hip_solver_report* report,
                             float* per_iter_max_norm, void* stream);
/* The same loop in pieces (quiet solves only; SOBFU_E_UNSUPPORTED when verbosity > 0).  begin: the warp of solver.cu:106 and the
 * entry into the iteration format, room for max_iters iterations.  step: ENQUEUES n_iters more iterations and returns without
 * synchronising (the device-side gate turns every launch after the reference's `break` into a no-op).  end: synchronises, finds
 * the iteration the reference stops at, rebuilds psi / phi_n_psi exactly as iterate() leaves them, fills report and
 * per_iter_max_norm (max_iters floats, may be NULL).  One open session per handle; the four buffers must stay valid until end. */
int sobfu_hip_solver_begin(sobfu_hip_solver* s, const float* d_phi_global, const float* d_phi_n, float* d_phi_n_psi,
                           float* d_psi, int max_iters, void* stream);
int sobfu_hip_solver_step(sobfu_hip_solver* s, int n_iters, void* stream);
int sobfu_hip_solver_end(sobfu_hip_solver* s, sobfu_hip_solver_report* report, float* per_iter_max_norm, void* stream);
/* Pointer to the `updates` buffer (Reductor::updates, src/sobfu/reductor.cpp:26); valid until destroy.  Holds
 * the last iteration's updates only when verbosity > 0 or keep_updates was set. */
float* sobfu_hip_solver_updates(sobfu_hip_solver* s);
int sobfu_hip_solver_keep_updates(sobfu_hip_solver* s, int keep);
/* Quiet solves (verbosity 0) iterate by default on a private compact copy of the state -- psi / nabla_U as 12-byte xyz
 * triples, tsdf-only 4-byte phi_global / phi_n / phi_n o psi -- and rebuild the caller's buffers after the loop
 * (76 instead of 112 bytes per voxel-iteration, identical results).  enable = 0 iterates directly on the API buffers. */
int sobfu_hip_solver_set_compact(sobfu_hip_solver* s, int enable);
/* Per-kernel timing of the quiet path: HIP events recorded on the solver's stream around the pass A / pass B launches of
 * every stride-th iteration (0 = off, 1 = every iteration).  An event between two kernels drains the pipeline (a few
 * microseconds), so time a profiled run for its kernel split, not for its wall time.  Totals and the number of timed
 * iterations accumulate until reset; call get_profile only after the stream has been synchronised. */
int sobfu_hip_solver_set_profiling(sobfu_hip_solver* s, int stride);
int sobfu_hip_solver_get_profile(sobfu_hip_solver* s, float* ms_pass_a, float* ms_pass_b, int* launches, int reset);
/* Callback invoked by estimate_psi for every line the reference prints with std::cout (solver.cu:115-190);
 * NULL (default) = print to stdout like the reference. */
typedef void (*sobfu_hip_log_fn)(const char* line, void* user);
int sobfu_hip_solver_set_logger(sobfu_hip_solver* s, sobfu_hip_log_fn fn, void* user);

/* ------------------------------------------------------------------------------------------------------
 * marching cubes -- include/kfusion/internal.hpp:213-225, src/kfusion/cuda/marching_cubes.cu
 * `occupied`: 3 rows of `stride` ints on the device -- voxel index, vertex count, vertex offset (the reference's
 * DeviceArray2D<int>(3, cols)).  Unlike the reference (atomic append, run-dependent order) cells come out in ascending
 * voxel-index order.  Vertices / normals are float4 (x, -y, -z, 1), three per triangle, one normal per triangle.
 * ---------------------------------------------------------------------------------------------------- */
/* d_workspace / workspace_bytes: optional device scratch of >= sobfu_hip_mc_workspace_bytes(X, Y, Z) bytes that the caller
 * keeps between calls (kfusion::cuda::MarchingCubes owns one); NULL or too small = the scratch is allocated and freed inside
 * the call (two implicit device synchronisations per call). */
size_t sobfu_hip_mc_workspace_bytes(int X, int Y, int Z);
/* getOccupiedVoxels (marching_cubes.cu:143-163): rows 0 and 1; *h_count = min(active cells, max_size).  Synchronises.
 * X*Y*Z > INT32_MAX: SOBFU_E_UNSUPPORTED (int voxel indices, as in the reference). */
int sobfu_hip_mc_occupied_voxels(void* stream, const float* d_vol, int X, int Y, int Z, int* d_occupied, int stride, int max_size,
                                 int* h_count, void* d_workspace, size_t workspace_bytes);
/* computeOffsetsAndTotalVertices (marching_cubes.cu:165-181): row 2 = exclusive scan of row 1.  Synchronises. */
int sobfu_hip_mc_offsets(void* stream, int* d_occupied, int stride, int count, int* h_total_vertices, void* d_workspace,
                         size_t workspace_bytes);
/* generateTriangles (marching_cubes.cu:275-313); pose = volume -> world (R row-major, t).  Triangles that would end beyond
 * max_vertices are dropped (the reference does not check). */
int sobfu_hip_mc_generate_triangles(void* stream, const float* d_vol, int X, int Y, int Z, const int* d_occupied, int stride, int count,
                                    float size_x, float size_y, float size_z, const float R[9], const float t[3], float* d_vertices,
                                    float* d_normals, int max_vertices);
/* Indexed (welded) meshes: one vertex per cut grid edge that some active cell uses, shared by all its triangles.  Voxel v owns the edges
 * leaving it in +x, +y, +z; vertices come in ascending owner index, then axis x < y < z.  A vertex is the soup's interpolation along its
 * edge from the lower corner up, posed and stored like the soup's ((x, -y, -z, 1)); its normal is the TSDF gradient (central differences,
 * one-sided on a volume face, interpolated along the edge like the vertex), normalised, rotated by R and stored as (nx, -ny, -nz, 1) --
 * pointing toward positive TSDF; a zero gradient gives (0, 0, 0, 1).  Face k (int32 x 3) is soup triangle k with corners 1 and 2 swapped:
 * counter-clockwise seen from outside.  The rules are in sobfu_amd/csrc/mc_kernels.hip.
 * d_workspace (required): >= sobfu_hip_mc_indexed_workspace_bytes(X, Y, Z) bytes (6 per voxel + per-2048-voxel sums); X*Y*Z > INT32_MAX:
 * SOBFU_E_UNSUPPORTED. */
size_t sobfu_hip_mc_indexed_workspace_bytes(int X, int Y, int Z);
/* Counts of the whole mesh: active cells, vertices, triangles.  Leaves the per-voxel state in d_workspace for
 * sobfu_hip_mc_indexed_generate.  Synchronises. */
int sobfu_hip_mc_indexed_count(void* stream, const float* d_vol, int X, int Y, int Z, void* d_workspace, size_t workspace_bytes,
                               int* h_active_cells, int* h_vertices, int* h_triangles);
/* Same d_vol and workspace as the preceding count call; pose = volume -> world (R row-major, t).  Vertices / normals: float4, faces:
 * int32 x 3.  Never truncates: max_vertices or max_triangles below the count call's totals is SOBFU_E_BADARG before any kernel is
 * launched (reads the totals back: synchronises). */
int sobfu_hip_mc_indexed_generate(void* stream, const float* d_vol, int X, int Y, int Z, float size_x, float size_y, float size_z,
                                  const float R[9], const float t[3], void* d_workspace, size_t workspace_bytes, float* d_vertices,
                                  float* d_normals, int max_vertices, int* d_faces, int max_triangles);

/* ------------------------------------------------------------------------------------------------------
 * rendering -- kfusion::cuda::renderImage / renderTangentColors (include/kfusion/cuda/imgproc.hpp:30,42-46: declared, never
 * defined in the reference) and the KinectFusion raycaster the reference's TsdfVolume keeps a step factor for (tsdf_volume.hpp:91)
 * but does not have.  Points / normals: pitched float4 images (step in bytes, 16-byte aligned); images: pitched 8-bit BGRA
 * (kfusion::RGB, types.hpp:57-63, 4-byte aligned).  The rules are in sobfu_amd/csrc/render_kernels.hip.
 * ---------------------------------------------------------------------------------------------------- */
/* raycast: pixel (u, v) casts ((u - cx) / fx, (v - cy) / fy, 1) from the camera of vol2cam = (R row-major, t) -- the pose argument of
 * sobfu_hip_integrate_depth -- through the trilinear TSDF; a hit is the first front-face zero crossing between two samples whose 8
 * corner weights are all > 0.  Hit: point (x, y, z, 0) in the camera frame, normal (nx, ny, nz, 1); miss: both all zero.
 * step_factor: the fine step in units of the smallest voxel size (KinFu: 0.75); trunc: the truncation distance in metres.
 * A corner weight that is not > 0 (0, negative, NaN) makes a sample invalid.  SOBFU_E_BADARG, before any launch: X, Y or Z < 2, rows or
 * cols < 1, a step below cols * 16 or a step / pointer off 16 bytes, a voxel size, trunc or step_factor that is not positive and finite,
 * fx or fy 0, non-finite intrinsics, or a NaN / Inf anywhere in R or t (as sobfu_hip_mesh_render).  SOBFU_E_UNSUPPORTED: a step so small
 * that the box diagonal takes 10^6 fine steps or more. */
int sobfu_hip_raycast(const float* d_vol, int X, int Y, int Z, float vsx, float vsy, float vsz, float trunc, const float R[9],
                      const float t[3], float fx, float fy, float cx, float cy, int rows, int cols, float step_factor, float* d_points,
                      int points_step, float* d_normals, int normals_step, void* stream);
/* renderImage: grey = 0.2 + 0.8 max(0, n . normalize(light - point)), light in the camera frame; misses are (0, 0, 0, 0). */
int sobfu_hip_render_image(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols,
                           float lx, float ly, float lz, uint8_t* d_image, int image_step, void* stream);
/* renderTangentColors: (r, g, b) = (n * 0.5 + 0.5) * 255; misses are (0, 0, 0, 0). */
int sobfu_hip_render_normals(const float* d_normals, int normals_step, int rows, int cols, uint8_t* d_image, int image_step,
                             void* stream);

/* ------------------------------------------------------------------------------------------------------
 * colour -- the reference's SobFusion::operator()(const Depth&, const Image&) (include/sobfu/sob_fusion.hpp:44) takes a colour image
 * and drops it (src/sobfu/sob_fusion.cpp:71).  Colour volume: one uchar4 (b, g, r, a) per voxel (kfusion::RGB order, a = colour
 * weight, 0 = no colour), dense, x fastest, like the TSDF volumes; colour frames: pitched 8-bit BGRA registered to the depth camera.
 * The rules are in sobfu_amd/csrc/colour_kernels.hip.  Every argument is checked before any device call.
 * ---------------------------------------------------------------------------------------------------- */
/* integrate_colour: fuses one colour frame into d_colour through the TSDF about to be fused (d_tsdf: phi_n o psi, phi_n, or phi_global
 * on frame 0) and psi (NULL = identity): a voxel that is observed in d_tsdf with |tsdf| < 1 takes the pixel psi(x) projects to with
 * vol2cam = (R row-major, t) and the intrinsics of sobfu_hip_integrate_depth.  Running average c' = rint((c a + c_new) / (a + 1)),
 * a' = min(a + 1, cap); 1 <= cap <= 255 (the frame driver: min(TSDF_MAX_WEIGHT, 255)). */
int sobfu_hip_integrate_colour(const uint8_t* d_image, int image_step, int rows, int cols, const float* d_tsdf, const float* d_psi,
                               uint8_t* d_colour, int X, int Y, int Z, const float voxel_size[3], const float R[9], const float t[3],
                               float fx, float fy, float cx, float cy, int cap, void* stream);
/* apply_colour: d_colour_warped(y) = sample(d_colour, psi_inv(y)) -- the colour counterpart of sobfu_hip_apply.  The sampler is
 * trilinear over the corners with a > 0, renormalised; no corner with colour gives (0, 0, 0, 0), any other result has a = 1. */
int sobfu_hip_apply_colour(const uint8_t* d_colour, uint8_t* d_colour_warped, const float* d_psi_inv, int X, int Y, int Z, void* stream);
/* sample_colour: rows x cols float4 points (pitched; a flat list is rows = 1) of a frame whose pose from volume metres is (R, t) -- a
 * raycast's vol2cam, or the marching-cubes pose with mc_vertices = 1, which undoes the vertices' (x, -y, -z) -- sampled from d_colour
 * into BGRA d_out.  d_normals (optional): a point whose normal.w == 0 (a raycast miss) gives (0, 0, 0, 0). */
int sobfu_hip_sample_colour(const uint8_t* d_colour, int X, int Y, int Z, const float voxel_size[3], const float R[9], const float t[3],
                            int mc_vertices, const float* d_points, int points_step, const float* d_normals, int normals_step, int rows,
                            int cols, uint8_t* d_out, int out_step, void* stream);
/* render_colour: a hit with colour (d_colour_image alpha != 0) is colour * (0.2 + 0.8 max(0, n . normalize(light - point))), a hit
 * without colour is sobfu_hip_render_image's grey, a miss is (0, 0, 0, 0). */
int sobfu_hip_render_colour(const float* d_points, int points_step, const float* d_normals, int normals_step, const uint8_t* d_colour_image,
                            int colour_step, int rows, int cols, float lx, float ly, float lz, uint8_t* d_image, int image_step,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------
 * points through the deformation -- the canonical mesh carried to the live frame (no reference counterpart: the reference's live meshes
 * are fresh marching-cubes runs on warped volumes).  Point and normal lists: n dense float4, 16-byte aligned.  (R row-major, t), voxel_size
 * and mc_vertices as in sobfu_hip_sample_colour.  The rules are in sobfu_amd/csrc/warp_points_kernels.hip.  Every argument is checked
 * before any device call; n = 0 succeeds and launches nothing.
 * ---------------------------------------------------------------------------------------------------- */
/* warp_points: point v -> v + the displacement of d_psi (float4 per voxel, absolute positions in voxel units) interpolated at v, w = 1;
 * normals (optional: d_normals and d_normals_out are both given or both NULL) through the cofactor matrix of psi's Jacobian in the same
 * cell, normalised, w = 1; a zero normal stays (0, 0, 0, 1).  Outputs may be the inputs. */
int sobfu_hip_warp_points(const float* d_psi, int X, int Y, int Z, const float voxel_size[3], const float R[9], const float t[3],
                          int mc_vertices, const float* d_points, const float* d_normals, int n, float* d_points_out, float* d_normals_out,
                          void* stream);
/* sample_tsdf: the trilinear TSDF of d_vol ({tsdf, weight} per voxel) at the points, one float per point in units of the truncation
 * distance; NaN where one of the eight corners has weight <= 0 (the raycaster's validity rule). */
int sobfu_hip_sample_tsdf(const float* d_vol, int X, int Y, int Z, const float voxel_size[3], const float R[9], const float t[3],
                          int mc_vertices, const float* d_points, int n, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * camera tracking -- kfusion::cuda::ProjectiveICP (include/kfusion/cuda/projective_icp.hpp, src/kfusion/projective_icp.cpp) and the image
 * helpers of include/kfusion/cuda/imgproc.hpp it needs (depthBuildPyramid, computePointNormals, computeNormalsAndMaskDepth,
 * resizeDepthNormals, resizePointsNormals), which the reference declares but never calls.  Depth: pitched uint16 mm; points / normals:
 * pitched float4 (16-byte aligned); invalid pixels are NaN (the raycaster's all-zero misses are invalid too).  The rules are in
 * sobfu_amd/csrc/icp_kernels.hip.  Every argument is checked before any device call.
 * ---------------------------------------------------------------------------------------------------- */
/* depthBuildPyramid: d_dst is (rows / 2) x (cols / 2); sigma_depth in metres. */
int sobfu_hip_depth_pyramid(const uint16_t* d_src, int src_step, int rows, int cols, uint16_t* d_dst, int dst_step, float sigma_depth,
                            void* stream);
/* computePointNormals: camera-frame points and normals of a depth image with intrinsics (fx, fy, cx, cy). */
int sobfu_hip_compute_point_normals(const uint16_t* d_depth, int depth_step, int rows, int cols, float fx, float fy, float cx, float cy,
                                    float* d_points, int points_step, float* d_normals, int normals_step, void* stream);
/* computeNormalsAndMaskDepth: normals of a depth image; the depth is zeroed in place where the normal is NaN. */
int sobfu_hip_compute_normals_mask_depth(uint16_t* d_depth, int depth_step, int rows, int cols, float fx, float fy, float cx, float cy,
                                         float* d_normals, int normals_step, void* stream);
/* resizeDepthNormals / resizePointsNormals: rows x cols in, (rows / 2) x (cols / 2) out. */
int sobfu_hip_resize_depth_normals(const uint16_t* d_depth, int depth_step, const float* d_normals, int normals_step, int rows, int cols,
                                   uint16_t* d_depth_out, int depth_out_step, float* d_normals_out, int normals_out_step, void* stream);
int sobfu_hip_resize_points_normals(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols,
                                    float* d_points_out, int points_out_step, float* d_normals_out, int normals_out_step, void* stream);
/* One pyramid level of an ICP pair: current and previous frame, both rows x cols.  curr / prev are float4 points (points mode) or uint16
 * depth (depth mode); ncurr / nprev are float4 normals.  Steps in bytes. */
typedef struct {
    const void* curr;
    int curr_step;
    const float* ncurr;
    int ncurr_step;
    const void* prev;
    int prev_step;
    const float* nprev;
    int nprev_step;
    int rows, cols;
} sobfu_hip_icp_level;
/* Device workspace of sobfu_hip_icp_step / _estimate (the per-workgroup partial sums). */
size_t sobfu_hip_icp_workspace_bytes(void);
/* One correspondence + reduction pass of pyramid level `level_index` (intrinsics (fx, fy, cx, cy) / 2^level_index) at the pose d_aff
 * (16 floats on the device, row-major 4 x 4, maps the current frame into the previous one).  d_sums (device, 29 doubles): the 21
 * upper-triangular entries of A (row-major), b (6), the inlier count and the sum of squared residuals.  d_codes (optional): rows x cols
 * uint8 per-pixel codes (0 inlier, 40 invalid source, 80 projects behind / outside, 120 invalid target, 160 too far, 200 angle).
 * depth_mode: 0 = points, 1 = depth; angle_thres in radians. */
int sobfu_hip_icp_step(const sobfu_hip_icp_level* level, int level_index, int depth_mode, float fx, float fy, float cx, float cy,
                       float dist_thres, float angle_thres, const float* d_aff, void* d_workspace, size_t workspace_bytes,
                       double* d_sums, uint8_t* d_codes, int codes_step, void* stream);
/* The whole coarse-to-fine estimate (ProjectiveICP::estimateTransform): levels[0] is full resolution with intrinsics (fx, fy, cx, cy),
 * levels[l] is half of levels[l - 1]; 1 <= n_levels <= 4; iters[l] iterations at level l, from level n_levels - 1 down to 0, starting
 * from identity.  Writes the pose (16 floats, row-major 4 x 4: current frame -> previous frame) to d_pose and 0 to *d_status, or, on the
 * first singular system, 0x10000 | level << 8 | iteration to *d_status and leaves the pose of the iteration before.  d_trace (optional):
 * (inliers, rms residual) per iteration, in launch order.  Enqueues only: no synchronisation, allocation or copy -- the caller reads the
 * results (the chain can be captured into a graph). */
int sobfu_hip_icp_estimate(const sobfu_hip_icp_level* levels, int n_levels, const int iters[4], int depth_mode, float fx, float fy, float cx,
                           float cy, float dist_thres, float angle_thres, void* d_workspace, size_t workspace_bytes, float* d_pose,
                           int* d_status, float* d_trace, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * native multi-GPU loop: one rank per z-slab, RCCL halo exchange issued from C++ and overlapped with the interior
 * compute (no reference counterpart; schedule documented in sobfu_amd/tiled.py)
 * ---------------------------------------------------------------------------------------------------- */
#define SOBFU_E_RCCL (-4) /* RCCL not loaded / an RCCL call failed (details on stderr) */
typedef struct sobfu_hip_tiled sobfu_hip_tiled; /* opaque */
/* dlopen()s the RCCL library the host process already uses (e.g. <torch>/lib/librccl.so); must precede the rest. */
int sobfu_hip_tiled_load_rccl(const char* librccl_path);
/* ncclGetUniqueId on one rank; the caller broadcasts the 128 bytes to all ranks (any transport). */
int sobfu_hip_tiled_unique_id(char out[128]);
/* Collective over all `world` ranks (ncclCommInitRank).  The volume's Z planes are split as evenly as possible.
 * An all-zero unique_id creates a communicator-less handle (no collective): the slab layout and launch schedule of
 * (world, rank) with the transport left to sobfu_hip_tiled_set_transport -- or to nobody, for compute-only timing. */
int sobfu_hip_tiled_create(sobfu_hip_tiled** out, int X, int Y, int Z, int world, int rank, const char unique_id[128],
                           const sobfu_hip_solver_params* params);
int sobfu_hip_tiled_destroy(sobfu_hip_tiled* t);
/* The same for a Px x Py x Pz grid of tiles (rank = cx + Px * (cy + Py * cz); the cells of every axis are split as evenly as
 * possible; every split axis needs >= 4 cells per tile).  Px = Py = 1 is the z-slab layout of sobfu_hip_tiled_create. */
int sobfu_hip_tiled_create3(sobfu_hip_tiled** out, int X, int Y, int Z, int Px, int Py, int Pz, int rank, const char unique_id[128],
                            const sobfu_hip_solver_params* params);
/* out[24] = per axis (x, y, z): tile grid P, tile coordinates c, owned global range [g0, g1), halo cells lo / hi, local extent L,
 * global coordinate `base` of local cell 0 -- eight triples in that order. */
int sobfu_hip_tiled_layout3(const sobfu_hip_tiled* t, int out[24]);
/* owned planes [z0, z1) of this rank, halo planes below / above, slab thickness Lz, global z of local plane 0 */
int sobfu_hip_tiled_layout(const sobfu_hip_tiled* t, int* z0, int* z1, int* lo, int* hi, int* Lz, int* zbase);
/* n_iters iterations on this rank's slab (collective).  Local slabs: phi_global / phi_n o psi float2 (X, Y, Lz), psi
 * float4 (X, Y, Lz) exact on owned +-1 planes on entry and exit; phi_n: the whole float2 (X, Y, Z) volume. */
int sobfu_hip_tiled_iterate(sobfu_hip_tiled* t, const float* d_phi_global_local, const float* d_phi_n_full,
                            float* d_phi_n_psi_local, float* d_psi_local, int n_iters, sobfu_hip_solver_report* report,
                            float* per_iter_max_norm, void* stream);
/* The same loop in pieces, as sobfu_hip_solver_begin / step / end (collective; step ENQUEUES n_iters more iterations and returns
 * without synchronising; end synchronises, reduces the max-norm rows the loop has not yet made global, finds the iteration the
 * reference stops at and rebuilds the caller's arrays). */
int sobfu_hip_tiled_begin(sobfu_hip_tiled* t, const float* d_phi_global_local, const float* d_phi_n_full, float* d_phi_n_psi_local,
                          float* d_psi_local, int max_iters, void* stream);
int sobfu_hip_tiled_step(sobfu_hip_tiled* t, int n_iters, void* stream);
int sobfu_hip_tiled_end(sobfu_hip_tiled* t, sobfu_hip_solver_report* report, float* per_iter_max_norm, void* stream);
/* Optional: a second communicator (a second ncclGetUniqueId, broadcast like the first) and a stream of its own for the max-norm
 * all-reduce of a live threshold.  With it the reduction of iteration k's row is issued right after that iteration's pass B and
 * runs beside iteration k+1 (the late gate only needs it by pass B of k+2) without ever queueing behind a halo exchange on the
 * main communicator; without it the reduction shares the exchange's communicator (comm stream, or in line when serial). */
int sobfu_hip_tiled_add_reduce_comm(sobfu_hip_tiled* t, const char unique_id[128]);
/* How a Z-SLAB iteration is issued on the RCCL / callback transports (the results never depend on it; 3-D tiles and the direct
 * transport have one way): 0 = built-in heuristic (by slab thickness), 1 = exchange overlapped with the interior compute, pass A
 * split into boundary + interior launches, 2 = overlapped, pass A in one launch, 3 = serial (pass A, exchange, pass B in line on one
 * stream: no cross-stream events -- the better choice when the exchange is fast).  Which one wins depends on the machine's
 * exchange latency; sobfu_amd.tiled.NativeTiledSolver.autotune times them. */
int sobfu_hip_tiled_set_schedule(sobfu_hip_tiled* t, int schedule);
/* diagnostics: host microseconds per iteration the last sobfu_hip_tiled_iterate spent ISSUING its loop (launches, events,
 * RCCL calls) -- against the measured time per iteration it tells whether a thin slab is host-bound */
double sobfu_hip_tiled_last_enqueue_us(const sobfu_hip_tiled* t);
/* One halo message: `count` floats from d_send + send_off of this rank to d_recv + recv_off of rank `peer`'s matching message
 * (every pair of neighbours exchanges exactly one message in each direction per exchange). */
typedef struct {
    int peer;
    size_t send_off, recv_off, count; /* in floats */
} sobfu_hip_tiled_msg;
/* The messages of one exchange and the boxes (6 ints each: x0, x1, y0, y1, z0, z1, local cells) they are packed from / scattered
 * to; returns their number (z-slabs on the RCCL transport send the same cells as plane ranges of the field itself).
 * WHAT ACTUALLY TRAVELS on the RCCL / callback transports of a 3-D tile: only the first *n_packed of these messages (x / y faces and
 * all edge strips) go through the packed send / receive buffers with the offsets and counts listed here.  The z-face messages that
 * follow them in this list describe the cells (their boxes are right), but they are NOT packed: they travel IN PLACE as 4 whole
 * padded planes of the nabla_U array (Lx x Ly x 4 cells) -- the list sobfu_hip_tiled_messages_inplace returns, with offsets into the
 * field itself.  A transport that pre-posts its requests (MPI persistent requests, ...) must build them from BOTH lists. */
int sobfu_hip_tiled_messages(const sobfu_hip_tiled* t, sobfu_hip_tiled_msg* msgs, int* send_boxes, int* recv_boxes, int max_msgs);
/* The in-place list of one exchange (3-D tiles: the z faces; empty for z-slabs, whose plane messages are built per call) and, in
 * *n_packed, how many messages of sobfu_hip_tiled_messages go through the buffers; returns the length of the in-place list. */
int sobfu_hip_tiled_messages_inplace(const sobfu_hip_tiled* t, sobfu_hip_tiled_msg* msgs, int max_msgs, int* n_packed);
/* Timing of the SERIAL schedule's pieces with HIP events on the loop's stream around every stride-th iteration (0 = off;
 * max_samples events sets are created here, outside any timed region): ms[0] pass A, ms[1] the exchange (pack + transfer +
 * unpack, including the wait for the peers), ms[2] pass B -- sums over `samples` iterations since the last reset.  Call
 * get_profile after the stream has been synchronised.  An event between two kernels drains the pipeline: time a profiled run for
 * its split, not for its wall time. */
int sobfu_hip_tiled_set_profiling(sobfu_hip_tiled* t, int stride, int max_samples);
int sobfu_hip_tiled_get_profile(sobfu_hip_tiled* t, float ms[3], int* samples, int reset);
/* Pluggable transport for communicator-less handles (MPI, an in-process loopback for tests, ...).  `exchange` must deliver every
 * message: msgs[i].count floats at d_send + msgs[i].send_off arrive at d_recv + recv_off of the message rank msgs[i].peer posts
 * for this rank; `allreduce_max` must leave the element-wise maximum over all ranks in d_buf.  Both are called on the host in
 * launch order and must order their work after everything already enqueued on `stream` and before anything enqueued on it later.
 * CALLS PER EXCHANGE: z-slabs: one, with d_send == d_recv == the field (planes in place).  3-D tiles: UP TO TWO -- first the packed
 * list (d_send = the send buffer, d_recv = the receive buffer, the first n_packed messages of sobfu_hip_tiled_messages), then the
 * in-place list (d_send == d_recv == the nabla_U array, the messages of sobfu_hip_tiled_messages_inplace: whole-plane offsets and
 * counts); a list that is empty is not called.  A call never carries more than one message per peer; the two calls of one exchange
 * may name the same peer.  Every rank makes the same sequence of calls, so a transport may match them by call order. */
typedef int (*sobfu_hip_tiled_exchange_fn)(void* ctx, int rank, const float* d_send, float* d_recv, const sobfu_hip_tiled_msg* msgs,
                                           int n_msgs, void* stream);
typedef int (*sobfu_hip_tiled_allreduce_fn)(void* ctx, int rank, uint32_t* d_buf, size_t n, void* stream);
int sobfu_hip_tiled_set_transport(sobfu_hip_tiled* t, sobfu_hip_tiled_exchange_fn exchange, sobfu_hip_tiled_allreduce_fn allreduce_max,
                                  void* ctx);
/* DIRECT transport (communicator-less handles): the halo cells travel as plain stores from pass A's launch into the neighbours'
 * own nabla_U arrays, peer-mapped over xGMI -- no pack / unpack kernels, no communication launch, no collective in the loop; arrival
 * flags and the max-norm rows travel the same way (see sobfu_amd/csrc/tiled_capi.hip).  Every rank exports two device
 * allocations (sobfu_hip_tiled_exports_get; across processes: sobfu_hip_ipc_export -> 64-byte handles -> sobfu_hip_ipc_open on the
 * other side), hands the pointers of ALL other ranks -- valid in ITS process -- to sobfu_hip_tiled_connect, and every rank must have
 * connected (a barrier of the caller's) before any begins a solve.  A peer whose flag does not arrive within
 * SOBFU_TILED_DEADLINE_S (default 30 s) is recorded instead of waited for: _end / _status return SOBFU_E_TIMEOUT. */
#define SOBFU_E_TIMEOUT (-5) /* a peer did not answer within the deadline; the handle is dead (destroy it) */
typedef struct {
    void* arena;           /* ONE allocation (what crosses the process boundary): the two halves of the double-buffered nabla_U tile
                              (12-byte cells, local extents) and the global max-norm rows (256 uint32 per iteration) ... */
    size_t nabla_u_off[2]; /* ... at these byte offsets */
    size_t rows_off;
    void* flags;           /* a second allocation: arrival flags, one uint32 per rank (uncached) */
} sobfu_hip_tiled_exports;
int sobfu_hip_tiled_exports_get(const sobfu_hip_tiled* t, sobfu_hip_tiled_exports* out);
int sobfu_hip_tiled_connect(sobfu_hip_tiled* t, int n_peers, const int* peer_ranks, const sobfu_hip_tiled_exports* peers);
int sobfu_hip_ipc_export(const void* d_ptr, char handle[64]);
int sobfu_hip_ipc_open(const char handle[64], void** d_ptr);
int sobfu_hip_ipc_close(void* d_ptr);
/* 0, or SOBFU_E_TIMEOUT with the rank that was missing (-1: unknown) */
int sobfu_hip_tiled_status(sobfu_hip_tiled* t, int* missing_peer);
/* Iterations ONE solve may run on this handle: the direct transport's max-norm rows are mapped by the peers, so their number is
 * fixed when the handle is created (16384); other transports grow their rows on demand. */
int sobfu_hip_tiled_max_iterations(const sobfu_hip_tiled* t);
/* What the runtime says about the path from `device` to `peer_device`: out = {hipDeviceCanAccessPeer, link type
 * (hipExtGetLinkTypeAndHopCount: 0 HyperTransport, 1 QPI, 2 PCIe, 3 InfiniBand, 4 xGMI), hops, hipDevP2PAttrPerformanceRank}; -1 = unknown. */
int sobfu_hip_p2p_info(int device, int peer_device, int out[4]);
/* Diagnostics of the direct transport (every rank of the world makes the same calls in the same order, outside a solve):
 *   wait_stats  microseconds the signalling workgroup of pass A has spent waiting for its peers' arrival flags, and how many waits --
 *               the part of the exchange an iteration did NOT hide behind its own compute
 *   pingpong    `reps` flag round trips between rank_a and rank_b inside one launch (the other ranks only advance their sequence numbers)
 *   probe_push  pass A's push boxes alone (the production store path into the peers' halo cells + signalling), `reps` launches */
int sobfu_hip_tiled_wait_stats(sobfu_hip_tiled* t, double* wait_us, int* waits, int reset);
int sobfu_hip_tiled_pingpong(sobfu_hip_tiled* t, int rank_a, int rank_b, int reps, void* stream);
int sobfu_hip_tiled_probe_push(sobfu_hip_tiled* t, int reps, void* stream);
/* test hooks: wait = 0 turns the in-kernel wait for the peers' flags off (a harness that drives N ranks from ONE process steps
 * them phase by phase with host barriers instead: phase 0 = pass A incl. the pushes, phase 1 = pass B; after the last iteration
 * phase 2 = the end-of-solve handshake, then sobfu_hip_tiled_end) */
int sobfu_hip_tiled_set_wait(sobfu_hip_tiled* t, int wait);
int sobfu_hip_tiled_step_phase(sobfu_hip_tiled* t, int phase, void* stream);
/* bring-up helpers: the loop's halo exchange on a caller-provided 12-byte tile field (planes < 4: z-slabs only); a self
 * send/recv and a MAX all-reduce through the same RCCL entry points (usable with a single rank) */
int sobfu_hip_tiled_exchange(sobfu_hip_tiled* t, float* d_field3, int planes, void* stream);
int sobfu_hip_tiled_self_sendrecv(sobfu_hip_tiled* t, const float* d_src, float* d_dst, size_t n, void* stream);
int sobfu_hip_tiled_allreduce_max_u32(sobfu_hip_tiled* t, uint32_t* d_buf, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * mesh distance  (no counterpart in the reference; sobfu_amd/csrc/mesh_distance_kernels.hip)
 * Exact Euclidean distances from points to an indexed triangle mesh: vertices as n_vertices dense float4 (x, y, z, w; w ignored, 16-byte
 * aligned like the other point lists), faces as n_triangles x 3 int32.  Per point: dist = the distance to the nearest triangle (fp32 rule:
 * sobfu_amd/csrc/sobfu_mesh_distance.hpp), tri = the lowest triangle index at that distance, closest = that triangle's closest point
 * (x, y, z, 1).  The answer is the same bit for bit whichever mode finds it and from run to run.
 * ---------------------------------------------------------------------------------------------------- */
/* Host only: the uniform grid over a mesh whose box is bbox = {min x, y, z, max x, y, z} -> origin, cell edge h and dims (<= 128 each;
 * dims * h covers the box).  cell = 0: cells along the longest extent = clamp(ceil(sqrt(n_triangles) / 4), 1, 128); cell > 0: that edge
 * (enlarged where it would need more than 128 cells).  SOBFU_E_BADARG: a non-finite or inverted box, a negative count or cell. */
int sobfu_hip_mesh_grid_plan(const float bbox[6], int n_triangles, float cell, float origin[3], float* h, int dims[3]);
/* Bytes of the caller-kept workspace of a grid with room for max_refs triangle references (0: invalid dims). */
size_t sobfu_hip_mesh_grid_workspace_bytes(const int dims[3], int max_refs);
/* Builds the grid into d_workspace (16-byte aligned): count, scan, fill.  SYNCHRONISES the stream once, after the count: *h_refs = the
 * references the mesh needs.  SOBFU_E_UNSUPPORTED with *h_refs > max_refs: build again with a workspace of that size.  SOBFU_E_BADARG
 * (after the synchronisation) for a face index outside [0, n_vertices) or a non-finite corner; a workspace whose build did not return 0
 * is not marked as built and every query through it answers (+Inf, -1). */
int sobfu_hip_mesh_grid_build(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, const float origin[3], float h,
                              const int dims[3], void* d_workspace, size_t workspace_bytes, int max_refs, int* h_refs, void* stream);
#define SOBFU_MESH_DISTANCE_AUTO 0  /* the grid; brute force for meshes of at most 64 triangles */
#define SOBFU_MESH_DISTANCE_GRID 1
#define SOBFU_MESH_DISTANCE_BRUTE 2 /* every point against every triangle */
/* n points (dense float4) against the mesh and plan the workspace was built with (the same arrays, unchanged).  max_dist <= 0 or +Inf:
 * unlimited; else a point farther than max_dist gets dist = +Inf, tri = -1, closest = (0, 0, 0, 0).  ring_cap: shells of cells a point
 * may walk before it is finished by brute force (0 = default, 8).  d_closest may be NULL; d_unresolved: n ints of scratch (may be NULL
 * for SOBFU_MESH_DISTANCE_BRUTE).  No triangles: every point gets (+Inf, -1).  n = 0 succeeds and launches nothing.  Asynchronous. */
int sobfu_hip_mesh_distance(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                            int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist,
                            int mode, int ring_cap, float* d_dist, int* d_tri, float* d_closest, int* d_unresolved, void* stream);
/* How many points of the last sobfu_hip_mesh_distance through this workspace hit the ring cap (synchronises the stream). */
int sobfu_hip_mesh_distance_unresolved(const void* d_workspace, int* h_count, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * mesh alignment  (no counterpart in the reference; sobfu_amd/csrc/mesh_align_kernels.hip)
 * Point-to-plane ICP of n points (dense float4, w ignored) against the mesh and grid of sobfu_hip_mesh_grid_build: per iteration the
 * points go through the pose in d_pose (16 floats, row-major 4 x 4, source -> target frame; rows 0..2 are read and written), their exact
 * nearest triangles come from sobfu_hip_mesh_distance (max_dist, mode, ring_cap as there), the 29 fp64 sums of the normal equations
 * are reduced without floating-point atomics and one workgroup solves and updates the pose.  Bitwise reproducible run to run.
 * Every argument is checked before any device call (SOBFU_E_BADARG); n = 0 succeeds, launches nothing and writes nothing.
 * ---------------------------------------------------------------------------------------------------- */
/* Bytes of the caller-kept workspace (16-byte aligned) for n points: the partial sums, the transformed points and the query's
 * dist / tri / closest / unresolved arrays.  0 for n < 0. */
size_t sobfu_hip_mesh_align_workspace_bytes(int n);
/* One transform + query + sums at the pose in d_pose -> d_sums, 29 doubles laid out as sobfu_hip_icp_step's: the 21 upper-triangular
 * J_i J_j, the 6 J_i r, the inlier count, the sum of r r.  No solve; the pose is only read.  Asynchronous. */
int sobfu_hip_mesh_align_step(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                              int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist, int mode,
                              int ring_cap, const float* d_pose, void* d_workspace, size_t workspace_bytes, double* d_sums, void* stream);
/* `iters` (0..1000) iterations from the pose already in d_pose; enqueues only.  dof: 6 rigid, 3 translation only.  eps_rot (radians),
 * eps_trans (metres) >= 0: the loop stops once an update is below BOTH (0: never).  *d_status: 0 every iteration ran;
 * 0x20000 | iterations done: stopped by the gate; 0x10000 | iteration: the solve of that iteration failed (a pivot <= 0 or non-finite:
 * no inliers, or a geometry that does not fix the pose) and the pose of the iteration before is left in place.  d_trace (may be NULL):
 * 4 floats per iteration -- inliers, rms residual, |w|, |t_inc| -- written for the iterations that ran. */
int sobfu_hip_mesh_align_estimate(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                                  int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, float max_dist,
                                  int mode, int ring_cap, int iters, int dof, float eps_rot, float eps_trans, void* d_workspace, size_t workspace_bytes,
                                  float* d_pose, int* d_status, float* d_trace, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * mesh rays  (no counterpart in the reference; sobfu_amd/csrc/mesh_ray_kernels.hip)
 * Rays against the mesh and grid of sobfu_hip_mesh_grid_build (the same arrays and plan, unchanged; the workspace is only read).  Per ray
 * o + t d, d not normalised: t = the smallest parameter in (t_min, t_max] at which it meets a triangle (the watertight fp32 rule of
 * sobfu_amd/csrc/sobfu_mesh_ray.hpp, two-sided), tri = the lowest triangle index at that t, bary = (u, v), the weights of the triangle's
 * second and third corner, side = +1 where the ray meets the face whose corners run counter-clockwise as seen from its origin, -1 for
 * the other face.  A miss is (+Inf, -1, (0, 0), 0): no triangles, a workspace that is not marked as built, a ray that passes the grid's
 * box, a zero or non-finite origin or direction.  The answer is the same bit for bit whichever mode finds it and from run to run.
 * Every argument is checked before any device call (SOBFU_E_BADARG).  Asynchronous.
 * ---------------------------------------------------------------------------------------------------- */
/* n rays as two dense float4 arrays (w ignored).  t_min: finite; t_max <= 0 or +Inf: unlimited.  mode: SOBFU_MESH_DISTANCE_AUTO (the grid
 * walk; brute force for meshes of at most 64 triangles), _GRID or _BRUTE.  d_bary (float2 per ray) and d_side (int8 per ray) may be NULL.
 * n = 0 succeeds and launches nothing. */
int sobfu_hip_mesh_raycast(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                           int n_triangles, const float origin[3], float h, const int dims[3], const float* d_origins, const float* d_dirs, int n,
                           float t_min, float t_max, int mode, float* d_t, int* d_tri, float* d_bary, int8_t* d_side, void* stream);
/* The mesh seen by a pinhole camera: pixel (u, v) casts ((u - cx) / fx, (v - cy) / fy, 1) from the camera of (R row-major, t), mesh frame
 * -> camera frame -- the pose argument of sobfu_hip_raycast and sobfu_hip_integrate_depth -- so the ray parameter is the depth z, limited
 * to (z_min, z_max] as t is above.  Outputs, pitched (step in bytes), each may be NULL:
 *   d_depth    uint16 millimetres, rint(1000 z); 0 for a miss and for z beyond 65.535 m
 *   d_points   float4 (x, y, z, 0) in the camera frame, d_normals float4 (nx, ny, nz, 1): sobfu_hip_raycast's format, a miss all zero.
 *              The normal is the barycentric mix of d_vertex_normals (dense float4 per vertex) or, without them, the face's; turned to
 *              face the camera, rotated into its frame and normalised
 *   d_colour   8-bit BGRA: the barycentric mix of d_vertex_colours (4 bytes per vertex, kfusion::RGB order), rounded to nearest, alpha
 *              255; a miss (0, 0, 0, 0).  Needs d_vertex_colours
 *   d_tri      int32, the triangle's index; a miss -1 */
int sobfu_hip_mesh_render(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                          const float origin[3], float h, const int dims[3], const float* d_vertex_normals, const uint8_t* d_vertex_colours,
                          const float R[9], const float t[3], float fx, float fy, float cx, float cy, int rows, int cols, float z_min, float z_max,
                          uint16_t* d_depth, int depth_step, float* d_points, int points_step, float* d_normals, int normals_step,
                          uint8_t* d_colour, int colour_step, int32_t* d_tri, int tri_step, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * mesh voxelisation  (no counterpart in the reference; sobfu_amd/csrc/mesh_voxel_kernels.hip)
 * A closed mesh, with the grid of sobfu_hip_mesh_grid_build (the same arrays and plan, unchanged; the workspace is only read) and its
 * vertices in the volume's frame, into a signed TSDF volume, and the inside / outside test behind it.  A point is inside iff the row
 * through it along +x crosses the mesh an odd number of times beyond it (the exact counting rule of sobfu_amd/csrc/sobfu_mesh_parity.hpp);
 * a row that crosses the mesh an odd number of times altogether is open: the mesh is not closed there, and signs along it mean nothing.
 * mode is SOBFU_MESH_DISTANCE_AUTO (the grid; brute force for meshes of at most 64 triangles), _GRID or _BRUTE and never changes a bit of
 * the output, nor does the run.  A workspace that is not marked as built, or no triangles: every voxel is (1, 1), every point outside,
 * nothing open.  Every argument is checked before any device call (SOBFU_E_BADARG).  Asynchronous.
 * ---------------------------------------------------------------------------------------------------- */
/* Bytes of the caller-kept workspace (16-byte aligned) of sobfu_hip_mesh_voxelise: the sign bits, ceil(X / 32) words per row.  0 for
 * X outside [1, 512], Y or Z < 1, or more than INT_MAX rows. */
size_t sobfu_hip_mesh_voxelise_workspace_bytes(int X, int Y, int Z);
/* d_vol (X * Y * Z float2 {tsdf, weight}, X <= 512): voxel (i, j, k) has its centre at (i vs + vs / 2) per axis, in fp32; d = its exact
 * distance to the nearest triangle (sobfu_mesh_distance.hpp), s = -d inside and d outside; it stores tsdf = clamp(s / trunc, -1, 1) and
 * weight = s > -eta ? 1 : 0, as sobfu_hip_init_sphere does.  *d_open_rows (device): the number of open rows of the volume. */
int sobfu_hip_mesh_voxelise(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                            int n_triangles, const float origin[3], float h, const int dims[3], float* d_vol, int X, int Y, int Z,
                            const float voxel_size[3], float trunc, float eta, int mode, void* d_workspace, size_t workspace_bytes,
                            int* d_open_rows, void* stream);
/* n points (dense float4, w ignored) -> d_inside[i] = 1 inside, 0 outside; d_open[i] = 1 where the point's row is open.  n = 0 succeeds
 * and launches nothing. */
int sobfu_hip_mesh_inside(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                          int n_triangles, const float origin[3], float h, const int dims[3], const float* d_points, int n, uint8_t* d_inside,
                          uint8_t* d_open, int mode, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * generalised winding numbers  (no counterpart in the reference; sobfu_amd/csrc/mesh_winding_kernels.hip)
 * Inside / outside for meshes that are not closed: w(p) is 1 inside and 0 outside a closed, outward-oriented mesh, varies smoothly
 * across holes, and "inside iff w > 1 / 2" is defined for any oriented triangle soup (Jacobson et al. 2013).  Computed from the mesh's
 * boundary: w = N + the solid angles of the strips from the boundary edges to infinity along -x, over 4 pi, with N the signed number of
 * crossings of the row beyond p (the counting rule of sobfu_mesh_parity.hpp with signs; sobfu_amd/csrc/sobfu_mesh_winding.hpp).  fp64,
 * accumulated in index order: the same bits from run to run and for every walk mode.  A workspace that is not marked as built, or no
 * triangles: w = 0 everywhere.  Every argument is checked before any device call (SOBFU_E_BADARG).
 * ---------------------------------------------------------------------------------------------------- */
/* Host only: the boundary chain of n_triangles faces (3 ints each, host memory) -> the (u, v, k) with u < v and
 * k = (#triangles that run u -> v) - (#that run v -> u) != 0, sorted by (u, v), 3 ints per edge into h_edges; *h_count = their number.
 * h_edges = NULL (capacity 0) only counts.  SOBFU_E_BADARG: an index outside [0, n_vertices); SOBFU_E_UNSUPPORTED: capacity (in
 * edges) is smaller than *h_count. */
int sobfu_hip_mesh_boundary(const int* h_faces, int n_triangles, int n_vertices, int* h_edges, int capacity, int* h_count);
#define SOBFU_MESH_WINDING_BOUNDARY 0 /* crossings + boundary strips; the definition where a point lies on a seam */
#define SOBFU_MESH_WINDING_SUM 1      /* the definition: every triangle's solid angle; d_boundary is not read */
/* n points (dense float4, w ignored) -> d_w[i], the winding number as a float.  d_boundary: n_boundary edges of the chain as two float4
 * each, (u.x, u.y, u.z, k) and (v.x, v.y, v.z, .), device memory (NULL for none).  mode: SOBFU_MESH_WINDING_*; walk: the crossing
 * walk, SOBFU_MESH_DISTANCE_AUTO, _GRID or _BRUTE (never changes a bit).  n = 0 succeeds and launches nothing.  Asynchronous. */
int sobfu_hip_mesh_winding(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                           int n_triangles, const float origin[3], float h, const int dims[3], const float* d_boundary, int n_boundary,
                           const float* d_points, int n, float* d_w, int mode, int walk, void* stream);
/* Bytes of the caller-kept workspace (16-byte aligned) of sobfu_hip_mesh_voxelise_winding: the sign bits and the list of seam voxels.
 * 0 for X outside [1, 512], Y or Z < 1, or more than INT_MAX voxels. */
size_t sobfu_hip_mesh_voxelise_winding_workspace_bytes(int X, int Y, int Z);
/* sobfu_hip_mesh_voxelise with the sign of the winding number: a voxel is inside iff w > 1 / 2 at its centre.  Distances, packing and
 * margins are sobfu_hip_mesh_voxelise's; for a closed, outward-oriented mesh (no boundary) so is every bit of the volume.
 * *d_open_rows stays the number of rows crossed an odd number of times, for information.  d_winding (X * Y * Z floats, may be NULL): w
 * at every voxel centre. */
int sobfu_hip_mesh_voxelise_winding(void* d_grid_workspace, size_t grid_workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces,
                                    int n_triangles, const float origin[3], float h, const int dims[3], const float* d_boundary, int n_boundary,
                                    float* d_vol, int X, int Y, int Z, const float voxel_size[3], float trunc, float eta, int mode, void* d_workspace,
                                    size_t workspace_bytes, int* d_open_rows, float* d_winding, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * depth sensor model  (no counterpart in the reference; sobfu_amd/csrc/depth_sensor_kernels.hip, sobfu_random.hpp)
 * A clean render -- the float4 point and normal images of sobfu_hip_mesh_render or sobfu_hip_raycast -- into the uint16 millimetre frame
 * a structured-light camera would report: lateral jitter, distance- and angle-dependent axial noise, disparity quantisation, dropouts
 * at grazing angles, at depth edges and at random, and a range gate.  The random numbers are Philox4x32-10 draws that depend on
 * (seed, frame, pixel, stream) alone: the same arguments give the same frame bit for bit on any machine and for any launch shape.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct sobfu_hip_sensor_params {
    uint64_t seed;
    uint32_t frame;
    float lateral;        /* sigma of the pixel jitter, pixels; >= 0, finite                         */
    float z_min, z_max;   /* depths kept: (z_min, z_max]; z_min finite, z_max = +Inf allowed         */
    float cos_min;        /* pixels seen flatter than this are lost; in [0, 1]                       */
    int edge_radius;      /* 0..3; 0: no edge test                                                   */
    float edge_jump;      /* metres; >= 0                                                            */
    float edge_drop;      /* probability in [0, 1] that a pixel at an edge is lost                   */
    float drop;           /* probability in [0, 1] that any pixel is lost                            */
    float a0, a1, z0, a2; /* sigma_z = (a0 + a1 (z - z0)^2) + a2 ((1 - c^2) / c^2) / sqrt(z); finite */
    float disparity;      /* focal x baseline x sub-pixel levels, pixel metres; 0: no quantisation; >= 0, finite */
} sobfu_hip_sensor_params;

/* what became of a pixel (d_flags) */
#define SOBFU_SENSOR_VALID 0   /* a depth was reported */
#define SOBFU_SENSOR_MISS 1    /* the ray missed */
#define SOBFU_SENSOR_RANGE 2   /* outside the depth range (also: no representable millimetre value, a NaN depth) */
#define SOBFU_SENSOR_GRAZING 3 /* seen at too flat an angle */
#define SOBFU_SENSOR_EDGE 4    /* lost at a depth edge */
#define SOBFU_SENSOR_DROPOUT 5 /* lost at random */

/* Known-answer entry of the generator: d_out[i] = philox4x32_10(counter d_counters[i], key), four words each (dense device arrays of
 * n x 4 uint32).  SOBFU_E_BADARG: a NULL or misaligned array, a NULL key, n < 0.  n = 0 succeeds and launches nothing.  Asynchronous. */
int sobfu_hip_philox4x32_10(const uint32_t* d_counters, const uint32_t key[2], int n, uint32_t* d_out, void* stream);
/* Pitched images (step in bytes): d_points float4 (x, y, z, .) in the camera frame, d_normals float4 with w = 1 on a hit and all zero on
 * a miss -> d_depth uint16 millimetres (0: no reading) and d_flags uint8 SOBFU_SENSOR_* (may be NULL).  Pixel (u, v) (column, row), all
 * arithmetic fp32 in this order; g0, g1, g2 are the normal variates of streams 0, 1, 2 of the pixel, U0, U1 the uniform variates of
 * words 0 and 1 of stream 3 (sobfu_random.hpp); the first condition that holds ends the pixel with depth 0 and that flag:
 *   jitter    du = clamp(rint(g0 lateral), -4, 4), dv likewise from g1; the source pixel s = (clamp(u + du, 0, cols - 1),
 *             clamp(v + dv, 0, rows - 1)) is the one everything below reads (nearest pixel: depths are never mixed)
 *   miss      N(s).w == 0
 *   range     z = P(s).z; not (z > z_min && z <= z_max) (a NaN too)
 *   grazing   l = sqrt((x x + y y) + z z), c = |(N.x x + N.y y) + N.z z| / l; c < cos_min
 *   edge      edge_radius r > 0 and some pixel q of the (2r + 1)^2 window around s inside the frame is a miss or has
 *             |z_q - z| > edge_jump; and U0 < edge_drop
 *   dropout   U1 < drop
 *   noise     dz = z - z0, cc = c c, sigma = (a0 + a1 (dz dz)) + a2 (((1 - cc) / cc) / sqrt(z)), zn = z + g2 sigma
 *   disparity when disparity > 0: q = rint(disparity / zn); not q >= 1: range; zn = disparity / q
 *   depth     mm = rint(1000 zn); not (mm >= 1 && mm <= 65535): range; else the depth is mm, valid
 * With lateral = a0 = a1 = a2 = drop = disparity = 0, edge_radius = 0, cos_min = 0, z_min = 0, z_max = +Inf the frame is
 * sobfu_hip_mesh_render's own d_depth of the same render, bit for bit.  Every argument is checked before any device call
 * (SOBFU_E_BADARG): NULL images or params, steps smaller than a row or misaligned, negative sizes, a parameter outside the range the
 * struct states.  rows * cols = 0 succeeds and launches nothing.  Asynchronous. */
int sobfu_hip_depth_sensor(const float* d_points, int points_step, const float* d_normals, int normals_step, int rows, int cols,
                           const sobfu_hip_sensor_params* p, uint16_t* d_depth, int depth_step, uint8_t* d_flags, int flags_step,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------
 * mesh sampling and F-score counts  (no counterpart in the reference; sobfu_amd/csrc/mesh_sample_kernels.hip)
 * Points drawn uniformly per unit area from an indexed triangle mesh (vertices as n_vertices dense float4, faces as n_triangles x 3
 * int32, as for the mesh distance), at `density` samples per square unit.  Triangle t of area A (fp64) receives floor(A density) samples
 * plus one more with probability frac(A density): its expectation is exactly A density and it is never more than one sample from it.
 * Sample k of triangle t is p = (a + (b - a) r1) + (c - a) r2 with (r1, r2) from the Philox4x32-10 draw of counter (t, k, 0, 1) under
 * the key (seed & 0xffffffff, seed >> 32), folded into the triangle on integers (the rule, operation by operation:
 * sobfu_amd/csrc/sobfu_mesh_sample.hpp).  Samples are ordered by triangle, then k.  The result depends on the mesh, the density and the
 * seed alone: the same bits on any machine, for any launch shape and from run to run.
 * Every argument is checked before any device call (SOBFU_E_BADARG): NULL or misaligned pointers, negative sizes, a non-finite or
 * negative density, a short workspace, n_thresholds outside 1 .. 16.
 * ---------------------------------------------------------------------------------------------------- */
/* Bytes of the caller-kept workspace (16-byte aligned) for a mesh of n_triangles: a header, the counts, their offsets and the scan's
 * block sums.  0 for n_triangles < 0. */
size_t sobfu_hip_mesh_sample_workspace_bytes(int n_triangles);
/* Counts the samples of every triangle and scans them into the workspace.  SYNCHRONISES the stream once, after the count:
 * *h_samples = the 64-bit total.  d_areas (may be NULL): n_triangles doubles, the triangles' areas.  SOBFU_E_BADARG (after the
 * synchronisation) for a face index outside [0, n_vertices) or a non-finite corner (such a triangle counts 0); SOBFU_E_UNSUPPORTED when
 * the total exceeds INT32_MAX (*h_samples still holds it; beyond 2^62 per triangle it saturates).  A workspace whose count did not
 * return 0 is not marked and sobfu_hip_mesh_sample_generate through it is refused.  n_triangles = 0 or density = 0: 0 samples, success. */
int sobfu_hip_mesh_sample_count(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, double density, uint64_t seed,
                                void* d_workspace, size_t workspace_bytes, double* d_areas, long long* h_samples, void* stream);
/* The samples of the last count through this workspace (the same mesh arrays, unchanged, and the same seed): d_points, dense float4
 * (x, y, z, 1); d_tri (may be NULL), the triangle of each sample; d_bary (may be NULL), float2 (r1, r2), the weights of the triangle's
 * second and third corner.  Reads the workspace's header back (one small copy), then only enqueues.  Never truncates: max_samples below
 * the count's total is SOBFU_E_BADARG before any launch, and so is a workspace that is not marked or was counted for another n_triangles. */
int sobfu_hip_mesh_sample_generate(const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles, uint64_t seed,
                                   void* d_workspace, size_t workspace_bytes, float* d_points, int* d_tri, float* d_bary, int max_samples,
                                   void* stream);
/* n float distances against n_thresholds (1 .. 16, host array, any order) -> d_counts, n_thresholds + 1 64-bit integers on the device
 * (8-byte aligned): d_counts[k] = #{i : d_i finite and d_i <= thresholds[k]}, d_counts[n_thresholds] = #{i : d_i finite}.  NaN and
 * +-Inf are never within.  Integer sums: the same from run to run.  n = 0 launches nothing and leaves zeros.  Asynchronous. */
int sobfu_hip_distance_score(const float* d_dist, int n, const float* h_thresholds, int n_thresholds, long long* d_counts, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * warp-field diagnostics  (no counterpart in the reference; sobfu_amd/csrc/warp_stats_kernels.hip)
 * One pass over psi (float4 per voxel: the absolute position in voxel units; dense, x fastest, 16-byte aligned), optionally psi^-1 (the
 * same format) and up to two masks in the {tsdf, weight} float2 format: a voxel is in a mask iff the pointer is NULL or
 * weight > 0 && fabsf(tsdf) < band.  The rules, operation by operation: sobfu_amd/csrc/sobfu_warp_stats.hpp.
 *   u           psi - id.  Its derivative along an axis of extent n at index i: 0 when n == 1; u(1) - u(0) at i == 0 and
 *               u(n - 1) - u(n - 2) at i == n - 1 (one-sided, not halved); (u(i + 1) - u(i - 1)) / 2 elsewhere
 *   det         of J_rc = (r == c) + d_c u_r, the expression of sobfu_hip_warp_points; unit-free; identity: exactly 1 at every voxel
 *   det group   (voxels in d_mask_det) a non-finite det counts in N_DET_NONFINITE only; else N_DET, N_FOLD (det <= 0),
 *               DET_BELOW + k (det < edges[k]), the exact sum, the minimum and the maximum
 *   disp group  (the same mask) |u| in metres, sqrtf(((u.x vs.x)^2 + (u.y vs.y)^2) + (u.z vs.z)^2): non-finite counts in
 *               N_DISP_NONFINITE; else N_DISP, the exact sum and the maximum
 *   res group   (only with d_psi_inv; voxels x in d_mask_res) p = psi^-1[x]: a non-finite component counts in N_RES_NONFINITE; else p
 *               outside [0, dim - 1] on any axis in N_RES_OUTSIDE; else e = (p + u(p)) - x with u(p) by the trilinear sampler of
 *               sobfu_hip_estimate_inverse, and |e| in metres: non-finite counts in N_RES_NONFINITE; else N_RES, N_RES_ABOVE
 *               (|e| > res_tol), the exact sum and the maximum.  Swapping the two fields measures psi^-1 o psi
 *   exact sums  of q = llrint(clamp((double) v, -1024, 1024) 2^44) in two signed words: HI = sum(q >> 24), LO = sum(q & 0xffffff);
 *               the sum is (HI 2^24 + LO) 2^-44.  Independent of the order
 *   keys        a minimum is the least (ord(v) << 32) | linear index over the group, ord the order-preserving map of the float's bits
 *               (b ^ 0x80000000 for b >= 0, ~b for b < 0, after v + 0.f); a maximum the least (~ord(v) << 32) | index: ties go to the
 *               lowest linear index.  An empty group leaves ~0, which decodes to NaN and index -1
 * d_result: SOBFU_WS_WORDS 64-bit words on the device (8-byte aligned), prepared by the call (a buffer may be reused uncleared); the
 * words beyond RES_MAX_KEY are 0.  d_det (may be NULL): det of every voxel, masked or not.  d_res (may be NULL; needs d_psi_inv): |e| of
 * every voxel, NaN where p is outside or non-finite.  In both a NaN is the quiet NaN 0x7fc00000.
 * The result is the same bits from run to run and for any launch shape.  Every argument is checked before any device call
 * (SOBFU_E_BADARG): NULL or misaligned pointers, d_res or d_mask_res without d_psi_inv, an extent < 1 or more than 2^31 voxels, a voxel
 * size or band that is not positive and finite, res_tol negative or NaN, n_edges outside 0 .. 16 or edges NULL with n_edges > 0, edges
 * (a host array) not finite and strictly ascending.  Asynchronous.
 * ---------------------------------------------------------------------------------------------------- */
enum {
    SOBFU_WS_N_DET = 0,
    SOBFU_WS_N_FOLD = 1,
    SOBFU_WS_N_DET_NONFINITE = 2,
    SOBFU_WS_N_DISP = 3,
    SOBFU_WS_N_DISP_NONFINITE = 4,
    SOBFU_WS_N_RES = 5,
    SOBFU_WS_N_RES_ABOVE = 6,
    SOBFU_WS_N_RES_OUTSIDE = 7,
    SOBFU_WS_N_RES_NONFINITE = 8,
    SOBFU_WS_DET_BELOW = 9, /* 16 words */
    SOBFU_WS_DET_SUM_HI = 25,
    SOBFU_WS_DET_SUM_LO = 26,
    SOBFU_WS_DISP_SUM_HI = 27,
    SOBFU_WS_DISP_SUM_LO = 28,
    SOBFU_WS_RES_SUM_HI = 29,
    SOBFU_WS_RES_SUM_LO = 30,
    SOBFU_WS_DET_MIN_KEY = 31,
    SOBFU_WS_DET_MAX_KEY = 32,
    SOBFU_WS_DISP_MAX_KEY = 33,
    SOBFU_WS_RES_MAX_KEY = 34,
    SOBFU_WS_WORDS = 64
};
int sobfu_hip_warp_stats(const float* d_psi, const float* d_psi_inv, const float* d_mask_det, const float* d_mask_res, int X, int Y, int Z,
                         const float voxel_size[3], float band, const float* edges, int n_edges, float res_tol, unsigned long long* d_result,
                         float* d_det, float* d_res, void* stream);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif /* SOBFU_HIP_H */
