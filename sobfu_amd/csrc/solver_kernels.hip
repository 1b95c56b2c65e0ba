// Solver kernels for gfx950.
//
// (The launcher-for-launcher counterparts of include/sobfu/solver.hpp:109-136 -- potential gradient, the three 1-D Sobolev
//  convolutions, psi update -- live in launcher_kernels.hip.)
// The MI355X-native two-pass decomposition of one solver iteration (solver.cu:114-193):
//             pass A  fused_potential_gradient : grad(phi_n o psi) + (-Lap psi) + combine      -> nabla_U
//             pass B  fused_smooth_update_apply: (Sx+Sy+Sz) nabla_U, psi -= alpha*.., phi_n o psi, max||u||^2
//           Both march along z with a register pipeline for the z taps and stage each xy plane (plus a
//           radius-1 / radius-3 halo) in a double-buffered LDS tile for the x/y taps: every plane is read from
//           HBM once per tile (+ halo), 112 B/voxel/iteration algorithmic traffic instead of the reference's
//           456 B/voxel.
//
// Arithmetic is op-for-op the reference's (see sobfu_device.hpp): results are bit-identical to the launcher-for-launcher kernels.
#include <type_traits>

#include "sobfu_device.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_launch.hpp"

using namespace sobfu_hip;

#ifndef SOBFU_SWIZZLE_B
#define SOBFU_SWIZZLE_B true  // XCD-aware tile map for pass B (see tile_of_block)
#endif

namespace {

struct Taps {
    float s[7];
};
constexpr int kMaxMsgs = 18;  // 6 face + 12 edge neighbours of a 3-D tile

// the fused two-pass iteration: device code in four included parts, one translation unit
#include "solver_iter_common.inl"
#include "solver_pass_a.inl"
#include "solver_pass_b.inl"
#include "solver_aux_kernels.inl"

}  // namespace

namespace sobfu_hip {

// Calls launch(std::integral_constant<size_t, I>{}) for the row I of `table` that equals `v`, which instantiates the kernel of that
// row: only the table's rows are ever instantiated.  false: `v` is no row of the table.
template <size_t I = 0, class Row, size_t N, class F>
static bool launch_row(const Row (&table)[N], const Row& v, F&& launch) {
    if constexpr (I < N) {
        if (table[I] == v) {
            launch(std::integral_constant<size_t, I>{});
            return true;
        }
        return launch_row<I + 1>(table, v, launch);
    } else {
        return false;
    }
}

// the launch of a box list in device memory by the tile kernel (v: choose_pass_a with tile = true)
static int launch_tile_boxes(const TilePassAArgsP& a, int groups, const PassAVariant& v, hipStream_t stream) {
    const dim3 grid((unsigned) groups), block(TX, kWY);
    const bool found = launch_row(kTilePassATable, v, [&](auto i) {
        constexpr PassAVariant V = kTilePassATable[decltype(i)::value];
        hipLaunchKernelGGL((tile_potential_gradient_kernel<kRPT, kWY, V.compact, V.nt ? kNT : 0>), grid, block, 0, stream, a);
    });
    return found ? (int) hipGetLastError() : SOBFU_E_UNSUPPORTED;
}

int launch_pass_a(const PassALaunch& L, hipStream_t stream) {
    if (L.n_boxes > kMaxBoxes) return SOBFU_E_BADARG;
    const bool direct = has_direct_box(L.boxes, L.n_boxes);
    const GridTraits g = grid_traits(L.X, L.Y, L.Z, L.X, L.Y, L.Z, env_cache_cells());
    PassAVariant v;
    SOBFU_TRY(choose_pass_a(g, L.compact, L.warp, direct, &v));
    if (direct) {  // thin boxes: the tile kernel (no messages, no signalling, no gate) with a list of this call's own
        TileBoxList B{};
        const int total = plan_pass_a_thin(B, L.boxes, L.n_boxes, g.resident);
        if (total <= 0) return total < 0 ? SOBFU_E_BADARG : 0;
        // a stream-ordered device copy, freed behind the launch (hipMemcpyAsync from pageable memory has read B when it returns)
        TileBoxList* d = nullptr;
        SOBFU_HIP_TRY(hipMallocAsync((void**) &d, sizeof B, stream));
        const hipError_t e = hipMemcpyAsync(d, &B, sizeof B, hipMemcpyHostToDevice, stream);
        const TilePassAArgsP a{{L.pnp, L.pg, L.psi, L.nU, {L.X, L.Y, L.Z}, L.w_reg, nullptr, 0.f}, d, {nullptr, 0, 0, nullptr, 0}};
        const int rc = e != hipSuccess ? (int) e : launch_tile_boxes(a, total, v, stream);
        const hipError_t f = hipFreeAsync(d, stream);
        return rc != 0 ? rc : (int) f;
    }
    PassAArgs a{{L.pnp, L.pg, L.psi, L.nU, {L.X, L.Y, L.Z}, L.w_reg, L.prev_slots, L.max_update_norm}, {}};
    const int groups = v.warp ? plan_pass_a_warp(a.boxes, L.boxes, L.n_boxes) : plan_pass_a(a.boxes, L.boxes, L.n_boxes);
    if (groups == 0) return 0;
    const dim3 grid((unsigned) groups);
    const bool found = launch_row(kPassATable, v, [&](auto i) {
        constexpr PassAVariant V = kPassATable[decltype(i)::value];
        constexpr int WY = V.warp ? kWarpWY : kWY;  // the warping march has a tile height of its own
        hipLaunchKernelGGL((fused_potential_gradient_kernel<kRPT, WY, V.compact, V.nt ? kNT : 0, V.warp>), grid, dim3(TX, WY), 0, stream, a);
    });
    return found ? (int) hipGetLastError() : SOBFU_E_UNSUPPORTED;
}

// A PLANNED launch of the same pass (compact format): the geometry is worked out once per handle and half of the nabla_U ping-pong
struct TilePassAPlan {
    TileBoxList* d_boxes = nullptr;
    int groups = 0, X = 0, Y = 0, Z = 0;
};
int tile_pass_a_plan_create(TilePassAPlan** out, const TileLaunchBox* boxes, int n, int X, int Y, int Z) {
    TileBoxList L{};
    const int total = fill_tile_boxes(L, boxes, n, grid_traits(X, Y, Z, X, Y, Z, env_cache_cells()).resident);
    if (total < 0) return SOBFU_E_BADARG;
    auto* p = new TilePassAPlan();
    p->groups = total; p->X = X; p->Y = Y; p->Z = Z;
    // a plan owns its device copy and lives as long as its handle: plan time is handle creation, not a launch path, so a blocking
    // copy is fine -- the list is simply there before any stream launches with it
    hipError_t e = hipSuccess;
    if (total > 0) {
        e = hipMalloc((void**) &p->d_boxes, sizeof L);
        if (e == hipSuccess) e = hipMemcpy(p->d_boxes, &L, sizeof L, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (p->d_boxes) (void) hipFree(p->d_boxes);
        delete p;
        return (int) e;
    }
    *out = p;
    return 0;
}
void tile_pass_a_plan_destroy(TilePassAPlan* p) {
    if (p == nullptr) return;
    if (p->d_boxes) (void) hipFree(p->d_boxes);  // (hipFree waits for the device: no launch is still reading the list)
    delete p;
}
int launch_tile_pass_a_plan(const TilePassAPlan* p, const float* pnp, const float* pg, const float* psi, float* nU, float w_reg, TileSync* sync,
                            uint32_t seq, int wait, const uint32_t* row, uint32_t row_index, hipStream_t stream) {
    if (p->groups == 0) return 0;
    PassAVariant v;
    SOBFU_TRY(choose_pass_a(grid_traits(p->X, p->Y, p->Z, p->X, p->Y, p->Z, env_cache_cells()), true, false, true, &v));
    const TilePassAArgsP a{{pnp, pg, psi, nU, {p->X, p->Y, p->Z}, w_reg, nullptr, 0.f}, p->d_boxes, {sync, seq, wait, row, row_index}};
    return launch_tile_boxes(a, p->groups, v, stream);
}

int launch_tile_pingpong(TileSync* sync, int q, int first, uint32_t seq0, int reps, hipStream_t stream) {
    hipLaunchKernelGGL(tile_pingpong_kernel, dim3(1), dim3(64), 0, stream, sync, q, first, seq0, reps);
    return (int) hipGetLastError();
}

int launch_tile_flush(TileSync* sync, uint32_t seq, int wait, const uint32_t* row, uint32_t row_index, hipStream_t stream) {
    hipLaunchKernelGGL(tile_flush_kernel, dim3(1), dim3(64), 0, stream, sync, seq, wait, row, row_index);
    return (int) hipGetLastError();
}

int launch_pass_b(const PassBLaunch& L, hipStream_t stream) {
    if (L.n_boxes > kMaxBoxes) return SOBFU_E_BADARG;
    PassBArgs a{L.nU, L.psi, L.phi_n, L.pnp, (float4*) L.updates, L.slots, {L.X, L.Y, L.Z}, {}, L.alpha, {}, L.prev_slots, L.max_update_norm,
                {L.pX, L.pY, L.pZ}, {L.own[0], L.own[1], L.own[2], L.own[3], L.own[4], L.own[5]}, L.prev_rows, L.psi_out ? L.psi_out : L.psi,
                L.sys_acquire ? 1 : 0};
    for (int i = 0; i < 7; ++i) a.S.s[i] = L.taps[i];
    const GridTraits g = grid_traits(L.X, L.Y, L.Z, L.pX, L.pY, L.pZ, env_cache_cells(), env_pipe_b());
    const PassBAsk ask{L.compact, L.updates != nullptr, L.sys_acquire, !L.warp};
    PassBMarch m;
    SOBFU_TRY(pass_b_march(g, ask, &m));
    const int groups = plan_pass_b(a.boxes, L.boxes, L.n_boxes, g, m);
    if (groups == 0) return 0;  // an empty launch is no launch, whatever stage 2 would say of it
    PassBVariant v;
    SOBFU_TRY(choose_pass_b(g, ask, m, &v));
    const dim3 grid((unsigned) groups), block(TX, kWY);
    const bool found = launch_row(kPassBTable, v, [&](auto i) {
        constexpr PassBVariant V = kPassBTable[decltype(i)::value];
        hipLaunchKernelGGL((fused_smooth_update_apply_kernel<kRPT, kWY, V.updates, V.compact, V.direct, V.idx32, V.lead ? SOBFU_HLEAD : 0,
                                                             V.nt ? kNT : 0, V.pipe, V.ntbuf, V.apply>),
                           grid, block, 0, stream, a);
    });
    return found ? (int) hipGetLastError() : SOBFU_E_UNSUPPORTED;
}

#define SOBFU_LIN(N) dim3((unsigned) (((N) + 255) / 256)), dim3(256), 0, stream
int launch_pack_vec(const float* src4, float* dst3, size_t N, hipStream_t stream) {
    hipLaunchKernelGGL(pack_vec_kernel, SOBFU_LIN(N), (const float4*) src4, (P3*) dst3, N);
    return (int) hipGetLastError();
}
int launch_unpack_vec(const float* src3, float* dst4, size_t N, hipStream_t stream) {
    hipLaunchKernelGGL(unpack_vec_kernel, SOBFU_LIN(N), (const P3*) src3, (float4*) dst4, N);
    return (int) hipGetLastError();
}
int launch_extract_tsdf(const float* src2, float* dst1, size_t N, hipStream_t stream) {
    hipLaunchKernelGGL(extract_tsdf_kernel, SOBFU_LIN(N), (const float2*) src2, dst1, N);
    return (int) hipGetLastError();
}
int launch_apply_tsdf_only(const float* phi1, float* out1, const float* psi3, int X, int Y, int Z, hipStream_t stream, int phi_Z, int phi_X,
                           int phi_Y) {
    hipLaunchKernelGGL(apply_tsdf_only_kernel, voxel_grid(X, Y, Z), voxel_block(), 0, stream, phi1, out1, (const P3*) psi3, Dims{X, Y, Z},
                       Dims{phi_X > 0 ? phi_X : X, phi_Y > 0 ? phi_Y : Y, phi_Z > 0 ? phi_Z : Z});
    return (int) hipGetLastError();
}
// n boxes of 6 ints (x0, x1, y0, y1, z0, z1) of a 12-byte (Lx, Ly, Lz) field <-> consecutive buffer segments (x fastest)
int launch_msg_copy(bool pack, float* field3, float* buf, int Lx, int Ly, int Lz, const int* boxes, int n, hipStream_t stream) {
    if (n <= 0) return 0;
    if (n > kMaxMsgs) return SOBFU_E_BADARG;
    MsgBoxes m{};
    m.n = n;
    unsigned total = 0;
    for (int i = 0; i < n; ++i) {
        const int* b = boxes + 6 * i;
        if (!(b[0] >= 0 && b[1] > b[0] && b[1] <= Lx && b[2] >= 0 && b[3] > b[2] && b[3] <= Ly && b[4] >= 0 && b[5] > b[4] && b[5] <= Lz)) return SOBFU_E_BADARG;
        m.x0[i] = b[0]; m.y0[i] = b[2]; m.z0[i] = b[4];
        m.nx[i] = b[1] - b[0]; m.ny[i] = b[3] - b[2];
        m.first[i] = total;
        total += (unsigned) (b[1] - b[0]) * (unsigned) (b[3] - b[2]) * (unsigned) (b[5] - b[4]);
    }
    for (int k = n; k <= kMaxMsgs; ++k) m.first[k] = total;
    const dim3 grid((total + 255u) / 256u), block(256);
    if (pack) hipLaunchKernelGGL(msg_copy_kernel<true>, grid, block, 0, stream, field3, buf, Dims{Lx, Ly, Lz}, m);
    else hipLaunchKernelGGL(msg_copy_kernel<false>, grid, block, 0, stream, field3, buf, Dims{Lx, Ly, Lz}, m);
    return (int) hipGetLastError();
}
int launch_msg_scatter_table(float* field3, const float* buf, const uint32_t* d_table, unsigned n_cells, hipStream_t stream) {
    if (n_cells == 0) return 0;
    hipLaunchKernelGGL(msg_scatter_table_kernel, dim3((n_cells + 255u) / 256u), dim3(256), 0, stream, field3, buf, d_table, n_cells);
    return (int) hipGetLastError();
}
#undef SOBFU_LIN
int launch_compact_enter(const float* psi4, const float* pg2, const float* pn2, float* c_psi, float* c_g, float* c_n, float* c_f, int X, int Y,
                         int Z, hipStream_t stream) {
    hipLaunchKernelGGL(compact_enter_kernel, voxel_grid(X, Y, Z), voxel_block(), 0, stream, (const float4*) psi4, (const float2*) pg2,
                       (const float2*) pn2, (P3*) c_psi, c_g, c_n, c_f, Dims{X, Y, Z});
    return (int) hipGetLastError();
}
int launch_compact_leave(const float* c_psi, const float* pn2, float* psi4, float* pnp2, int X, int Y, int Z, hipStream_t stream) {
    hipLaunchKernelGGL(compact_leave_kernel, voxel_grid(X, Y, Z), voxel_block(), 0, stream, (const P3*) c_psi, (const float2*) pn2,
                       (float4*) psi4, (float2*) pnp2, Dims{X, Y, Z});
    return (int) hipGetLastError();
}

}  // namespace sobfu_hip

extern "C" {

int sobfu_hip_fused_potential_gradient(const float* d_phi_n_psi, const float* d_phi_global, const float* d_psi,
                                       float* d_nabla_U, float w_reg, int X, int Y, int Z, void* stream) {
    SOBFU_CHECK_ARGS(d_phi_n_psi && d_phi_global && d_psi && d_nabla_U && X > 1 && Y > 1 && Z > 1);
    if ((size_t) X * Y * Z > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    sobfu_hip::PassALaunch L;
    sobfu_hip::set_whole_grid(L, X, Y, Z);
    L.pnp = d_phi_n_psi; L.pg = d_phi_global; L.psi = d_psi; L.nU = d_nabla_U; L.w_reg = w_reg;
    return sobfu_hip::launch_pass_a(L, (hipStream_t) stream);
}

int sobfu_hip_fused_smooth_update_apply(const float* d_nabla_U, float* d_psi, const float* d_phi_n, float* d_phi_n_psi,
                                        float* d_updates, uint32_t* d_max_sq_slots, const float taps[7], float alpha,
                                        int X, int Y, int Z, void* stream) {
    SOBFU_CHECK_ARGS(d_nabla_U && d_psi && d_phi_n && d_phi_n_psi && d_max_sq_slots && taps && X > 0 && Y > 0 && Z > 0);
    if ((size_t) X * Y * Z > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    sobfu_hip::PassBLaunch L;
    sobfu_hip::set_whole_grid(L, X, Y, Z);
    L.nU = d_nabla_U; L.psi = d_psi; L.phi_n = d_phi_n; L.pnp = d_phi_n_psi; L.updates = d_updates; L.slots = d_max_sq_slots;
    L.taps = taps; L.alpha = alpha;
    return sobfu_hip::launch_pass_b(L, (hipStream_t) stream);
}

int sobfu_hip_pack_vec3(const float* d_src4, float* d_dst3, size_t n, void* stream) {
    SOBFU_CHECK_ARGS(d_src4 && d_dst3 && n > 0);
    return sobfu_hip::launch_pack_vec(d_src4, d_dst3, n, (hipStream_t) stream);
}
int sobfu_hip_unpack_vec3(const float* d_src3, float* d_dst4, size_t n, void* stream) {
    SOBFU_CHECK_ARGS(d_src3 && d_dst4 && n > 0);
    return sobfu_hip::launch_unpack_vec(d_src3, d_dst4, n, (hipStream_t) stream);
}
int sobfu_hip_extract_tsdf(const float* d_src2, float* d_dst1, size_t n, void* stream) {
    SOBFU_CHECK_ARGS(d_src2 && d_dst1 && n > 0);
    return sobfu_hip::launch_extract_tsdf(d_src2, d_dst1, n, (hipStream_t) stream);
}
// ---- 3-D tiles (sobfu_hip_tile3_*): local arrays (Lx, Ly, Lz) with halo cells on every side that faces a neighbour ----
static bool box_ok(const int b[6], int Lx, int Ly, int Lz) {
    return b[0] >= 0 && b[0] <= b[1] && b[1] <= Lx && b[2] >= 0 && b[2] <= b[3] && b[3] <= Ly && b[4] >= 0 && b[4] <= b[5] && b[5] <= Lz;
}

int sobfu_hip_tile3_potential_gradient(const float* d_phi_n_psi, const float* d_phi_global, const float* d_psi, float* d_nabla_U, float w_reg,
                                       int Lx, int Ly, int Lz, const int box[6], int thin, const uint32_t* d_prev_slots,
                                       float max_update_norm, int compact, void* stream) {
    SOBFU_CHECK_ARGS(d_phi_n_psi && d_phi_global && d_psi && d_nabla_U && Lx > 1 && Ly > 1 && Lz > 1 && box && box_ok(box, Lx, Ly, Lz));
    if ((size_t) Lx * Ly * Lz > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    sobfu_hip::PassALaunch L;
    L.pnp = d_phi_n_psi; L.pg = d_phi_global; L.psi = d_psi; L.nU = d_nabla_U; L.w_reg = w_reg;
    L.X = Lx; L.Y = Ly; L.Z = Lz;
    L.boxes[0] = sobfu_hip::LaunchBox{box[0], box[1], box[2], box[3], box[4], box[5], thin != 0};
    L.n_boxes = 1;
    L.prev_slots = d_prev_slots; L.max_update_norm = max_update_norm;
    L.compact = compact != 0;
    return sobfu_hip::launch_pass_a(L, (hipStream_t) stream);
}

int sobfu_hip_tile3_smooth_update_apply(const float* d_nabla_U, float* d_psi, const float* d_phi_n, float* d_phi_n_psi, float* d_updates,
                                        uint32_t* d_max_sq_slots, const float taps[7], float alpha, int Lx, int Ly, int Lz, int Xg, int Yg,
                                        int Zg, const int own[6], const int box[6], int thin, const uint32_t* d_prev_slots,
                                        float max_update_norm, int compact, void* stream) {
    SOBFU_CHECK_ARGS(d_nabla_U && d_psi && d_phi_n && d_phi_n_psi && d_max_sq_slots && taps && Lx > 0 && Ly > 0 && Lz > 0 && Xg > 0 && Yg > 0 &&
                     Zg > 0 && own && box && box_ok(own, Lx, Ly, Lz) && box_ok(box, Lx, Ly, Lz));
    if ((size_t) Lx * Ly * Lz > (size_t) 0x7fffffff || (size_t) Xg * Yg * Zg > (size_t) 0x7fffffff) return SOBFU_E_UNSUPPORTED;
    sobfu_hip::PassBLaunch L;
    L.nU = d_nabla_U; L.psi = d_psi; L.phi_n = d_phi_n; L.pnp = d_phi_n_psi; L.updates = d_updates; L.slots = d_max_sq_slots;
    L.taps = taps; L.alpha = alpha;
    L.X = Lx; L.Y = Ly; L.Z = Lz;
    L.pX = Xg; L.pY = Yg; L.pZ = Zg;
    for (int i = 0; i < 6; ++i) L.own[i] = own[i];
    L.boxes[0] = sobfu_hip::LaunchBox{box[0], box[1], box[2], box[3], box[4], box[5], thin != 0};
    L.n_boxes = 1;
    L.prev_slots = d_prev_slots; L.max_update_norm = max_update_norm;
    L.compact = compact != 0;
    return sobfu_hip::launch_pass_b(L, (hipStream_t) stream);
}

int sobfu_hip_tile3_apply_tsdf_only(const float* d_phi1, int Xg, int Yg, int Zg, float* d_out1, const float* d_psi3, int Lx, int Ly, int Lz,
                                    void* stream) {
    SOBFU_CHECK_ARGS(d_phi1 && d_out1 && d_psi3 && Lx > 0 && Ly > 0 && Lz > 0 && Xg > 0 && Yg > 0 && Zg > 0);
    return sobfu_hip::launch_apply_tsdf_only(d_phi1, d_out1, d_psi3, Lx, Ly, Lz, (hipStream_t) stream, Zg, Xg, Yg);
}

int sobfu_hip_tile3_pack(const float* d_field3, int Lx, int Ly, int Lz, float* d_buf, const int* boxes, int n_boxes, void* stream) {
    SOBFU_CHECK_ARGS(d_field3 && d_buf && boxes && n_boxes >= 0 && Lx > 0 && Ly > 0 && Lz > 0);
    return sobfu_hip::launch_msg_copy(true, const_cast<float*>(d_field3), d_buf, Lx, Ly, Lz, boxes, n_boxes, (hipStream_t) stream);
}

int sobfu_hip_tile3_unpack(float* d_field3, int Lx, int Ly, int Lz, const float* d_buf, const int* boxes, int n_boxes, void* stream) {
    SOBFU_CHECK_ARGS(d_field3 && d_buf && boxes && n_boxes >= 0 && Lx > 0 && Ly > 0 && Lz > 0);
    return sobfu_hip::launch_msg_copy(false, d_field3, const_cast<float*>(d_buf), Lx, Ly, Lz, boxes, n_boxes, (hipStream_t) stream);
}

}  // extern "C"
