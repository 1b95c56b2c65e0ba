// Diagnostics of the deformation for gfx950: one pass over psi -- and optionally psi^-1 and up to two TSDF masks -- into a
// block of 64 integer words (include/sobfu_hip.h, SOBFU_WS_*) and, on request, the per-voxel det J and inverse residual.  The reference has
// no such step; the rules are this project's (sobfu_warp_stats.hpp, restated by tests/warp_stats_reference.py): every output is an integer
// sum, an integer minimum or a per-voxel value, so the result does not depend on the launch shape, the schedule or the run.
//
// Launch shape (ws_launch): a workgroup is a 64 x 4 tile of (x, y) columns marching a chunk of z planes, about 1024 workgroups (what the chip holds at once)
// (chunks never shorter than 4 planes), numbered so that an XCD owns a band of tile rows (ws_tile: xcd_tile's rule on a 1-D grid).  A lane
// keeps the displacement of its column at z - 1, z and z + 1 in registers: psi is requested once per voxel along z, the +-x and +-y taps are
// the neighbouring lanes' and rows' lines and come from cache.  The pass moves 16 B / voxel (24 with one mask; 48 with psi^-1 and both
// masks, plus the sampler's gathers around psi^-1(x), which lie within max |u| of x).  The streams read or written exactly once -- the
// masks, psi^-1, the two volumes -- are nontemporal where launcher_streams says so; psi is not: its lines are the stencil's taps.
//
// Reduction: the result block is two cache lines, so a lane accumulates its column in registers (35 words: 25 counts, three two-word exact
// sums, four keys), the 64 lanes of a wave fold them by shuffles, the four waves through LDS, and 35 lanes of the workgroup issue one
// integer atomic each -- and only for words that are not the neutral element.  ~1024 x 35 atomics at any size; no floating-point atomics,
// no waiting between workgroups, no flags.
#include "sobfu_device.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_warp_stats.hpp"

using namespace sobfu_hip;

namespace {

// the accumulators of a lane, in the order of the result block's words
constexpr int kAccBelow = SOBFU_WS_DET_BELOW, kAccSums = SOBFU_WS_DET_SUM_HI, kAccKeys = SOBFU_WS_DET_MIN_KEY, kAcc = SOBFU_WS_RES_MAX_KEY + 1;
static_assert(kAccBelow == 9 && kAccSums == kAccBelow + kWsMaxEdges && kAccKeys == kAccSums + 6 && kAcc == 35, "the accumulators follow the result block");

struct WsArgs {
    const float4* psi;
    const float4* psi_inv;   // may be null
    const float2* mask_det;  // may be null
    const float2* mask_res;  // may be null
    WsDims d;
    float vs[3];
    float band;
    float edges[kWsMaxEdges];  // the unused ones -Inf: no det is below
    float res_tol;
    unsigned long long* result;
    float* det;  // may be null
    float* res;  // may be null
    WsLaunch l;
};

// component by component: a select between two struct objects goes through the stack
SOBFU_DEV WsV3 sel3(bool c, const WsV3& a, const WsV3& b) { return WsV3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }

template <bool NT>
SOBFU_DEV void st1(float* p, float v) {
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <bool INV, bool MASK, bool VOL, bool NT>
__global__ void __launch_bounds__(256) warp_stats_kernel(WsArgs a) {
    unsigned bx, by, bz;
    ws_tile(blockIdx.x, a.l, bx, by, bz);
    const WsDims d = a.d;
    const long long xq = (long long) bx * kWsTileX + threadIdx.x, yq = (long long) by * kWsTileY + threadIdx.y;
    const int z0 = (int) ((long long) bz * a.l.zc);
    const int z1 = (long long) z0 + a.l.zc < d.z ? z0 + a.l.zc : d.z;

    unsigned cnt[kAccSums];
#pragma unroll
    for (int k = 0; k < kAccSums; ++k) cnt[k] = 0u;
    WsSum det_sum{0, 0}, disp_sum{0, 0}, res_sum{0, 0};
    uint64_t det_min = kWsEmptyKey, det_max = kWsEmptyKey, disp_max = kWsEmptyKey, res_max = kWsEmptyKey;

    if (xq < d.x && yq < d.y && z0 < z1) {
        const int x = (int) xq, y = (int) yq;
        const size_t sy = (size_t) d.x, sz = (size_t) d.x * (size_t) d.y;
        const float4* psi = a.psi;
        auto disp = [&](int i, int j, int k) {
            const float4 p = psi[(size_t) i + sy * (size_t) j + sz * (size_t) k];
            return ws_disp(p.x, p.y, p.z, i, j, k);
        };
        int xl, xh, yl, yh;
        bool xhalf, yhalf;
        ws_axis(d.x, x, xl, xh, xhalf);
        ws_axis(d.y, y, yl, yh, yhalf);
        WsV3 uc = disp(x, y, z0);
        WsV3 um = uc;
        if (z0 > 0) um = disp(x, y, z0 - 1);
        for (int z = z0; z < z1; ++z) {
            const bool top = z == d.z - 1;
            WsV3 up = uc, ux0 = uc, ux1 = uc, uy0 = uc, uy1 = uc;  // a tap the volume does not have is the centre
            if (!top) up = disp(x, y, z + 1);
            if (xl != x) ux0 = disp(xl, y, z);
            if (xh != x) ux1 = disp(xh, y, z);
            if (yl != y) uy0 = disp(x, yl, z);
            if (yh != y) uy1 = disp(x, yh, z);
            const WsV3 dx = ws_deriv(ux0, ux1, xhalf, d.x == 1), dy = ws_deriv(uy0, uy1, yhalf, d.y == 1);
            const WsV3 dz = ws_deriv(sel3(z > 0, um, uc), up, z > 0 && !top, d.z == 1);
            const float det = ws_det(dx, dy, dz);
            const size_t i = (size_t) x + sy * (size_t) y + sz * (size_t) z;
            const uint32_t index = (uint32_t) i;
            if (VOL && a.det) st1<NT>(a.det + i, ws_canonical(det));

            bool in_det = true;
            if (MASK && a.mask_det) {
                const float2 m = ld2<NT>(a.mask_det + i);
                in_det = ws_in_mask(m.x, m.y, a.band);
            }
            if (in_det) {
                if (ws_finite(det)) {
                    ++cnt[SOBFU_WS_N_DET];
                    cnt[SOBFU_WS_N_FOLD] += det <= 0.f ? 1u : 0u;
#pragma unroll
                    for (int k = 0; k < kWsMaxEdges; ++k) cnt[kAccBelow + k] += det < a.edges[k] ? 1u : 0u;
                    ws_add(det_sum, det);
                    const uint64_t lo = ws_min_key(det, index), hi = ws_max_key(det, index);
                    det_min = lo < det_min ? lo : det_min;
                    det_max = hi < det_max ? hi : det_max;
                } else {
                    ++cnt[SOBFU_WS_N_DET_NONFINITE];
                }
                const float len = ws_len(uc, a.vs);
                if (ws_finite(len)) {
                    ++cnt[SOBFU_WS_N_DISP];
                    ws_add(disp_sum, len);
                    const uint64_t hi = ws_max_key(len, index);
                    disp_max = hi < disp_max ? hi : disp_max;
                } else {
                    ++cnt[SOBFU_WS_N_DISP_NONFINITE];
                }
            }
            if (INV) {
                bool in_res = true;
                if (MASK && a.mask_res) {
                    const float2 m = ld2<NT>(a.mask_res + i);
                    in_res = ws_in_mask(m.x, m.y, a.band);
                }
                if (in_res || (VOL && a.res)) {
                    const float4 p = ld4<NT>(a.psi_inv + i);
                    float len;
                    const int cls = ws_residual(disp, d, p.x, p.y, p.z, x, y, z, a.vs, &len);
                    if (VOL && a.res) st1<NT>(a.res + i, len);
                    if (in_res) {
                        if (cls == kWsResOk) {
                            ++cnt[SOBFU_WS_N_RES];
                            cnt[SOBFU_WS_N_RES_ABOVE] += len > a.res_tol ? 1u : 0u;
                            ws_add(res_sum, len);
                            const uint64_t hi = ws_max_key(len, index);
                            res_max = hi < res_max ? hi : res_max;
                        } else {
                            cnt[SOBFU_WS_N_RES_OUTSIDE] += cls == kWsResOutside ? 1u : 0u;  // constant indices: the counts stay in registers
                            cnt[SOBFU_WS_N_RES_NONFINITE] += cls == kWsResOutside ? 0u : 1u;
                        }
                    }
                }
            }
            um = uc, uc = up;
        }
    }

    // every lane of the workgroup arrives here.  Words below kAccKeys are sums (the signed ones in two's complement), the rest minima
    __shared__ unsigned long long s_part[4][kAcc];
    const int tid = threadIdx.y * kWsTileX + threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the counts in 32 bits -- a lane's is at most the planes of its chunk (< 2^21: ws_launch), a wave's 64 times that -- so a level of
    // their fold is one shuffle, not two
#pragma unroll
    for (int k = 0; k < kAccSums; ++k) {
        unsigned v = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) s_part[wave][k] = v;
    }
    unsigned long long acc[kAcc - kAccSums];
    acc[0] = (unsigned long long) det_sum.hi, acc[1] = (unsigned long long) det_sum.lo;
    acc[2] = (unsigned long long) disp_sum.hi, acc[3] = (unsigned long long) disp_sum.lo;
    acc[4] = (unsigned long long) res_sum.hi, acc[5] = (unsigned long long) res_sum.lo;
    acc[6] = det_min, acc[7] = det_max, acc[8] = disp_max, acc[9] = res_max;
#pragma unroll
    for (int k = kAccSums; k < kAcc; ++k) {
        unsigned long long v = acc[k - kAccSums];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long w = __shfl_down(v, o, 64);
            v = k < kAccKeys ? v + w : (w < v ? w : v);
        }
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (tid < kAcc) {
        const unsigned long long p0 = s_part[0][tid], p1 = s_part[1][tid], p2 = s_part[2][tid], p3 = s_part[3][tid];
        if (tid < kAccKeys) {
            const unsigned long long sum = (p0 + p1) + (p2 + p3);
            if (sum) atomicAdd(a.result + tid, sum);
        } else {
            const unsigned long long m01 = p0 < p1 ? p0 : p1, m23 = p2 < p3 ? p2 : p3, m = m01 < m23 ? m01 : m23;
            if (m != kWsEmptyKey) atomicMin(a.result + tid, m);
        }
    }
}

// the one table of instantiations: [psi^-1][mask][volumes][nontemporal]
typedef void (*WsKernel)(WsArgs);
#define WS_ROW(I, M, V) {warp_stats_kernel<I, M, V, false>, warp_stats_kernel<I, M, V, true>}
const WsKernel kWsKernels[2][2][2][2] = {{{WS_ROW(false, false, false), WS_ROW(false, false, true)}, {WS_ROW(false, true, false), WS_ROW(false, true, true)}},
                                         {{WS_ROW(true, false, false), WS_ROW(true, false, true)}, {WS_ROW(true, true, false), WS_ROW(true, true, true)}}};
#undef WS_ROW

}  // namespace

extern "C" {

int sobfu_hip_warp_stats(const float* d_psi, const float* d_psi_inv, const float* d_mask_det, const float* d_mask_res, int X, int Y, int Z,
                         const float voxel_size[3], float band, const float* edges, int n_edges, float res_tol, unsigned long long* d_result,
                         float* d_det, float* d_res, void* stream) {
    SOBFU_CHECK_ARGS(d_psi && d_result && voxel_size && aligned(d_psi, 0, 16) && aligned(d_psi_inv, 0, 16) && aligned(d_mask_det, 0, 8) &&
                     aligned(d_mask_res, 0, 8) && aligned(d_result, 0, 8) && aligned(d_det, 0, 4) && aligned(d_res, 0, 4));
    SOBFU_CHECK_ARGS(d_psi_inv || (!d_res && !d_mask_res));
    SOBFU_CHECK_ARGS(X > 0 && Y > 0 && Z > 0 && (long long) X * Y <= kWsMaxVoxels && (long long) X * Y * Z <= kWsMaxVoxels);
    SOBFU_CHECK_ARGS(positive_finite(voxel_size[0]) && positive_finite(voxel_size[1]) && positive_finite(voxel_size[2]) && positive_finite(band));
    SOBFU_CHECK_ARGS(res_tol >= 0.f && n_edges >= 0 && n_edges <= kWsMaxEdges && (n_edges == 0 || edges));
    for (int k = 0; k < n_edges; ++k) SOBFU_CHECK_ARGS(std::isfinite(edges[k]) && (k == 0 || edges[k] > edges[k - 1]));

    WsArgs a{(const float4*) d_psi, (const float4*) d_psi_inv, (const float2*) d_mask_det, (const float2*) d_mask_res, WsDims{X, Y, Z},
             {voxel_size[0], voxel_size[1], voxel_size[2]}, band, {}, res_tol, d_result, d_det, d_res, ws_launch(X, Y, Z)};
    for (int k = 0; k < kWsMaxEdges; ++k) a.edges[k] = k < n_edges ? edges[k] : -INFINITY;
    hipStream_t st = (hipStream_t) stream;
    SOBFU_HIP_TRY(hipMemsetAsync(d_result, 0, SOBFU_WS_WORDS * sizeof(unsigned long long), st));
    SOBFU_HIP_TRY(hipMemsetAsync(d_result + kAccKeys, 0xff, (kAcc - kAccKeys) * sizeof(unsigned long long), st));  // kWsEmptyKey
    const WsKernel kern = kWsKernels[d_psi_inv != nullptr][d_mask_det || d_mask_res][d_det || d_res][launcher_streams(X, Y, Z)];
    hipLaunchKernelGGL(kern, dim3((unsigned) ws_workgroups(a.l)), dim3(kWsTileX, kWsTileY), 0, st, a);
    return (int) hipGetLastError();
}

}  // extern "C"
