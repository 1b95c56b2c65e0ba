// CPU-only driver of the warp-field diagnostics' rules (sobfu_amd/csrc/sobfu_warp_stats.hpp, no HIP; built with -ffp-contract=off, as the
// kernels are): the header's det, lengths, sampler, sums and keys on the host, voxel by voxel in linear order, for
// tests/test_warp_stats_cpu.py to compare with tests/warp_stats_reference.py.
//   warp_stats_tool IN OUT
//   IN:  int32 X, Y, Z, has_psi_inv, has_mask_det, has_mask_res, n_edges; float32 voxel_size[3], band, res_tol, edges[16];
//        psi (X Y Z x 4 float32); then, each when present, psi_inv (x 4), mask_det (x 2), mask_res (x 2)
//   OUT: 64 uint64 result words (the layout of include/sobfu_hip.h); X Y Z float32 det; with psi_inv, X Y Z float32 residuals
//   "launch X Y Z" instead prints ws_launch's gx gy chunks zc and checks that ws_tile visits every (tile, chunk) exactly once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sobfu_hip.h"
#include "sobfu_warp_stats.hpp"

using namespace sobfu_hip;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool write_n(FILE* f, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

static int launch(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1 || (long long) X * Y * Z > kWsMaxVoxels) return 2;
    const WsLaunch l = ws_launch(X, Y, Z);
    const unsigned long long n = ws_workgroups(l);
    std::printf("%u %u %u %d\n", l.gx, l.gy, l.chunks, l.zc);
    if (n > (1u << 24)) return 4;
    std::vector<unsigned char> seen((size_t) n, 0);
    for (unsigned w = 0; w < (unsigned) n; ++w) {
        unsigned bx, by, bz;
        ws_tile(w, l, bx, by, bz);
        if (bx >= l.gx || by >= l.gy || bz >= l.chunks) return 3;
        unsigned char& s = seen[(size_t) bx + (size_t) l.gx * (by + (size_t) l.gy * bz)];
        if (s) return 3;
        s = 1;
    }
    return (long long) l.chunks * l.zc >= Z && (long long) (l.chunks - 1) * l.zc < Z ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "launch")) return launch(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
    if (argc != 3) {
        std::printf("usage: %s IN OUT | launch X Y Z\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t h[7];
    float f[5 + kWsMaxEdges];
    std::vector<float> psi, inv, mdet, mres;
    bool ok = std::fread(h, sizeof h, 1, in) == 1 && std::fread(f, sizeof f, 1, in) == 1 && h[0] > 0 && h[1] > 0 && h[2] > 0 &&
              (long long) h[0] * h[1] * h[2] <= (1 << 24) && h[6] >= 0 && h[6] <= kWsMaxEdges;
    const size_t n = ok ? (size_t) h[0] * h[1] * h[2] : 0;
    ok = ok && read_n(in, psi, 4 * n) && read_n(in, inv, h[3] ? 4 * n : 0) && read_n(in, mdet, h[4] ? 2 * n : 0) && read_n(in, mres, h[5] ? 2 * n : 0);
    std::fclose(in);
    if (!ok) return 2;
    const WsDims d{h[0], h[1], h[2]};
    const float vs[3] = {f[0], f[1], f[2]}, band = f[3], res_tol = f[4];
    const float* edges = f + 5;
    auto at = [&](int x, int y, int z) { return (size_t) x + (size_t) d.x * ((size_t) y + (size_t) d.y * (size_t) z); };
    auto disp = [&](int x, int y, int z) {
        const float* p = &psi[4 * at(x, y, z)];
        return ws_disp(p[0], p[1], p[2], x, y, z);
    };
    std::vector<uint64_t> words(SOBFU_WS_WORDS, 0);
    for (int k = SOBFU_WS_DET_MIN_KEY; k <= SOBFU_WS_RES_MAX_KEY; ++k) words[k] = kWsEmptyKey;
    WsSum det_sum{0, 0}, disp_sum{0, 0}, res_sum{0, 0};
    auto least = [&](int word, uint64_t key) { words[word] = key < words[word] ? key : words[word]; };
    std::vector<float> det_vol(n), res_vol(h[3] ? n : 0);
    for (int z = 0; z < d.z; ++z)
        for (int y = 0; y < d.y; ++y)
            for (int x = 0; x < d.x; ++x) {
                const size_t i = at(x, y, z);
                const uint32_t index = (uint32_t) i;
                int lo, hi;
                bool halved;
                ws_axis(d.x, x, lo, hi, halved);
                const WsV3 dx = ws_deriv(disp(lo, y, z), disp(hi, y, z), halved, d.x == 1);
                ws_axis(d.y, y, lo, hi, halved);
                const WsV3 dy = ws_deriv(disp(x, lo, z), disp(x, hi, z), halved, d.y == 1);
                ws_axis(d.z, z, lo, hi, halved);
                const WsV3 dz = ws_deriv(disp(x, y, lo), disp(x, y, hi), halved, d.z == 1);
                const float det = ws_det(dx, dy, dz);
                det_vol[i] = ws_canonical(det);
                if (!h[4] || ws_in_mask(mdet[2 * i], mdet[2 * i + 1], band)) {
                    if (ws_finite(det)) {
                        ++words[SOBFU_WS_N_DET];
                        words[SOBFU_WS_N_FOLD] += det <= 0.f;
                        for (int k = 0; k < h[6]; ++k) words[SOBFU_WS_DET_BELOW + k] += det < edges[k];
                        ws_add(det_sum, det);
                        least(SOBFU_WS_DET_MIN_KEY, ws_min_key(det, index));
                        least(SOBFU_WS_DET_MAX_KEY, ws_max_key(det, index));
                    } else {
                        ++words[SOBFU_WS_N_DET_NONFINITE];
                    }
                    const float len = ws_len(disp(x, y, z), vs);
                    if (ws_finite(len)) {
                        ++words[SOBFU_WS_N_DISP];
                        ws_add(disp_sum, len);
                        least(SOBFU_WS_DISP_MAX_KEY, ws_max_key(len, index));
                    } else {
                        ++words[SOBFU_WS_N_DISP_NONFINITE];
                    }
                }
                if (h[3]) {
                    float len;
                    const int cls = ws_residual(disp, d, inv[4 * i], inv[4 * i + 1], inv[4 * i + 2], x, y, z, vs, &len);
                    res_vol[i] = len;
                    if (!h[5] || ws_in_mask(mres[2 * i], mres[2 * i + 1], band)) {
                        if (cls == kWsResOk) {
                            ++words[SOBFU_WS_N_RES];
                            words[SOBFU_WS_N_RES_ABOVE] += len > res_tol;
                            ws_add(res_sum, len);
                            least(SOBFU_WS_RES_MAX_KEY, ws_max_key(len, index));
                        } else {
                            ++words[cls == kWsResOutside ? SOBFU_WS_N_RES_OUTSIDE : SOBFU_WS_N_RES_NONFINITE];
                        }
                    }
                }
            }
    words[SOBFU_WS_DET_SUM_HI] = (uint64_t) det_sum.hi, words[SOBFU_WS_DET_SUM_LO] = (uint64_t) det_sum.lo;
    words[SOBFU_WS_DISP_SUM_HI] = (uint64_t) disp_sum.hi, words[SOBFU_WS_DISP_SUM_LO] = (uint64_t) disp_sum.lo;
    words[SOBFU_WS_RES_SUM_HI] = (uint64_t) res_sum.hi, words[SOBFU_WS_RES_SUM_LO] = (uint64_t) res_sum.lo;
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool wrote = write_n(out, words) && write_n(out, det_vol) && write_n(out, res_vol);
    return std::fclose(out) == 0 && wrote ? 0 : 2;
}
