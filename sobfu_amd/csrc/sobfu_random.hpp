// Counter-based random numbers for the frame-side kernels (depth_sensor_kernels.hip): Philox4x32-10 (Salmon, Moraes,
// Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain integer arithmetic, and the two variates made from its words.
// tests/depth_sensor_reference.py restates all of it; the variates use integers until their last step, so numpy gives the same bits.
// Plain integers and floats, no HIP types: a host compiler takes this header too.
//
//   philox   ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), M0 = 0xD2511F53,
//            M1 = 0xCD9E8D57; the key grows by (0x9E3779B9, 0xBB67AE85) between rounds
//   draw     of pixel (u, v) (column, row), frame f, stream s under a 64-bit seed: philox(counter (u, v, f, s), key (seed & 0xffffffff,
//            seed >> 32)).  It depends on nothing else: not the pitch, the tile, the launch shape or the image size
//   normal   S = the sum of the eight 16-bit halves of the four words; g = float(S - 262140) * kNormalScale, kNormalScale =
//            1 / sqrt(8 (65536^2 - 1) / 12) rounded to fp32: an Irwin-Hall variate of variance 1 and support about +-4.9, not a Gaussian
//            tail -- chosen so that it needs neither log nor cos
//   uniform  of a word w: float(w >> 8) * 2^-24, in [0, 1)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SOBFU_RNG_FN __host__ __device__ __forceinline__
#else
#define SOBFU_RNG_FN inline
#endif

namespace sobfu_hip {

struct Philox {
    uint32_t w[4];
};

constexpr float kNormalScale = 0x1.3988e2p-16f;

SOBFU_RNG_FN Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t) p1, c2 = n2, c3 = (uint32_t) p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

SOBFU_RNG_FN Philox pixel_draw(uint64_t seed, uint32_t frame, int u, int v, uint32_t stream) {
    return philox4x32_10((uint32_t) u, (uint32_t) v, frame, stream, (uint32_t) (seed & 0xffffffffu), (uint32_t) (seed >> 32));
}

SOBFU_RNG_FN float normal_variate(const Philox& r) {
    int s = 0;
    for (int i = 0; i < 4; ++i) s += (int) (r.w[i] & 0xffffu) + (int) (r.w[i] >> 16);
    return (float) (s - 262140) * kNormalScale;
}

SOBFU_RNG_FN float uniform_variate(uint32_t w) { return (float) (w >> 8) * 0x1p-24f; }

}  // namespace sobfu_hip
