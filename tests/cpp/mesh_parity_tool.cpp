// CPU-only driver of the row-crossing rule (sobfu_amd/csrc/sobfu_mesh_parity.hpp as a host compiler takes it, -ffp-contract=off like the
// kernels) for tests/test_mesh_parity_cpu.py:
//   mesh_parity_tool IN.bin OUT.bin   IN = int32 n, int32 T, n x 2 float32 (py, pz), T x 9 float32 (a, b, c); OUT = n x T uint8 crossing
//                                     flags, then n x T float64 X (0 where there is no crossing), row by row
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sobfu_mesh_parity.hpp"

using sobfu_hip::P3;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: %s IN.bin OUT.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t n = 0, T = 0;
    if (!f || std::fread(&n, 4, 1, f) != 1 || std::fread(&T, 4, 1, f) != 1 || n < 0 || T < 0) return 2;
    std::vector<float> rows(2 * (size_t) n), tris(9 * (size_t) T);
    const bool ok = std::fread(rows.data(), 4, rows.size(), f) == rows.size() && std::fread(tris.data(), 4, tris.size(), f) == tris.size();
    std::fclose(f);
    if (!ok) return 2;
    std::vector<uint8_t> hit((size_t) n * T);
    std::vector<double> X((size_t) n * T);
    for (size_t i = 0; i < (size_t) n; ++i)
        for (size_t k = 0; k < (size_t) T; ++k) {
            const float* c = &tris[9 * k];
            const sobfu_hip::SignedCrossing x =
                sobfu_hip::signed_row_crossing(P3{c[0], c[1], c[2]}, P3{c[3], c[4], c[5]}, P3{c[6], c[7], c[8]}, rows[2 * i], rows[2 * i + 1]);
            hit[i * T + k] = x.sign != 0 ? 1 : 0;  // a crossing is sign != 0
            X[i * T + k]   = x.sign != 0 ? x.X : 0.0;
        }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool wrote = hit.empty() || (std::fwrite(hit.data(), 1, hit.size(), f) == hit.size() && std::fwrite(X.data(), 8, X.size(), f) == X.size());
    return (std::fclose(f) == 0 && wrote) ? 0 : 2;
}
