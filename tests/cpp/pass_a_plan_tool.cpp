// CPU-only driver of the warping march's launch plan (sobfu_amd/csrc/sobfu_geometry.hpp: plan_pass_a_warp), for
// tests/test_pass_a_warp_plan.py.  One grid "X Y Z" per input line, planned as launch_pass_a plans it (the whole grid as one marching box),
// one answer line each:
//   "ty T groups G first f.. | x0 x1 y0 y1 z0 z1 zc kind wpg rem pair | cover min MIN max MAX outside O"
// cover: every workgroup's cells are laid out as the kernel derives them from the plan (geom_in_box of solver_iter_common.inl, restated
// below: 64-lane x-tiles fastest, then y-tiles of T rows, then z-chunks, the first `rem` of them one plane longer) and counted per cell:
// MIN / MAX over the grid's cells, O = cells a workgroup would store outside the grid.  The tuning environment is the process's own.
#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sobfu_geometry.hpp"

using namespace sobfu_hip;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int X, Y, Z;
        if (!(in >> X >> Y >> Z)) continue;
        const LaunchBox whole{0, X, 0, Y, 0, Z, false};
        BoxList L{};
        const int groups = plan_pass_a_warp(L, &whole, 1);
        const int ty = kRPT * kWarpWY;
        std::cout << "ty " << ty << " groups " << groups << " first";
        for (int k = 0; k <= kMaxBoxes; ++k) std::cout << ' ' << L.first[k];
        std::vector<unsigned char> count((size_t) X * Y * Z, 0);  // saturating at 255
        long outside = 0;
        for (int i = 0; i < L.n; ++i) {
            const Box& b = L.b[i];
            std::cout << " | " << b.x0 << ' ' << b.x1 << ' ' << b.y0 << ' ' << b.y1 << ' ' << b.z0 << ' ' << b.z1 << ' ' << b.zc << ' ' << b.kind << ' '
                      << b.wpg << ' ' << b.rem << ' ' << b.pair;
            const unsigned ntu = (unsigned) ((b.x1 - b.x0 + TX - 1) / TX), ntv = (unsigned) ((b.y1 - b.y0 + ty - 1) / ty);
            for (unsigned t = 0; t < (unsigned) (L.first[i + 1] - L.first[i]); ++t) {
                const int u0 = b.x0 + (int) (t % ntu) * TX, v0 = b.y0 + (int) ((t / ntu) % ntv) * ty;
                const int ck = (int) (t / (ntu * ntv));
                const int zb = b.z0 + ck * b.zc + std::min(ck, b.rem), ze = std::min(zb + b.zc + (ck < b.rem ? 1 : 0), b.z1);
                for (int z = zb; z < ze; ++z)
                    for (int v = v0; v < std::min(v0 + ty, b.y1); ++v)
                        for (int u = u0; u < std::min(u0 + TX, b.x1); ++u) {
                            if (u < 0 || u >= X || v < 0 || v >= Y || z < 0 || z >= Z) ++outside;
                            else if (unsigned char& c = count[(size_t) u + (size_t) X * ((size_t) v + (size_t) Y * z)]; c < 255) ++c;
                        }
            }
        }
        const auto mm = std::minmax_element(count.begin(), count.end());
        std::cout << " | cover min " << (int) *mm.first << " max " << (int) *mm.second << " outside " << outside << "\n";
    }
    return 0;
}
