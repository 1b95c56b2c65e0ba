// CPU-only driver of the ray-triangle rule (sobfu_amd/csrc/sobfu_mesh_ray.hpp as a host compiler takes it, -ffp-contract=off like the
// kernels) for tests/test_mesh_ray_cpu.py:
//   mesh_ray_tool IN.bin OUT.bin   IN = int32 n, int32 T, float32 t_min, float32 t_max (<= 0: unlimited), n x 6 float32 (origin,
//                                  direction), T x 9 float32 (a, b, c); OUT = per ray float32 t, int32 tri, float32 u, v, int32 side:
//                                  the minimum t over the triangles in ascending order, the first triangle attaining it
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sobfu_mesh_ray.hpp"

using sobfu_hip::P3;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: %s IN.bin OUT.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t n = 0, T = 0;
    float lim[2] = {0.f, 0.f};
    if (!f || std::fread(&n, 4, 1, f) != 1 || std::fread(&T, 4, 1, f) != 1 || std::fread(lim, 4, 2, f) != 2 || n < 0 || T < 0) return 2;
    std::vector<float> rays(6 * (size_t) n), tris(9 * (size_t) T);
    const bool ok = std::fread(rays.data(), 4, rays.size(), f) == rays.size() && std::fread(tris.data(), 4, tris.size(), f) == tris.size();
    std::fclose(f);
    if (!ok) return 2;
    const float t_min = lim[0], t_max = lim[1] > 0.f ? lim[1] : INFINITY;
    struct Out {
        float t;
        int32_t tri;
        float u, v;
        int32_t side;
    };
    std::vector<Out> out((size_t) n);
    for (size_t i = 0; i < (size_t) n; ++i) {
        const float* r = &rays[6 * i];
        const sobfu_hip::Ray ray = sobfu_hip::ray_setup(P3{r[0], r[1], r[2]}, P3{r[3], r[4], r[5]});
        Out best{INFINITY, -1, 0.f, 0.f, 0};
        for (size_t k = 0; ray.valid && k < (size_t) T; ++k) {
            const float* c = &tris[9 * k];
            const sobfu_hip::RayHit h = sobfu_hip::ray_triangle(ray, P3{c[0], c[1], c[2]}, P3{c[3], c[4], c[5]}, P3{c[6], c[7], c[8]}, t_min, t_max);
            if (h.t < best.t) best = Out{h.t, (int32_t) k, h.u, h.v, h.side};
        }
        out[i] = best;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool wrote = out.empty() || std::fwrite(out.data(), sizeof(Out), out.size(), f) == out.size();
    return (std::fclose(f) == 0 && wrote) ? 0 : 2;
}
