// Driver of the evaluation shells for the tests (include/sobfu_amd/evaluate.hpp):
//   mesh_eval_tool read FILE.ply PREFIX            read_ply -> "ok <V> <F> <normals 0|1> <colours 0|1>" and PREFIX.v / .n (float32 x 4),
//                                                  PREFIX.f (int32 x 3), PREFIX.c (uint8 BGRA); a refusal prints "refused: <why>", exit 1
//   mesh_eval_tool closest IN.bin OUT.bin          the point-triangle rule on the CPU (sobfu_amd/csrc/sobfu_mesh_distance.hpp as a host
//                                                  compiler takes it): IN = int32 n, then n x 12 float32 (p, a, b, c); OUT = n x 4 float32 (q, d2)
//   mesh_eval_tool compare A.ply B.ply MAX PREFIX  compare_meshes on the GPU -> its line at 17 digits; PREFIX.ab / .ba: the float32 distances
// read and closest run without a GPU.
#include <cstdio>
#include <string>
#include <vector>

#include "sobfu_amd/sobfu.hpp"
#include "sobfu_mesh_distance.hpp"

template <class T>
static bool dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return (std::fclose(f) == 0) && ok;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "read" && argc == 4) {
        sobfu_amd::IndexedMesh m;
        std::string why;
        if (!sobfu_amd::read_ply(argv[2], m, &why)) {
            std::printf("refused: %s\n", why.c_str());
            return 1;
        }
        const std::string pre = argv[3];
        if (!dump(pre + ".v", m.vertices) || !dump(pre + ".n", m.normals) || !dump(pre + ".f", m.faces) || !dump(pre + ".c", m.colours)) return 2;
        std::printf("ok %zu %zu %d %d\n", m.vertices.size(), m.triangles(), (int) !m.normals.empty(), (int) !m.colours.empty());
        return 0;
    }
    if (cmd == "closest" && argc == 4) {
        FILE* f = std::fopen(argv[2], "rb");
        int n = 0;
        if (!f || std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
        std::vector<float> in(12 * (size_t) n), out(4 * (size_t) n);
        const bool ok = std::fread(in.data(), 4, in.size(), f) == in.size();
        std::fclose(f);
        if (!ok) return 2;
        for (size_t i = 0; i < (size_t) n; ++i) {
            const float* r = &in[12 * i];
            const sobfu_hip::Closest c = sobfu_hip::closest_on_triangle(sobfu_hip::P3{r[0], r[1], r[2]}, sobfu_hip::P3{r[3], r[4], r[5]},
                                                                        sobfu_hip::P3{r[6], r[7], r[8]}, sobfu_hip::P3{r[9], r[10], r[11]});
            out[4 * i] = c.q.x, out[4 * i + 1] = c.q.y, out[4 * i + 2] = c.q.z, out[4 * i + 3] = c.d2;
        }
        return dump(argv[3], out) ? 0 : 2;
    }
    if (cmd == "compare" && argc == 6) {
        sobfu_amd::IndexedMesh a, b;
        std::string why;
        if (!sobfu_amd::read_ply(argv[2], a, &why) || !sobfu_amd::read_ply(argv[3], b, &why)) {
            std::printf("refused: %s\n", why.c_str());
            return 1;
        }
        kfusion::cuda::setDevice(0);
        sobfu_amd::MeshComparison r;
        std::vector<float> ab, ba;
        if (!sobfu_amd::compare_meshes(a, b, std::strtof(argv[4], nullptr), r, &ab, &ba, &why)) {
            std::printf("refused: %s\n", why.c_str());
            return 1;
        }
        const std::string pre = argv[5];
        if (!dump(pre + ".ab", ab) || !dump(pre + ".ba", ba)) return 2;
        std::printf("%s\n", sobfu_amd::format_comparison(r, 17).c_str());
        return 0;
    }
    std::printf("usage: %s read FILE.ply PREFIX | closest IN.bin OUT.bin | compare A.ply B.ply MAX_DIST PREFIX\n", argv[0]);
    return 2;
}
