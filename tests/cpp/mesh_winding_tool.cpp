// CPU-only driver of the winding-number rule and the boundary chain (sobfu_amd/csrc/sobfu_mesh_winding.hpp and sobfu_mesh_boundary.hpp as a
// host compiler takes them, -ffp-contract=off like the kernels) for tests/test_mesh_winding_cpu.py:
//   mesh_winding_tool crossings IN OUT   IN = int32 n, int32 T, n x 2 float32 (py, pz), T x 9 float32 (a, b, c); OUT = n x T int8 signs (0: no
//                                        crossing), then n x T float64 X (0 where there is none), row by row
//   mesh_winding_tool strips IN OUT      IN = int32 n, int32 B, n x 3 float32 points, B x 6 float32 (u, v); OUT = n x B float64 strip angles
//   mesh_winding_tool triangles IN OUT   IN = int32 n, int32 T, n x 3 float32 points, T x 9 float32; OUT = n x T float64 solid angles
//   mesh_winding_tool seams IN OUT       IN = int32 n, int32 V, n x 3 float32 points, V x 3 float32 vertices; OUT = n x V uint8
//   mesh_winding_tool boundary IN OUT    IN = int32 T, int32 V, T x 3 int32 faces; OUT = int32 ok, int32 B, B x 3 int32 (u, v, k)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sobfu_mesh_boundary.hpp"
#include "sobfu_mesh_winding.hpp"

using sobfu_hip::P3;

namespace {

template <class T> bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> bool write_n(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
P3 p3(const float* c) { return P3{c[0], c[1], c[2]}; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::printf("usage: %s crossings|strips|triangles|seams|boundary IN.bin OUT.bin\n", argv[0]);
        return 2;
    }
    const std::string what = argv[1];
    FILE* f = std::fopen(argv[2], "rb");
    int32_t n = 0, m = 0;
    if (!f || std::fread(&n, 4, 1, f) != 1 || std::fread(&m, 4, 1, f) != 1 || n < 0 || m < 0) return 2;
    const size_t N = (size_t) n, M = (size_t) m;
    std::vector<float> first, second;
    std::vector<int32_t> faces;
    bool ok = false;
    if (what == "boundary") ok = read_n(f, faces, 3 * N);
    else ok = read_n(f, first, (what == "crossings" ? 2 : 3) * N) && read_n(f, second, (what == "strips" ? 6 : what == "seams" ? 3 : 9) * M);
    std::fclose(f);
    if (!ok) return 2;
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    bool wrote = false;
    if (what == "crossings") {
        std::vector<int8_t> sign(N * M);
        std::vector<double> X(N * M);
        for (size_t i = 0; i < N; ++i)
            for (size_t k = 0; k < M; ++k) {
                const float* c = &second[9 * k];
                const sobfu_hip::SignedCrossing x = sobfu_hip::signed_row_crossing(p3(c), p3(c + 3), p3(c + 6), first[2 * i], first[2 * i + 1]);
                sign[i * M + k] = (int8_t) x.sign, X[i * M + k] = x.sign ? x.X : 0.0;
            }
        wrote = write_n(o, sign) && write_n(o, X);
    } else if (what == "strips" || what == "triangles") {
        std::vector<double> out(N * M);
        for (size_t i = 0; i < N; ++i)
            for (size_t k = 0; k < M; ++k) {
                const P3 p = p3(&first[3 * i]);
                if (what == "strips") {
                    out[i * M + k] = sobfu_hip::strip_angle(p3(&second[6 * k]), p3(&second[6 * k + 3]), p);
                } else {
                    const float* c = &second[9 * k];
                    out[i * M + k] = sobfu_hip::triangle_angle(sobfu_hip::from(p3(c), p), sobfu_hip::from(p3(c + 3), p), sobfu_hip::from(p3(c + 6), p));
                }
            }
        wrote = write_n(o, out);
    } else if (what == "seams") {
        std::vector<uint8_t> out(N * M);
        for (size_t i = 0; i < N; ++i)
            for (size_t k = 0; k < M; ++k) out[i * M + k] = sobfu_hip::seam_point(p3(&second[3 * k]), p3(&first[3 * i])) ? 1 : 0;
        wrote = write_n(o, out);
    } else if (what == "boundary") {
        std::vector<sobfu_hip::BoundaryEdge> edges;
        const bool fine = sobfu_hip::mesh_boundary(faces.data(), n, m, &edges);
        std::vector<int32_t> out{fine ? 1 : 0, fine ? (int32_t) edges.size() : 0};
        for (size_t i = 0; fine && i < edges.size(); ++i) out.push_back(edges[i].u), out.push_back(edges[i].v), out.push_back(edges[i].k);
        wrote = write_n(o, out);
    }
    return (std::fclose(o) == 0 && wrote) ? 0 : 2;
}
