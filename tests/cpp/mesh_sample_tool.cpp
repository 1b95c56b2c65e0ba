// CPU-only driver of the mesh sampling rule (sobfu_amd/csrc/sobfu_mesh_sample.hpp, no HIP; built with -ffp-contract=off, as the kernels
// are): the header's area, count and sample on the host, for tests/test_mesh_sample_cpu.py to compare with tests/mesh_sample_reference.py.
//   mesh_sample_tool IN OUT
//   IN:  int32 n_vertices, n_triangles; float64 density; uint64 seed; n_vertices x 4 float32; n_triangles x 3 int32
//   OUT: n_triangles float64 areas; n_triangles int64 counts; int64 N; N x 4 float32 points; N int32 triangles; N x 2 float32 (r1, r2)
// A face index outside [0, n_vertices) or a non-finite corner ends the run with status 3 (the kernels raise their flag for these).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sobfu_mesh_sample.hpp"

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

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t sizes[2];
    double density;
    uint64_t seed;
    std::vector<float> verts;
    std::vector<int32_t> faces;
    const bool ok = std::fread(sizes, sizeof sizes, 1, in) == 1 && sizes[0] >= 0 && sizes[1] >= 0 && std::fread(&density, sizeof density, 1, in) == 1 &&
                    std::fread(&seed, sizeof seed, 1, in) == 1 && read_n(in, verts, 4 * (size_t) sizes[0]) && read_n(in, faces, 3 * (size_t) sizes[1]);
    std::fclose(in);
    if (!ok || !(density >= 0.0) || !std::isfinite(density)) return 2;
    const int nv = sizes[0], nt = sizes[1];
    auto corner = [&](int i) { return P3{verts[4 * (size_t) i], verts[4 * (size_t) i + 1], verts[4 * (size_t) i + 2]}; };
    std::vector<double> areas((size_t) nt);
    std::vector<int64_t> counts((size_t) nt), total(1, 0);
    for (int t = 0; t < nt; ++t) {
        for (int j = 0; j < 3; ++j) {
            const int i = faces[3 * (size_t) t + j];
            if (i < 0 || i >= nv) return 3;
            const P3 p = corner(i);
            if (!(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) return 3;
        }
        areas[t]  = triangle_area(corner(faces[3 * (size_t) t]), corner(faces[3 * (size_t) t + 1]), corner(faces[3 * (size_t) t + 2]));
        counts[t] = sample_count(areas[t], density, seed, t);
        total[0] += counts[t];
    }
    if (total[0] > (int64_t) 1 << 26) return 4;  // a test's meshes stay far below
    std::vector<float> points, bary;
    std::vector<int32_t> tri;
    for (int t = 0; t < nt; ++t)
        for (int64_t k = 0; k < counts[t]; ++k) {
            const MeshSample s = sample_point(corner(faces[3 * (size_t) t]), corner(faces[3 * (size_t) t + 1]), corner(faces[3 * (size_t) t + 2]), seed, t, (int) k);
            const float p[4] = {s.p.x, s.p.y, s.p.z, 1.f};
            points.insert(points.end(), p, p + 4);
            tri.push_back(t);
            bary.push_back(s.r1), bary.push_back(s.r2);
        }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool wrote = write_n(out, areas) && write_n(out, counts) && write_n(out, total) && write_n(out, points) && write_n(out, tri) && write_n(out, bary);
    return std::fclose(out) == 0 && wrote ? 0 : 2;
}
