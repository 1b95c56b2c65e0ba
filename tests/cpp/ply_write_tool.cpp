// CPU-only driver of sobfu_amd::write_ply (include/sobfu_amd/sobfu.hpp) for tests/test_mc_indexed_cpu.py: writes the test mesh of
// n vertices and f faces that the test also builds in numpy -- vertex i = (0.5 i, -i, 0.25 i + 1), normal i = (i / (i + 1), -1 / (i + 1),
// 0.5), face k = (k, k + 1, k + 2) mod n, colour i (b, g, r) = (7 i, 13 i + 1, 29 i + 2) mod 256 when coloured != 0.
//   ply_write_tool <out.ply> <n> <f> <coloured>
#include <cstdio>
#include <cstdlib>

#include <sobfu_amd/sobfu.hpp>

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <out.ply> <vertices> <faces> <coloured>\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[2]), nf = std::atoi(argv[3]);
    const bool coloured = std::atoi(argv[4]) != 0;
    if (n < 0 || nf < 0 || (nf > 0 && n == 0)) return 2;
    sobfu_amd::IndexedMesh m;
    for (int i = 0; i < n; ++i) {
        const float fi = (float) i;
        float4 v, nn;
        v.x = fi * 0.5f, v.y = -fi, v.z = fi * 0.25f + 1.f, v.w = 1.f;
        nn.x = fi / (fi + 1.f), nn.y = -1.f / (fi + 1.f), nn.z = 0.5f, nn.w = 1.f;
        m.vertices.push_back(v);
        m.normals.push_back(nn);
        if (coloured) {
            kfusion::RGB c;
            c.bgra = 0;
            c.b = (unsigned char) ((7 * i) & 255), c.g = (unsigned char) ((13 * i + 1) & 255), c.r = (unsigned char) ((29 * i + 2) & 255);
            m.colours.push_back(c);
        }
    }
    for (int k = 0; k < nf; ++k)
        for (int c = 0; c < 3; ++c) m.faces.push_back((k + c) % n);
    return sobfu_amd::write_ply(argv[1], m) ? 0 : 1;
}
