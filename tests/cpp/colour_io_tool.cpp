// CPU-only driver of the colour I/O (tests/test_colour_cpu.py):
//   colour_io_tool read <file> <rows> <cols> <out.raw>   sobfu_amd::read_colour -> raw BGRA bytes; on failure "error: <why>", exit 1
//   colour_io_tool vtk <out.vtk> <n> <coloured>          sobfu_amd::write_vtk of n vertices (x, y, z) = (0.5 i, -0.25 i, i / 3), with
//                                                        colours (b, g, r) = (i, 2 i, 3 i) mod 256 when coloured != 0
//   colour_io_tool npy <out.npy> <d0> <d1> ...            the uint8 write_npy of the ramp i mod 256
#include <sobfu_amd/depth_io.hpp>
#include <sobfu_amd/sobfu.hpp>

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (argc == 6 && cmd == "read") {
        std::vector<uint8_t> px;
        std::string why;
        if (!sobfu_amd::read_colour(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), px, &why)) {
            std::printf("error: %s\n", why.c_str());
            return 1;
        }
        FILE* f = std::fopen(argv[5], "wb");
        if (!f) return 2;
        std::fwrite(px.data(), 1, px.size(), f);
        return std::fclose(f) == 0 ? 0 : 2;
    }
    if (argc == 5 && cmd == "vtk") {
        sobfu_amd::TriangleMesh m;
        const int n = std::atoi(argv[3]);
        for (int i = 0; i < n; ++i) {
            float4 v;
            v.x = 0.5f * (float) i, v.y = -0.25f * (float) i, v.z = (float) i / 3.f, v.w = 1.f;
            m.vertices.push_back(v);
            if (std::atoi(argv[4])) {
                kfusion::RGB c;
                c.b = (unsigned char) (i & 255), c.g = (unsigned char) ((2 * i) & 255), c.r = (unsigned char) ((3 * i) & 255);
                m.colours.push_back(c);
            }
        }
        return sobfu_amd::write_vtk(argv[2], m) ? 0 : 1;
    }
    if (argc >= 4 && cmd == "npy") {
        std::vector<size_t> shape;
        size_t n = 1;
        for (int i = 3; i < argc; ++i) { shape.push_back((size_t) std::atol(argv[i])); n *= shape.back(); }
        std::vector<uint8_t> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = (uint8_t) (i & 255);
        return sobfu_amd::write_npy(argv[2], v.data(), shape) ? 0 : 1;
    }
    std::printf("usage: colour_io_tool read <file> <rows> <cols> <out.raw> | vtk <out.vtk> <n> <coloured> | npy <out.npy> <dims...>\n");
    return 2;
}
