// CPU-only driver of sobfu_amd::write_png_rgb (include/sobfu_amd/depth_io.hpp): writes a rows x cols test pattern whose byte
// (y, x, c) is (7 * y + 13 * x + 101 * c) mod 256, so the test can check every pixel of the decoded file.
//   png_write_tool <out.png> <rows> <cols>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <sobfu_amd/depth_io.hpp>

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <out.png> <rows> <cols>\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    if (rows < 1 || cols < 1) return 2;
    std::vector<uint8_t> rgb((size_t) rows * cols * 3);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x)
            for (int c = 0; c < 3; ++c) rgb[((size_t) y * cols + x) * 3 + c] = (uint8_t) ((7 * y + 13 * x + 101 * c) & 255);
    return sobfu_amd::write_png_rgb(argv[1], rows, cols, rgb.data()) ? 0 : 1;
}
