// Driver of the C++ twin of the depth sensor model (sobfu_amd::SensorModel, sobfu_amd::depth_sensor; needs a GPU) for
// tests/test_gpu_depth_sensor.py:
//   depth_sensor_tool kinect|ideal SEED FRAME IN.bin OUT.bin [name=value ...]
//     IN  = int32 rows, int32 cols, rows x cols x 4 float32 points, rows x cols x 4 float32 normals
//     OUT = rows x cols uint16 depth, rows x cols uint8 flags
//     name=value: a field of the model, as apps/sobfu_headless --sensor-set takes it
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <sobfu_amd/sobfu.hpp>

int main(int argc, char** argv) {
    if (argc < 6) {
        std::printf("usage: %s kinect|ideal SEED FRAME IN.bin OUT.bin [name=value ...]\n", argv[0]);
        return 2;
    }
    const std::string name = argv[1];
    if (name != "kinect" && name != "ideal") return 2;
    sobfu_amd::SensorModel model = name == "kinect" ? sobfu_amd::SensorModel::kinect() : sobfu_amd::SensorModel::ideal();
    for (int i = 6; i < argc; ++i) {
        const std::string kv = argv[i];
        const size_t eq = kv.find('=');
        if (eq == std::string::npos || !model.set(kv.substr(0, eq), std::strtod(kv.c_str() + eq + 1, nullptr))) {
            std::printf("no field %s\n", kv.c_str());
            return 2;
        }
    }
    FILE* f = std::fopen(argv[4], "rb");
    int32_t size[2] = {0, 0};
    if (!f || std::fread(size, 4, 2, f) != 2 || size[0] < 1 || size[1] < 1) return 2;
    const size_t n = (size_t) size[0] * size[1];
    std::vector<float4> points(n), normals(n);
    const bool ok = std::fread(points.data(), 16, n, f) == n && std::fread(normals.data(), 16, n, f) == n;
    std::fclose(f);
    if (!ok) return 2;
    kfusion::cuda::Cloud dp;
    kfusion::cuda::Normals dn;
    kfusion::cuda::Depth depth;
    kfusion::cuda::DeviceArray2D<unsigned char> flags;
    dp.upload(points.data(), (size_t) size[1] * 16, size[0], size[1]);
    dn.upload(normals.data(), (size_t) size[1] * 16, size[0], size[1]);
    if (!sobfu_amd::depth_sensor(dp, dn, model, std::strtoull(argv[2], nullptr, 0), (uint32_t) std::strtoul(argv[3], nullptr, 0), depth, &flags)) {
        std::printf("a parameter is outside its range\n");
        return 3;
    }
    std::vector<uint16_t> hd(n);
    std::vector<uint8_t> hf(n);
    depth.download(hd.data(), (size_t) size[1] * 2);
    flags.download(hf.data(), (size_t) size[1]);
    f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    const bool wrote = std::fwrite(hd.data(), 2, n, f) == n && std::fwrite(hf.data(), 1, n, f) == n;
    return (std::fclose(f) == 0 && wrote) ? 0 : 2;
}
