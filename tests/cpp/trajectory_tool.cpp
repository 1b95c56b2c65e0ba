// CPU-only driver of include/sobfu_amd/trajectory.hpp for tests/test_depth_sensor_cpu.py:
//   trajectory_tool EST.txt GT.txt [DELTA] [OUT.txt]   prints "ate=%.17g rpe_trans=%.17g rpe_rot=%.17g" of EST against GT (TUM format);
//                                                      OUT.txt: EST written back by write_tum
#include <cstdio>
#include <cstdlib>
#include <string>

#include <sobfu_amd/trajectory.hpp>

int main(int argc, char** argv) {
    if (argc < 3) {
        std::printf("usage: %s EST.txt GT.txt [DELTA] [OUT.txt]\n", argv[0]);
        return 2;
    }
    sobfu_amd::Trajectory est, gt;
    std::string why;
    if (!sobfu_amd::read_tum(argv[1], est, &why) || !sobfu_amd::read_tum(argv[2], gt, &why)) {
        std::printf("%s\n", why.c_str());
        return 2;
    }
    double trans = 0, rot = 0;
    if (!sobfu_amd::rpe(est, gt, &trans, &rot, argc > 3 ? std::atoi(argv[3]) : 1)) return 3;
    std::printf("ate=%.17g rpe_trans=%.17g rpe_rot=%.17g\n", sobfu_amd::ate(est, gt), trans, rot);
    if (argc > 4 && !sobfu_amd::write_tum(argv[4], est)) return 2;
    return 0;
}
