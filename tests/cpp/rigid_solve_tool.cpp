// CPU-only driver of sobfu_amd/csrc/sobfu_rigid.hpp (no HIP, built with -ffp-contract=off as the kernels are): the LDL^T solve, Rodrigues,
// the pose composition and the rigid inverse on records of doubles, for tests/test_mesh_align_cpu.py to compare bit for bit with
// tests/mesh_align_reference.py.
//   rigid_solve_tool MODE in.bin out.bin      in.bin: int32 count, then count records of doubles; out.bin: count records
//     ldlt6      36 A (row-major) + 6 b        -> doubles: 6 x, 6 D, det, ok (1 / 0)
//     ldlt3      9 A + 3 b                     -> doubles: 3 x, 3 D, det, ok
//     rodrigues  3 w                           -> doubles: 9 R, theta
//     compose    9 R, 3 t, 16 P (float values) -> 16 floats
//     inverse    16 P (float values)           -> 16 floats
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sobfu_rigid.hpp"

using namespace sobfu_hip;

template <int N>
static void ldlt_record(const double* in, std::vector<double>& out) {
    double A[N][N], b[N], x[N];
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < N; ++c) A[r][c] = in[N * r + c];
    for (int r = 0; r < N; ++r) b[r] = in[N * N + r];
    Ldlt<N> f;
    ldlt_factor<N>(A, f);
    ldlt_solve<N>(f, b, x);
    out.insert(out.end(), x, x + N);
    out.insert(out.end(), f.D, f.D + N);
    out.push_back(f.det);
    out.push_back(ldlt_ok(f) ? 1.0 : 0.0);
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: rigid_solve_tool ldlt6|ldlt3|rodrigues|compose|inverse in.bin out.bin\n");
        return 2;
    }
    const std::string mode = argv[1];
    const int rec = mode == "ldlt6" ? 42 : mode == "ldlt3" ? 12 : mode == "rodrigues" ? 3 : mode == "compose" ? 28 : mode == "inverse" ? 16 : 0;
    FILE* fi = std::fopen(argv[2], "rb");
    int count = 0;
    if (!rec || !fi || std::fread(&count, 4, 1, fi) != 1 || count < 0) return 2;
    std::vector<double> in((size_t) count * rec);
    if (std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
    std::fclose(fi);
    std::vector<double> od;
    std::vector<float> of;
    for (int i = 0; i < count; ++i) {
        const double* p = in.data() + (size_t) i * rec;
        if (mode == "ldlt6") {
            ldlt_record<6>(p, od);
        } else if (mode == "ldlt3") {
            ldlt_record<3>(p, od);
        } else if (mode == "rodrigues") {
            const double w[3] = {p[0], p[1], p[2]};
            double R[9];
            const double th = rodrigues(w, R);
            od.insert(od.end(), R, R + 9);
            od.push_back(th);
        } else if (mode == "compose") {
            double R[9], t[3];
            float P[12], pose[16];
            std::memcpy(R, p, sizeof R);
            std::memcpy(t, p + 9, sizeof t);
            for (int k = 0; k < 16; ++k) pose[k] = (float) p[12 + k];
            for (int k = 0; k < 12; ++k) P[k] = pose[k];
            pose_compose(R, t, P, pose);
            of.insert(of.end(), pose, pose + 16);
        } else {
            float P[16], out[16];
            for (int k = 0; k < 16; ++k) P[k] = (float) p[k];
            rigid_inverse(P, out);
            of.insert(of.end(), out, out + 16);
        }
    }
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    if (!od.empty()) std::fwrite(od.data(), sizeof(double), od.size(), fo);
    if (!of.empty()) std::fwrite(of.data(), sizeof(float), of.size(), fo);
    std::fclose(fo);
    return 0;
}
