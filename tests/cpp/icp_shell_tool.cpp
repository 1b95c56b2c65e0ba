// Camera tracking through the reference's class surface (kfusion::cuda::ProjectiveICP, Frame and the imgproc helpers), written the way
// the reference's KinFu would call it: depth -> pyramid -> point / normal pyramids, then estimateTransform on the Frame and on the two
// pyramid overloads.  usage: icp_shell_tool <depth0.raw> <depth1.raw> rows cols fx fy cx cy  (raw little-endian uint16 mm)
// Prints "points ok R00 .. R22 t0 t1 t2" and "depth ok ..." lines: the pose mapping frame 1 into frame 0.
#include <cstdio>
#include <fstream>
#include <vector>

#include <kfusion/cuda/imgproc.hpp>
#include <kfusion/cuda/projective_icp.hpp>
#include <kfusion/types.hpp>

using namespace kfusion;

static bool load(const char* path, int rows, int cols, cuda::Depth& d) {
    std::vector<unsigned short> h((size_t) rows * cols);
    std::ifstream f(path, std::ios::binary);
    if (!f.read((char*) h.data(), (std::streamsize) (h.size() * 2))) return false;
    d.upload(h.data(), (size_t) cols * 2, rows, cols);
    return true;
}

static void print(const char* what, bool ok, const Affine3f& a) {
    std::printf("%s %d", what, ok ? 1 : 0);
    for (int i = 0; i < 9; ++i) std::printf(" %.9g", a.R[i]);
    for (int i = 0; i < 3; ++i) std::printf(" %.9g", a.t[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::printf("usage: %s depth0.raw depth1.raw rows cols fx fy cx cy\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
    Intr intr;
    intr.fx = std::atof(argv[5]), intr.fy = std::atof(argv[6]), intr.cx = std::atof(argv[7]), intr.cy = std::atof(argv[8]);
    cuda::ProjectiveICP icp;
    std::vector<int> iters = {10, 5, 4};
    icp.setIterationsNum(iters);
    icp.setDistThreshold(0.1f);
    icp.setAngleThreshold(20.f * 0.017453293f);
    const int LEVELS = icp.getUsedLevelsNum();

    cuda::Frame frames[2];
    for (int k = 0; k < 2; ++k) {
        cuda::Frame& f = frames[k];
        f.use_points = true;
        f.depth_pyr.resize(LEVELS), f.points_pyr.resize(LEVELS), f.normals_pyr.resize(LEVELS);
        if (!load(argv[1 + k], rows, cols, f.depth_pyr[0])) {
            std::printf("cannot read %s\n", argv[1 + k]);
            return 2;
        }
        for (int i = 1; i < LEVELS; ++i) cuda::depthBuildPyramid(f.depth_pyr[i - 1], f.depth_pyr[i], 0.04f);
        for (int i = 0; i < LEVELS; ++i) cuda::computePointNormals(intr(i), f.depth_pyr[i], f.points_pyr[i], f.normals_pyr[i]);
    }
    Affine3f aff;
    bool ok = icp.estimateTransform(aff, intr, frames[1], frames[0]);
    print("points", ok, aff);

    // the model side as KinFu predicts it: level 0 points / normals, resized into the coarser levels
    cuda::ProjectiveICP::PointsPyr vprev(LEVELS);
    cuda::ProjectiveICP::NormalsPyr nprev(LEVELS);
    vprev[0] = frames[0].points_pyr[0], nprev[0] = frames[0].normals_pyr[0];
    for (int i = 1; i < LEVELS; ++i) cuda::resizePointsNormals(vprev[i - 1], nprev[i - 1], vprev[i], nprev[i]);
    ok = icp.estimateTransform(aff, intr, frames[1].points_pyr, frames[1].normals_pyr, vprev, nprev);
    print("points_resized", ok, aff);

    // depth overload: masked depth + normals per level
    cuda::ProjectiveICP::DepthPyr dp[2];
    cuda::ProjectiveICP::NormalsPyr np[2];
    for (int k = 0; k < 2; ++k) {
        dp[k].resize(LEVELS), np[k].resize(LEVELS);
        for (int i = 0; i < LEVELS; ++i) {
            dp[k][i] = frames[k].depth_pyr[i];  // shares the block: the frames are not used again
            cuda::computeNormalsAndMaskDepth(intr(i), dp[k][i], np[k][i]);
        }
    }
    ok = icp.estimateTransform(aff, intr, dp[1], np[1], dp[0], np[0]);
    print("depth", ok, aff);
    cuda::Depth dr;
    cuda::Normals nr;
    cuda::resizeDepthNormals(dp[0][0], np[0][0], dr, nr);
    std::printf("resized %d %d\n", dr.rows(), dr.cols());
    return 0;
}
