// The canonical mesh carried to live through the C++ shells: runs SobFusion on the synthetic translating sphere (the headless app's
// --synthetic N: 5 mm in x per frame), then dumps what tests/test_gpu_mesh_warp.py compares with ops.warp_points / ops.sample_tsdf on the
// same volumes.  usage: mesh_warp_tool <params.ini> <frames> <out dir>
// Writes .npy files: psi (Z, Y, X, 4), phi_n (Z, Y, X, 2), canonical_vertices / canonical_normals (V, 4) (get_phi_global_indexed_mesh),
// warped_vertices / warped_normals (get_phi_global_warped_indexed_mesh: the device path), kept_vertices / kept_normals (warp_to_live of
// the canonical mesh: the upload path), faces (F, 3) as float, fit_samples (V,) (fit_to_live of the warped mesh) and prints
// "fit <vertices> <valid> <mean_abs> <rms> <max>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <sobfu_amd/depth_io.hpp>
#include <sobfu_amd/sobfu.hpp>

// uint16 mm depth of a sphere, the convention of apps/sobfu_headless.cpp and sobfu_amd/synthetic.py::render_sphere_depth
static void render_sphere(double cx, double cy, double cz, double r, const kfusion::Intr& in, int rows, int cols, std::vector<uint16_t>& out) {
    out.assign((size_t) rows * cols, 0);
    for (int v = 0; v < rows; ++v)
        for (int u = 0; u < cols; ++u) {
            double dx = (u - (double) in.cx) / (double) in.fx, dy = (v - (double) in.cy) / (double) in.fy;
            double a = dx * dx + dy * dy + 1.0, b = -2.0 * (dx * cx + dy * cy + cz), c = cx * cx + cy * cy + cz * cz - r * r;
            double disc = b * b - 4.0 * a * c;
            if (disc >= 0) out[(size_t) v * cols + u] = (uint16_t) std::nearbyint(1000.0 * (-b - std::sqrt(disc)) / (2.0 * a));
        }
}

static bool dump4(const std::string& path, const std::vector<float4>& v) {
    return sobfu_amd::write_npy(path, (const float*) v.data(), {v.size(), (size_t) 4});
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::printf("usage: %s params.ini frames outdir\n", argv[0]);
        return 2;
    }
    Params p;
    std::string why;
    if (!sobfu_amd::read_params_ini(argv[1], p, nullptr, &why)) {
        std::printf("bad parameter file: %s\n", why.c_str());
        return 2;
    }
    const int frames = std::atoi(argv[2]);
    const std::string out = argv[3];
    kfusion::cuda::setDevice(0);
    SobFusion fusion(p);
    std::vector<uint16_t> img;
    kfusion::cuda::Depth depth;
    for (int n = 0; n < frames; ++n) {
        render_sphere(0.005 * n, 0.0, 0.75, 0.1, p.intr, p.rows, p.cols, img);
        depth.upload(img.data(), (size_t) p.cols * sizeof(uint16_t), p.rows, p.cols);
        fusion(depth);
    }
    const sobfu_amd::IndexedMesh canonical = fusion.get_phi_global_indexed_mesh();
    const sobfu_amd::IndexedMesh warped = fusion.get_phi_global_warped_indexed_mesh();
    const sobfu_amd::IndexedMesh kept = fusion.warp_to_live(canonical);
    std::vector<float> samples;
    const sobfu_amd::MeshFit fit = fusion.fit_to_live(warped, &samples);

    const cv::Vec3i d = p.volume_dims;
    const size_t n = (size_t) d[0] * d[1] * d[2], Z = (size_t) d[2], Y = (size_t) d[1], X = (size_t) d[0];
    std::vector<float4> h(n);
    std::vector<float2> t(n);
    fusion.psi->get_data().download(h.data());
    fusion.phi_n->data().download(t.data());
    std::vector<float> faces(warped.faces.begin(), warped.faces.end());
    bool ok = sobfu_amd::write_npy(out + "/psi.npy", (const float*) h.data(), {Z, Y, X, 4}) &&
              sobfu_amd::write_npy(out + "/phi_n.npy", (const float*) t.data(), {Z, Y, X, 2}) && dump4(out + "/canonical_vertices.npy", canonical.vertices) &&
              dump4(out + "/canonical_normals.npy", canonical.normals) && dump4(out + "/warped_vertices.npy", warped.vertices) &&
              dump4(out + "/warped_normals.npy", warped.normals) && dump4(out + "/kept_vertices.npy", kept.vertices) &&
              dump4(out + "/kept_normals.npy", kept.normals) &&
              sobfu_amd::write_npy(out + "/faces.npy", faces.data(), {warped.triangles(), (size_t) 3}) &&
              sobfu_amd::write_npy(out + "/fit_samples.npy", samples.data(), {samples.size()});
    if (!ok || canonical.faces != warped.faces || canonical.faces != kept.faces) {
        std::printf("cannot write the dumps, or the faces changed\n");
        return 1;
    }
    std::printf("fit %zu %zu %.9g %.9g %.9g\n", fit.vertices, fit.valid, fit.mean_abs, fit.rms, fit.max);
    return 0;
}
