// sobfu_headless -- headless counterpart of the reference app's frame loop (src/apps/demo.cpp:285-340) on the MI355X
// shells: reads a params .ini, feeds depth frames to SobFusion::operator(), prints per-frame volume statistics and can
// dump the fields.  No OpenCV / PCL / VTK: depth frames are 16-bit grayscale PNG (what the reference's datasets ship),
// binary 16-bit PGM or raw little-endian uint16 files of rows*cols pixels (sobfu_amd/depth_io.hpp), or a built-in
// synthetic translating sphere.  --dump DIR writes psi, psi_inv and the four TSDF volumes as .npy (float32); --mesh DIR
// writes marching-cubes meshes of the volumes per frame as legacy-ASCII .vtk polydata (the reference: demo.cpp:236-246); with
// --mesh-format ply they are indexed meshes instead -- shared vertices with TSDF normals, binary little-endian .ply.
// --screenshots DIR writes DIR/%06d.png per frame (the reference's --enable-viz, demo.cpp:380-505): raycast + shaded views of the
// canonical model phi_global (left) and of the canonical model warped to live, phi_global_psi_inv (right; black until a frame has been
// solved); --screenshots-detailed adds a second row -- phi_n, phi_global_psi_inv / phi_global, phi_n_psi (demo.cpp:445-456).  The
// views are drawn from the depth camera (the pose and intrinsics the frames are integrated with) with a headlight at its origin, not
// from the reference viewer's camera at z = max + 3 (demo.cpp:403,467): with the depth camera the live panel lines up with the input.
// Colour (opt-in): --data DIR reads a dataset laid out as the reference app expects (demo.cpp:177-197): sorted DIR/depth/*, DIR/color/*
// when present (8-bit PNG or binary PPM, registered to depth) and DIR/omask/* when present (a mask zeroes the depth where it is 0,
// demo.cpp:314-328); --synthetic N --textured gives the sphere a texture that moves with it.  With colour frames the canonical colour is
// fused through psi: --mesh writes per-vertex colours for phi_global and phi_global_psi_inv, the phi_global / phi_global_psi_inv
// screenshot panels are coloured (the live panels of --screenshots-detailed stay grey) and --dump adds colour_global.npy (Z, Y, X, 4)
// uint8 (b, g, r, weight).  Without colour frames every output is the geometry-only one.
// Camera tracking (opt-in): --track (or TRACK_CAMERA=1 in the .ini) estimates each frame's camera pose with projective ICP against the
// model raycast at the previous pose before the non-rigid solve, and integrates the frame at that pose; the screenshots are then drawn
// from the current tracked pose.  --poses FILE writes one TUM-format line per frame, "frame tx ty tz qx qy qz qw" (identity without
// tracking).
// The canonical mesh carried to live (opt-in; sobfu_amd/csrc/warp_points_kernels.hip): --warp-mesh (with --mesh DIR) writes, on every solved
// frame n, DIR/phi_global_warped_<n>.ply -- the indexed mesh of phi_global with its vertices and normals pushed through psi and the canonical
// colours of its vertices.  --track-mesh K (with --mesh DIR) extracts that indexed mesh once, after frame K, and on every solved frame n >= K
// writes DIR/tracked_<n>.ply: the kept mesh carried to frame n by that frame's psi, so vertex i and the faces are the same in every file.
// --fit-stats prints one line per solved frame: phi_n sampled at the canonical mesh's vertices warped to live (and unwarped), in millimetres.
//
// Reconstruction error against ground-truth meshes (opt-in; sobfu_amd/csrc/mesh_distance_kernels.hip): exact vertex-to-surface
// distances both ways, a = the model, b = the ground truth, one printed line per evaluation with every field of compare_meshes at %.9g, in
// metres.  --evaluate GT.ply: after the last frame, the indexed mesh of phi_global against GT ("evaluate canonical <frame>: ...").
// --evaluate-live PATTERN (printf-style, one %d or %0Nd: the frame number): on every solved frame, phi_global's mesh carried through psi
// against that frame's ground truth ("evaluate live <frame>: ...").  The ground truth is in the frame of the meshes written here (x, -y, -z);
// --evaluate-pose FILE (16 numbers, row-major 4 x 4) is applied to it first.  --evaluate-max-dist METRES (default 5 x the truncation distance):
// vertices farther than that have no match.  --error-mesh DIR writes the evaluated mesh as DIR/error_canonical_<frame>.ply /
// DIR/error_live_<frame>.ply with vertices coloured by error: blue (0) to red (max-dist), grey where there is no match.
// --evaluate-align [ITERS] (default 30) refines the pose of --evaluate-pose (or the identity) before each canonical --evaluate, by
// point-to-plane ICP of the model's vertices against the ground truth (a start within ICP's basin is the caller's to give),
// and prints "align: status=... iterations=... inliers=... rms=... pose=<16 numbers at %.9g>"; --evaluate-align-dof 3|6 (default 6; 3:
// translation only, for symmetric objects); --evaluate-pose-out FILE writes the refined pose as --evaluate-pose reads it.  --evaluate-live
// uses the pose as given: aligning every live frame would hide the tracking error that evaluation measures.
//
// Depth frames from ground-truth meshes (opt-in; sobfu_amd/csrc/mesh_ray_kernels.hip): --render-mesh PATTERN is a fourth
// frame source beside --synthetic, --data and depth files, and excludes them.  PATTERN is printf-style like --evaluate-live's: frames 0, 1, ...
// while the file exists; without a conversion it names one static mesh, rendered for --render-frames N frames (default 1).  The meshes are
// in the frame --evaluate reads them in (x, -y, -z); --render-pose FILE (16 numbers, as --evaluate-pose) is applied first.  Each is ray cast
// on the GPU from the depth camera of the .ini into uint16 millimetres, which then goes the way a depth file's pixels go.  When the .ply
// has vertex colours and --textured is given, colour frames are rendered too.  --render-mesh and --evaluate-live given the same pattern
// and pose share one triangle grid per ground-truth frame: built once, used to render the frame and to score it.
//
// Volumes from ground-truth meshes (opt-in; sobfu_amd/csrc/mesh_voxel_kernels.hip): --voxelise-mesh PATTERN is a fifth frame
// source that takes --render-mesh's place and its --render-frames / --render-pose: every closed mesh reaches the solver as a full signed
// TSDF (SobFusion::integrate_mesh), without a depth camera in between; a mesh that is not closed ends the run.  It shares the mesh and the
// scoring grid with --evaluate-live as --render-mesh does (the voxelisation builds a grid of its own over the vertices in the volume's
// frame).  --evaluate-signed adds signed_mean, inside and open to each side of the evaluate lines: the sign of a vertex against the
// other mesh, > 0 outside.  --mesh-sign parity|winding chooses the inside / outside rule of both: parity (the default) is for
// closed meshes; winding takes the generalised winding number, is defined for open meshes too, and refuses none for being open.
//
// A depth sensor and a moving camera for --render-mesh (opt-in; sobfu_amd/csrc/depth_sensor_kernels.hip): --sensor kinect|ideal
// passes every rendered frame -- its points and normals -- through the depth sensor model before it goes the way a depth file's pixels go:
// lateral jitter, axial noise, disparity quantisation, dropouts and a range gate, drawn from --sensor-seed N (default 0) and the frame
// number, so a run repeats bit for bit.  --sensor-set name=value (repeatable, after --sensor; the names of sobfu_hip_sensor_params:
// lateral, z_min, z_max, cos_min, edge_radius, edge_jump, edge_drop, drop, a0, a1, z0, a2, disparity) overrides one field.  --sensor ideal
// changes nothing.  --render-trajectory FILE reads camera poses in the format --poses writes (camera -> frame 0's camera): frame n is
// rendered from pose n of the file, that is with inverse(pose_n) applied to the mesh after --render-pose and the (x, -y, -z) flip; fewer
// poses than frames is an error, and --voxelise-mesh, which has no camera, excludes it.  With --track as well, one line after the last
// frame scores the tracked poses against the file: "trajectory: ate=... rpe_trans=... rpe_rot=..." (sobfu_amd/trajectory.hpp: metres,
// metres, radians; steps of one frame).
//
// Precision, recall and F-score (opt-in; sobfu_amd/csrc/mesh_sample_kernels.hip): --evaluate-fscore TAU[,TAU...] (metres,
// up to 16, each > 0; needs --evaluate or --evaluate-live) samples both meshes of every evaluation uniformly per unit area and prints, after
// each "evaluate canonical|live <frame>: ..." line, "fscore canonical|live <frame>: a_samples=... b_samples=... tau=... precision=... recall=...
// f=... [tau=... ...] a_to_b.n=... ... chamfer=... hausdorff=..." from the same (aligned, posed) meshes: precision is the share of the model's
// samples within tau of the ground truth, recall the share of the ground truth's within tau of the model, the statistics those of
// compare_meshes over the samples, so weighted by area.  --evaluate-samples N (default 200 000: the density is N over the larger of the two
// areas) or --evaluate-density D (samples per square metre), not both; --evaluate-seed S (default 0) picks the draws.  A sample farther
// than --evaluate-max-dist is a miss.  The evaluate lines are the same with and without.
//
// Diagnostics of the deformation (opt-in; sobfu_amd/csrc/warp_stats_kernels.hip): --warp-stats [BAND] prints, after each solved
// frame, "warp <frame>: voxels=... det min=... @x,y,z max=... mean=... folds=... (...%) disp max=... mean=... inv res max=... @x,y,z mean=...
// above=... outside=...": det J of psi (1 = volume preserving, <= 0 = folded) and the displacement |psi - id| in metres over the voxels of
// phi_global within BAND (default 1, units of the truncation distance) of the surface, and the residual |psi(psi_inv(x)) - x| in metres over
// those of phi_global o psi_inv: its maximum, its mean, how many exceed a tenth of the smallest voxel side and how many psi_inv(x) leave the
// volume.  Floats are printed as %.9g: they round-trip.  --warp-stats-dump DIR (implies --warp-stats) also writes the per-voxel volumes
// detJ_<frame>.npy and invres_<frame>.npy (Z, Y, X float32; every voxel, masked or not; NaN where psi_inv(x) is outside or non-finite).
//
//   sobfu_headless <params.ini> [--max-iter N] [--verbose|--vverbose] [--dims N] [--dump DIR] [--mesh DIR [--mesh-format vtk|ply]] [--no-stats]
//                  [--screenshots DIR [--screenshots-detailed]] [--track] [--poses FILE]
//                  [--warp-mesh] [--track-mesh K] [--fit-stats] [--warp-stats [BAND]] [--warp-stats-dump DIR]
//                  (--synthetic FRAMES [--shift DX] [--textured] | --data DIR | --render-mesh PATTERN [--render-frames N] [--render-pose FILE]
//                   [--textured] [--sensor kinect|ideal [--sensor-seed N] [--sensor-set name=value]...] [--render-trajectory FILE]
//                   | --voxelise-mesh PATTERN [--render-frames N] [--render-pose FILE] | frame0.pgm frame1.pgm ...)
//                  [--evaluate GT.ply] [--evaluate-live PATTERN] [--evaluate-signed] [--mesh-sign parity|winding]
//                  [--evaluate-fscore TAU[,TAU...] [--evaluate-samples N | --evaluate-density D] [--evaluate-seed S]]
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <sobfu_amd/depth_io.hpp>
#include <sobfu_amd/sobfu.hpp>
#include <sobfu_amd/trajectory.hpp>

// uint16 mm depth of a sphere, same convention as sobfu_amd/synthetic.py::render_sphere_depth (float64, rint)
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

// BGRA colour frame of the same sphere: a pixel that hits it takes a fixed function of the direction n from the centre to the hit point
// (the texture moves with the sphere); a miss is black.  Same convention as sobfu_amd/synthetic.py::render_textured_sphere_colour.
static void render_sphere_colour(double cx, double cy, double cz, double r, const kfusion::Intr& in, int rows, int cols, std::vector<uint8_t>& out) {
    out.assign((size_t) rows * cols * 4, 0);
    for (int v = 0; v < rows; ++v)
        for (int u = 0; u < cols; ++u) {
            double dx = (u - (double) in.cx) / (double) in.fx, dy = (v - (double) in.cy) / (double) in.fy;
            double a = dx * dx + dy * dy + 1.0, b = -2.0 * (dx * cx + dy * cy + cz), c = cx * cx + cy * cy + cz * cz - r * r;
            double disc = b * b - 4.0 * a * c;
            if (disc < 0) continue;
            const double z = (-b - std::sqrt(disc)) / (2.0 * a);
            const double nx = (z * dx - cx) / r, ny = (z * dy - cy) / r;
            uint8_t* o = &out[((size_t) v * cols + u) * 4];
            o[2] = (uint8_t) std::nearbyint(127.5 * (1.0 + nx));
            o[1] = (uint8_t) std::nearbyint(127.5 * (1.0 + ny));
            o[0] = (uint8_t) std::nearbyint(127.5 * (1.0 + std::sin(12.0 * nx) * std::cos(12.0 * ny)));
            o[3] = 255;
        }
}

// sorted regular files of a directory; false when it does not exist
static bool list_dir(const std::string& dir, std::vector<std::string>& out) {
    DIR* d = opendir(dir.c_str());
    if (!d) return false;
    while (dirent* e = readdir(d)) {
        const std::string path = dir + "/" + e->d_name;
        struct stat st;
        if (e->d_name[0] != '.' && stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode)) out.push_back(path);
    }
    closedir(d);
    std::sort(out.begin(), out.end());
    return true;
}

static void stats(const char* name, kfusion::cuda::TsdfVolume& v) {
    cv::Vec3i d = v.getDims();
    std::vector<float2> h((size_t) d[0] * d[1] * d[2]);
    v.data().download(h.data());
    double st = 0, sw = 0;
    long nt = 0;
    for (auto& e : h) { st += e.x; sw += e.y; nt += (std::fabs(e.x) < 1.f && e.y > 0.f); }
    std::printf("%s: sum_tsdf=%.4f sum_weight=%.0f non_truncated_observed=%ld\n", name, st, sw, nt);
}

// Screenshot compositor: one device image of 2 x 1 (or 2 x 2) panels of rows x cols, each view raycast into the same point / normal
// buffers and shaded straight into its panel (pitched output); every buffer is allocated once, on the first frame.
struct Screenshots {
    std::string dir;
    bool detailed = false;
    int rows = 0, cols = 0;
    kfusion::cuda::Cloud points;
    kfusion::cuda::Normals normals;
    kfusion::cuda::Image colours;  // sampled colour of a coloured panel
    kfusion::cuda::Image image;  // (2 or 1 panel rows) x 2 panels
    std::vector<kfusion::RGB> bgra;
    std::vector<uint8_t> rgb;

    void create(int rows_, int cols_) {
        rows = rows_, cols = cols_;
        points.create(rows, cols);
        normals.create(rows, cols);
        image.create((detailed ? 2 : 1) * rows, 2 * cols);
        bgra.resize((size_t) image.rows() * image.cols());
        rgb.resize(bgra.size() * 3);
    }
    // shades `v` (or leaves the panel black when v is null) into panel (pr, pc), in colour when `colour` is given
    void panel(kfusion::cuda::TsdfVolume* v, const cv::Affine3f& pose, const kfusion::Intr& intr, int pr, int pc,
               const kfusion::cuda::ColourVolume* colour = nullptr) {
        if (!v) return;
        v->raycast(pose, intr, points, normals);  // the depth camera (SobFusion's camera_pose_: identity unless tracking)
        uint8_t* dst = (uint8_t*) image.ptr() + (size_t) pr * rows * image.step() + (size_t) pc * cols * sizeof(kfusion::RGB);
        if (colour) {
            colour->sample(points, normals, pose.inv() * v->getPose(), v->getVoxelSize(), colours);
            sobfuSafeCall(sobfu_hip_render_colour((const float*) points.ptr(), (int) points.step(), (const float*) normals.ptr(), (int) normals.step(),
                                                  (const uint8_t*) colours.ptr(), (int) colours.step(), rows, cols, 0.f, 0.f, 0.f, dst,
                                                  (int) image.step(), nullptr));
            return;
        }
        sobfuSafeCall(sobfu_hip_render_image((const float*) points.ptr(), (int) points.step(), (const float*) normals.ptr(), (int) normals.step(),
                                             rows, cols, 0.f, 0.f, 0.f, dst, (int) image.step(), nullptr));  // headlight at the camera
    }
    bool write(int frame, SobFusion& fusion, bool solved, const kfusion::Intr& intr) {
        if (points.empty()) create(fusion.getParams().rows, fusion.getParams().cols);
        sobfuSafeCall(hipMemset2D(image.ptr(), image.step(), 0, (size_t) image.cols() * sizeof(kfusion::RGB), image.rows()));
        const cv::Affine3f pose = fusion.getCameraPose();
        panel(fusion.phi_global.get(), pose, intr, detailed ? 1 : 0, 0, fusion.colour_global.get());
        panel(solved ? fusion.phi_global_psi_inv.get() : nullptr, pose, intr, 0, 1, solved ? fusion.get_colour_global_psi_inv().get() : nullptr);
        if (detailed) {
            panel(frame > 0 ? fusion.phi_n.get() : nullptr, pose, intr, 0, 0);
            panel(solved ? fusion.phi_n_psi.get() : nullptr, pose, intr, 1, 1);
        }
        image.download(bgra.data(), (size_t) image.cols() * sizeof(kfusion::RGB));
        for (size_t i = 0; i < bgra.size(); ++i) {
            rgb[3 * i] = bgra[i].r;
            rgb[3 * i + 1] = bgra[i].g;
            rgb[3 * i + 2] = bgra[i].b;
        }
        char name[32];
        std::snprintf(name, sizeof name, "/%06d.png", frame);  // demo.cpp:409-414
        return sobfu_amd::write_png_rgb(dir + name, image.rows(), image.cols(), rgb.data());
    }
};

// PATTERN of --evaluate-live with the frame number in place of its one %d / %0Nd; empty: not such a pattern
static std::string frame_path(const std::string& pattern, int n) {
    const size_t at = pattern.find('%');
    if (at == std::string::npos || pattern.find('%', at + 1) != std::string::npos) return "";
    size_t e = at + 1;
    while (e < pattern.size() && pattern[e] >= '0' && pattern[e] <= '9') ++e;
    if (e >= pattern.size() || pattern[e] != 'd' || e - at > 4) return "";
    std::string digits = std::to_string(n);
    const int width = e > at + 1 ? std::atoi(pattern.substr(at + 1, e - at - 1).c_str()) : 0;
    if (pattern[at + 1] == '0' || width > 0)
        while ((int) digits.size() < width) digits.insert(digits.begin(), pattern[at + 1] == '0' ? '0' : ' ');
    return pattern.substr(0, at) + digits + pattern.substr(e + 1);
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::printf("usage: %s <params.ini> [--max-iter N] [--verbose|--vverbose] [--dims N] [--dump DIR] [--mesh DIR [--mesh-format vtk|ply]] [--no-stats] "
                    "[--screenshots DIR [--screenshots-detailed]] [--track] [--poses FILE] [--warp-mesh] [--track-mesh K] [--fit-stats] [--warp-stats [BAND]] [--warp-stats-dump DIR] [--evaluate GT.ply] [--evaluate-live PATTERN] [--evaluate-max-dist METRES] [--evaluate-pose FILE] [--evaluate-align [ITERS]] [--evaluate-align-dof 3|6] [--evaluate-pose-out FILE] [--evaluate-signed] [--evaluate-fscore TAU[,TAU...] [--evaluate-samples N | --evaluate-density D] [--evaluate-seed S]] [--error-mesh DIR] (--synthetic FRAMES [--shift DX] [--textured] | --data DIR | --render-mesh PATTERN [--render-frames N] [--render-pose FILE] [--textured] [--sensor kinect|ideal [--sensor-seed N] [--sensor-set name=value]...] [--render-trajectory FILE] | --voxelise-mesh PATTERN [--render-frames N] [--render-pose FILE] | depth files...)\n",
                    argv[0]);
        return 2;
    }
    Params p;
    std::string why;
    if (!sobfu_amd::read_params_ini(argv[1], p, nullptr, &why)) {
        std::printf("bad parameter file: %s\n", why.c_str());
        return 2;
    }
    int synthetic = 0;
    double shift = 0.005;
    bool textured = false, warp_mesh = false, fit_stats = false;
    int track_mesh = -1;  // the frame after which the tracked mesh is cut; -1: off
    bool warp_stats = false;  // --warp-stats: a "warp" line after each solved frame
    float warp_stats_band = 1.f;
    std::string warp_stats_dump;  // --warp-stats-dump: detJ_<n>.npy and invres_<n>.npy as well
    std::string dump, mesh_dir, data_dir, mesh_format = "vtk", poses_path;
    std::string eval_gt, eval_live, eval_pose, error_dir, eval_pose_out;
    std::string render_mesh, render_pose;  // --render-mesh: the frame source; --render-pose: applied to its meshes first
    bool voxelise = false, eval_signed = false;  // --voxelise-mesh: the meshes reach the solver as volumes, not as depth frames
    int mesh_sign = sobfu_amd::kSignParity;      // --mesh-sign: the inside / outside rule of --voxelise-mesh and --evaluate-signed
    int render_frames = 1;
    bool sensor = false;  // --sensor: rendered frames pass through sensor_model
    sobfu_amd::SensorModel sensor_model;
    uint64_t sensor_seed = 0;
    std::string render_trajectory;  // --render-trajectory: frame n is rendered from pose n of this file
    int eval_align = -1, eval_align_dof = 6;  // --evaluate-align: the iterations; -1: off
    float eval_max_dist = -1.f;  // < 0: 5 x the truncation distance
    sobfu_amd::ScoreRequest score;  // --evaluate-fscore: its thresholds; empty: off
    bool score_given = false, score_samples = false, score_density = false, score_seed = false;
    Screenshots shots;
    bool print_stats = true;  // per-frame volume statistics download four volumes: --no-stats leaves only the frame loop (timing runs)
    std::vector<std::string> files;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--max-iter" && i + 1 < argc) p.max_iter = std::atoi(argv[++i]);
        else if (a == "--verbose") p.verbosity = 1;
        else if (a == "--vverbose") p.verbosity = 2;
        else if (a == "--dims" && i + 1 < argc) { int n = std::atoi(argv[++i]); p.volume_dims = cv::Vec3i::all(n); }
        else if (a == "--synthetic" && i + 1 < argc) synthetic = std::atoi(argv[++i]);
        else if (a == "--shift" && i + 1 < argc) shift = std::atof(argv[++i]);
        else if (a == "--textured") textured = true;
        else if (a == "--data" && i + 1 < argc) data_dir = argv[++i];
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--mesh" && i + 1 < argc) mesh_dir = argv[++i];
        else if (a == "--mesh-format" && i + 1 < argc) mesh_format = argv[++i];
        else if (a == "--no-stats") print_stats = false;
        else if (a == "--screenshots" && i + 1 < argc) shots.dir = argv[++i];
        else if (a == "--screenshots-detailed") shots.detailed = true;
        else if (a == "--track") p.track_camera = true;
        else if (a == "--poses" && i + 1 < argc) poses_path = argv[++i];
        else if (a == "--warp-mesh") warp_mesh = true;
        else if (a == "--track-mesh" && i + 1 < argc) track_mesh = std::atoi(argv[++i]);
        else if (a == "--fit-stats") fit_stats = true;
        else if (a == "--warp-stats") {
            warp_stats = true;
            char* end = nullptr;  // an optional BAND: the next argument when all of it is a number
            const float band = i + 1 < argc ? std::strtof(argv[i + 1], &end) : 0.f;
            if (i + 1 < argc && end != argv[i + 1] && *end == '\0') {
                if (!std::isfinite(band) || !(band > 0.f)) {
                    std::printf("--warp-stats %s: expected a band > 0 (units of the truncation distance)\n", argv[i + 1]);
                    return 2;
                }
                warp_stats_band = band, ++i;
            }
        }
        else if (a == "--warp-stats-dump" && i + 1 < argc) warp_stats = true, warp_stats_dump = argv[++i];
        else if (a == "--evaluate" && i + 1 < argc) eval_gt = argv[++i];
        else if (a == "--evaluate-live" && i + 1 < argc) eval_live = argv[++i];
        else if (a == "--evaluate-max-dist" && i + 1 < argc) eval_max_dist = std::strtof(argv[++i], nullptr);
        else if (a == "--evaluate-pose" && i + 1 < argc) eval_pose = argv[++i];
        else if (a == "--evaluate-align") {
            eval_align = 30;
            if (i + 1 < argc && argv[i + 1][0] != '\0' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos)
                eval_align = std::atoi(argv[++i]);
        }
        else if (a == "--evaluate-align-dof" && i + 1 < argc) eval_align_dof = std::atoi(argv[++i]);
        else if (a == "--evaluate-pose-out" && i + 1 < argc) eval_pose_out = argv[++i];
        else if (a == "--error-mesh" && i + 1 < argc) error_dir = argv[++i];
        else if (a == "--evaluate-fscore" && i + 1 < argc) {
            const std::string list = argv[++i];
            score_given = true;
            for (size_t at = 0; at <= list.size();) {  // TAU[,TAU...]: every entry a finite number > 0
                const size_t comma = std::min(list.find(',', at), list.size());
                const std::string item = list.substr(at, comma - at);
                char* end = nullptr;
                const float tau = std::strtof(item.c_str(), &end);
                if (item.empty() || end != item.c_str() + item.size() || !std::isfinite(tau) || !(tau > 0.f) || score.thresholds.size() == 16) {
                    std::printf("--evaluate-fscore %s: expected 1 to 16 comma-separated distances in metres, each > 0\n", list.c_str());
                    return 2;
                }
                score.thresholds.push_back(tau);
                at = comma + 1;
            }
        }
        else if (a == "--evaluate-samples" && i + 1 < argc) {
            char* end = nullptr;
            score.samples = std::strtoll(argv[++i], &end, 10);
            score_samples = true;
            if (end == argv[i] || *end != '\0' || score.samples < 1) {
                std::printf("--evaluate-samples %s: expected a count >= 1\n", argv[i]);
                return 2;
            }
        }
        else if (a == "--evaluate-density" && i + 1 < argc) {
            char* end = nullptr;
            score.density = std::strtod(argv[++i], &end);
            score_density = true;
            if (end == argv[i] || *end != '\0' || !std::isfinite(score.density) || !(score.density > 0.0)) {
                std::printf("--evaluate-density %s: expected samples per square metre, finite and > 0\n", argv[i]);
                return 2;
            }
        }
        else if (a == "--evaluate-seed" && i + 1 < argc) {
            char* end = nullptr;
            score.seed = std::strtoull(argv[++i], &end, 0);
            score_seed = true;
            if (end == argv[i] || *end != '\0') {
                std::printf("--evaluate-seed %s: expected an unsigned integer\n", argv[i]);
                return 2;
            }
        }
        else if (a == "--render-mesh" && i + 1 < argc) {
            if (voxelise) {
                std::printf("--voxelise-mesh and --render-mesh exclude each other\n");
                return 2;
            }
            render_mesh = argv[++i];
        }
        else if (a == "--voxelise-mesh" && i + 1 < argc) {
            if (!render_mesh.empty()) {
                std::printf("--voxelise-mesh and --render-mesh exclude each other\n");
                return 2;
            }
            render_mesh = argv[++i], voxelise = true;
        }
        else if (a == "--evaluate-signed") eval_signed = true;
        else if (a == "--mesh-sign" && i + 1 < argc) {
            const std::string rule = argv[++i];
            if (rule != "parity" && rule != "winding") {
                std::printf("--mesh-sign takes parity or winding\n");
                return 2;
            }
            mesh_sign = rule == "winding" ? sobfu_amd::kSignWinding : sobfu_amd::kSignParity;
        }
        else if (a == "--render-frames" && i + 1 < argc) render_frames = std::atoi(argv[++i]);
        else if (a == "--render-pose" && i + 1 < argc) render_pose = argv[++i];
        else if (a == "--sensor" && i + 1 < argc) {
            const std::string name = argv[++i];
            if (name != "kinect" && name != "ideal") {
                std::printf("--sensor is kinect or ideal, not %s\n", name.c_str());
                return 2;
            }
            sensor = true, sensor_model = name == "kinect" ? sobfu_amd::SensorModel::kinect() : sobfu_amd::SensorModel::ideal();
        }
        else if (a == "--sensor-seed" && i + 1 < argc) sensor_seed = std::strtoull(argv[++i], nullptr, 0);
        else if (a == "--sensor-set" && i + 1 < argc) {
            const std::string kv = argv[++i];
            const size_t eq = kv.find('=');
            char* end = nullptr;
            const double value = eq == std::string::npos ? 0.0 : std::strtod(kv.c_str() + eq + 1, &end);
            if (!sensor || eq == std::string::npos || end == kv.c_str() + eq + 1 || *end != '\0' || !sensor_model.set(kv.substr(0, eq), value)) {
                std::printf("--sensor-set %s: expected name=value after --sensor, name a field of sobfu_hip_sensor_params\n", kv.c_str());
                return 2;
            }
        }
        else if (a == "--render-trajectory" && i + 1 < argc) render_trajectory = argv[++i];
        else files.push_back(a);
    }
    if (mesh_format != "vtk" && mesh_format != "ply") {
        std::printf("--mesh-format is vtk or ply, not %s\n", mesh_format.c_str());
        return 2;
    }
    if (eval_align_dof != 3 && eval_align_dof != 6) {
        std::printf("--evaluate-align-dof is 3 or 6, not %d\n", eval_align_dof);
        return 2;
    }
    if (eval_align > 1000 || (eval_align >= 0 && eval_gt.empty()) || (!eval_pose_out.empty() && eval_align < 0)) {
        std::printf("--evaluate-align takes at most 1000 iterations and needs --evaluate GT.ply; --evaluate-pose-out needs --evaluate-align\n");
        return 2;
    }
    if (score_samples && score_density) {
        std::printf("--evaluate-samples and --evaluate-density exclude each other\n");
        return 2;
    }
    if (!score_given && (score_samples || score_density || score_seed)) {
        std::printf("--evaluate-samples, --evaluate-density and --evaluate-seed need --evaluate-fscore\n");
        return 2;
    }
    if (score_given && eval_gt.empty() && eval_live.empty()) {
        std::printf("--evaluate-fscore needs --evaluate GT.ply or --evaluate-live PATTERN\n");
        return 2;
    }
    if ((warp_mesh || track_mesh >= 0) && mesh_dir.empty()) {
        std::printf("--warp-mesh and --track-mesh need --mesh DIR\n");
        return 2;
    }
    if (argc > 2) {  // --dims changes the voxel size: re-derive the voxel-unit parameters
        std::map<std::string, std::string> kv;
        Params q = p;
        sobfu_amd::read_params_ini(argv[1], q, &kv);
        float tv = std::strtof(kv["TSDF_TRUNC_DIST"].c_str(), nullptr), ev = std::strtof(kv["ETA"].c_str(), nullptr);
        p.tsdf_trunc_dist = tv * p.voxel_sizes()[0];
        p.eta = ev * p.voxel_sizes()[0];
    }
    // ground truth of --evaluate / --evaluate-live: read, posed, compared; one printed line, one optional error mesh
    float gt_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, mesh_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    auto read_pose = [](const char* option, const std::string& path, float pose[16]) {
        if (path.empty()) return true;
        FILE* f = std::fopen(path.c_str(), "r");
        int got = 0;
        while (f && got < 16 && std::fscanf(f, "%f", &pose[got]) == 1) ++got;
        if (f) std::fclose(f);
        if (got != 16) std::printf("%s %s: expected 16 numbers\n", option, path.c_str());
        return got == 16;
    };
    if (!read_pose("--evaluate-pose", eval_pose, gt_pose) || !read_pose("--render-pose", render_pose, mesh_pose)) return 2;
    // the ground-truth frame of --render-mesh being rendered: its mesh (posed) and the grid over it, which --evaluate-live shares
    struct {
        std::string path;
        sobfu_amd::IndexedMesh mesh;
        sobfu_amd::TriangleGrid grid;
    } rendered;
    if (!eval_live.empty() && frame_path(eval_live, 0).empty()) {
        std::printf("--evaluate-live needs a pattern with one %%d or %%0Nd, not %s\n", eval_live.c_str());
        return 2;
    }
    if (eval_max_dist < 0.f) eval_max_dist = 5.f * p.tsdf_trunc_dist;
    auto evaluate = [&](SobFusion& fusion, const std::string& gt_path, bool live, int n) {
        sobfu_amd::IndexedMesh read, model;
        std::string why;
        const bool shared = live && gt_path == rendered.path && eval_pose == render_pose;  // the frame just rendered: its mesh and grid
        if (!shared && !sobfu_amd::read_ply(gt_path, read, &why)) {
            std::printf("cannot read ground truth: %s\n", why.c_str());
            return false;
        }
        sobfu_amd::IndexedMesh& gt = shared ? rendered.mesh : read;
        const bool align = !live && eval_align >= 0;  // the live evaluation uses the pose as given
        if (!eval_pose.empty() && !align && !shared) sobfu_amd::transform_points(gt.vertices, gt_pose);
        sobfu_amd::MeshComparison r;
        std::vector<float> d;
        sobfu_amd::AlignRequest request;
        std::copy(gt_pose, gt_pose + 16, request.pose);
        request.iters = eval_align, request.dof = eval_align_dof;
        sobfu_amd::MeshScore scored;
        const sobfu_amd::ScoreRequest* scoring = score_given ? &score : nullptr;
        if (!(live ? fusion.evaluate_live(gt, eval_max_dist, r, &model, &d, &why, shared ? &rendered.grid : nullptr, eval_signed, mesh_sign, scoring, &scored)
                   : fusion.evaluate_canonical(gt, eval_max_dist, r, &model, &d, &why, align ? &request : nullptr, eval_signed, mesh_sign, scoring, &scored))) {
            std::printf("cannot evaluate against %s: %s\n", gt_path.c_str(), why.c_str());
            return false;
        }
        if (align) {
            std::printf("align: %s\n", sobfu_amd::format_alignment(request.info, request.pose).c_str());
            if (!eval_pose_out.empty()) {
                FILE* f = std::fopen(eval_pose_out.c_str(), "w");
                if (!f) {
                    std::printf("cannot write %s\n", eval_pose_out.c_str());
                    return false;
                }
                for (int k = 0; k < 16; ++k) std::fprintf(f, k % 4 == 3 ? "%.9g\n" : "%.9g ", (double) request.pose[k]);
                std::fclose(f);
            }
        }
        std::printf("evaluate %s %d: %s\n", live ? "live" : "canonical", n, sobfu_amd::format_comparison(r).c_str());
        if (scoring) std::printf("fscore %s %d: %s\n", live ? "live" : "canonical", n, sobfu_amd::format_f_score(scored).c_str());
        if (!error_dir.empty() && !model.empty()) {
            sobfu_amd::error_colours(d, eval_max_dist, model.colours);
            const std::string path = error_dir + (live ? "/error_live_" : "/error_canonical_") + std::to_string(n) + ".ply";
            if (!sobfu_amd::write_ply(path, model)) std::printf("cannot write %s\n", path.c_str());
        }
        return true;
    };
    std::vector<std::string> colour_files, mask_files;
    if (!data_dir.empty()) {  // demo.cpp:177-197, with a colour-less dataset allowed
        if (!files.empty() || synthetic > 0) {
            std::printf("--data excludes --synthetic and depth files\n");
            return 2;
        }
        if (!list_dir(data_dir + "/depth", files) || files.empty()) {
            std::printf("no depth frames in %s/depth\n", data_dir.c_str());
            return 2;
        }
        if (list_dir(data_dir + "/color", colour_files) && colour_files.size() != files.size()) {
            std::printf("%s: %zu depth frames but %zu colour frames\n", data_dir.c_str(), files.size(), colour_files.size());
            return 2;
        }
        if (list_dir(data_dir + "/omask", mask_files) && mask_files.size() != files.size()) {
            std::printf("%s: %zu depth frames but %zu masks\n", data_dir.c_str(), files.size(), mask_files.size());
            return 2;
        }
    }
    if (!render_mesh.empty() && (synthetic > 0 || !data_dir.empty() || !files.empty())) {
        std::printf("%s excludes --synthetic, --data and depth files\n", voxelise ? "--voxelise-mesh" : "--render-mesh");
        return 2;
    }
    if (textured && ((synthetic <= 0 && render_mesh.empty()) || voxelise)) {
        std::printf("--textured needs --synthetic or --render-mesh\n");
        return 2;
    }
    if (voxelise && (!shots.dir.empty() || p.track_camera)) {
        std::printf("--voxelise-mesh has no depth camera: it excludes --screenshots and --track\n");
        return 2;
    }
    if ((sensor || !render_trajectory.empty()) && (render_mesh.empty() || voxelise)) {
        std::printf("--sensor and --render-trajectory need --render-mesh (--voxelise-mesh has no depth camera)\n");
        return 2;
    }
    const bool mesh_sequence = !frame_path(render_mesh, 0).empty();
    int mesh_frames = 0;
    if (!render_mesh.empty()) {
        if (mesh_sequence) {
            struct stat st;
            while (stat(frame_path(render_mesh, mesh_frames).c_str(), &st) == 0) ++mesh_frames;
        } else if (render_mesh.find('%') == std::string::npos) {
            mesh_frames = render_frames;
        }
        if (mesh_frames < 1) {
            std::printf("%s %s: no frame 0 (a pattern has one %%d or %%0Nd; a static mesh takes --render-frames N >= 1)\n", voxelise ? "--voxelise-mesh" : "--render-mesh", render_mesh.c_str());
            return 2;
        }
    }
    sobfu_amd::Trajectory trajectory;  // --render-trajectory: the camera of every rendered frame
    if (!render_trajectory.empty()) {
        std::string why;
        if (!sobfu_amd::read_tum(render_trajectory, trajectory, &why)) {
            std::printf("--render-trajectory: %s\n", why.c_str());
            return 2;
        }
        if ((int) trajectory.size() < mesh_frames) {
            std::printf("--render-trajectory %s: %zu poses for %d frames\n", render_trajectory.c_str(), trajectory.size(), mesh_frames);
            return 2;
        }
        trajectory.resize((size_t) mesh_frames);
    }
    kfusion::cuda::setDevice(0);
    kfusion::cuda::printShortCudaDeviceInfo(0);
    // frame n of --render-mesh: read and posed once, one grid built over it
    auto load_rendered = [&](int n) {
        const std::string path = mesh_sequence ? frame_path(render_mesh, n) : render_mesh;
        if (path == rendered.path) return true;
        std::string why;
        rendered.path.clear();
        if (!sobfu_amd::read_ply(path, rendered.mesh, &why)) {
            std::printf("cannot read the mesh to render: %s\n", why.c_str());
            return false;
        }
        if (!render_pose.empty()) sobfu_amd::transform_points(rendered.mesh.vertices, mesh_pose);
        if (!rendered.grid.build(rendered.mesh.vertices, rendered.mesh.faces, 0.f, &why)) {
            std::printf("cannot render %s: %s\n", path.c_str(), why.c_str());
            return false;
        }
        rendered.path = path;
        return true;
    };
    if (!render_mesh.empty() && !load_rendered(0)) return 2;
    const bool mesh_coloured = textured && !render_mesh.empty() && !rendered.mesh.colours.empty();
    const bool coloured = (textured && render_mesh.empty()) || mesh_coloured || !colour_files.empty();
    SobFusion fusion(p);
    const int nframes = synthetic > 0 ? synthetic : !render_mesh.empty() ? mesh_frames : (int) files.size();
    std::vector<uint16_t> img, mask;
    std::vector<uint8_t> bgra;
    kfusion::cuda::Depth depth;
    kfusion::cuda::Image colour;
    kfusion::cuda::Cloud clean_points;  // --sensor: the clean render the sensor model reads
    kfusion::cuda::Normals clean_normals;
    double time_ms = 0.0;
    sobfu_amd::IndexedMesh tracked;  // --track-mesh: the canonical mesh cut after frame track_mesh
    for (int n = 0; n < nframes; ++n) {
        if (synthetic > 0) {
            render_sphere(shift * n, 0.0, 0.75, 0.1, p.intr, p.rows, p.cols, img);
            if (textured) render_sphere_colour(shift * n, 0.0, 0.75, 0.1, p.intr, p.rows, p.cols, bgra);
        } else if (!render_mesh.empty()) {
            if (!load_rendered(n)) return 2;
            if (mesh_coloured && rendered.mesh.colours.empty()) {
                std::printf("%s has no vertex colours, unlike frame 0\n", rendered.path.c_str());
                return 2;
            }
            if (!voxelise) {  // --voxelise-mesh renders no frame: the mesh itself is integrated below
                sobfu_amd::TriangleGrid::Camera cam;  // the depth camera; the meshes are in its frame with y and z negated
                cam.R[4] = cam.R[8] = -1.f;
                cam.fx = p.intr.fx, cam.fy = p.intr.fy, cam.cx = p.intr.cx, cam.cy = p.intr.cy, cam.rows = p.rows, cam.cols = p.cols;
                if (!trajectory.empty()) {  // inverse(pose n) after the flip
                    double R[9];
                    sobfu_amd::trajectory_rotation(trajectory[n], R);
                    cv::Affine3f pose, flip;
                    for (int k = 0; k < 9; ++k) pose.R[k] = (float) R[k];
                    for (int k = 0; k < 3; ++k) pose.t[k] = (float) trajectory[n].t[k];
                    flip.R[4] = flip.R[8] = -1.f;
                    const cv::Affine3f view = pose.inv() * flip;
                    std::copy(view.R, view.R + 9, cam.R), std::copy(view.t, view.t + 3, cam.t);
                }
                rendered.grid.render(cam, sensor ? nullptr : &depth, mesh_coloured ? &colour : nullptr, mesh_coloured ? &rendered.mesh.colours : nullptr,
                                     sensor ? &clean_points : nullptr, sensor ? &clean_normals : nullptr);
                if (sensor && !sobfu_amd::depth_sensor(clean_points, clean_normals, sensor_model, sensor_seed, (uint32_t) n, depth)) {
                    std::printf("--sensor: a parameter is outside its range (include/sobfu_hip.h, sobfu_hip_sensor_params)\n");
                    return 2;
                }
                img.resize((size_t) p.rows * p.cols);
                depth.download(img.data(), (size_t) p.cols * sizeof(uint16_t));
                if (mesh_coloured) {
                    bgra.resize((size_t) p.rows * p.cols * 4);
                    colour.download(bgra.data(), (size_t) p.cols * 4);
                }
            }
        } else {
            std::string why;
            if (!sobfu_amd::read_depth(files[n], p.rows, p.cols, img, &why)) {
                std::printf("cannot read depth frame %s: %s\n", files[n].c_str(), why.c_str());
                return 2;
            }
            if (!mask_files.empty()) {  // depth.copyTo(depth_masked, mask) (demo.cpp:314-317): masks are grey PNG / PGM / raw, or colour
                std::vector<uint8_t> cm;
                if (sobfu_amd::read_depth(mask_files[n], p.rows, p.cols, mask, &why)) {
                    for (size_t i = 0; i < img.size(); ++i) if (mask[i] == 0) img[i] = 0;
                } else if (sobfu_amd::read_colour(mask_files[n], p.rows, p.cols, cm, &why)) {
                    for (size_t i = 0; i < img.size(); ++i) if ((cm[4 * i] | cm[4 * i + 1] | cm[4 * i + 2]) == 0) img[i] = 0;
                } else {
                    std::printf("cannot read mask %s: %s\n", mask_files[n].c_str(), why.c_str());
                    return 2;
                }
            }
            if (!colour_files.empty() && !sobfu_amd::read_colour(colour_files[n], p.rows, p.cols, bgra, &why)) {
                std::printf("cannot read colour frame %s: %s\n", colour_files[n].c_str(), why.c_str());
                return 2;
            }
        }
        if (voxelise) {
            std::string why;
            kfusion::SampledScopeTime fps(time_ms);
            if (!fusion.integrate_mesh(rendered.mesh, sobfu_amd::mesh_frame(), false, &why, nullptr, mesh_sign)) {
                std::printf("cannot voxelise %s: %s\n", rendered.path.c_str(), why.c_str());
                return 2;
            }
        } else {
            depth.upload(img.data(), (size_t) p.cols * sizeof(uint16_t), p.rows, p.cols);  // demo.cpp:327-329
            if (coloured) colour.upload(bgra.data(), (size_t) p.cols * 4, p.rows, p.cols);
            kfusion::SampledScopeTime fps(time_ms);  // demo.cpp:331 -- "avg. frame time" every 34 frames
            if (coloured) fusion(depth, colour);
            else fusion(depth);
        }
        if (print_stats) stats("phi_global", *fusion.phi_global);
        auto save_mesh = [&](const char* name, const sobfu_amd::TriangleMesh& m) {  // demo.cpp:236-246 (name_frame.vtk)
            if (m.empty()) return;
            const std::string path = mesh_dir + "/" + name + "_" + std::to_string(n) + ".vtk";
            if (sobfu_amd::write_vtk(path, m)) std::printf("mesh %s: %zu triangles\n", name, m.triangles());
            else std::printf("cannot write %s\n", path.c_str());
        };
        auto save_ply = [&](const char* name, const sobfu_amd::IndexedMesh& m) {  // name_frame.ply
            if (m.empty()) return;
            const std::string path = mesh_dir + "/" + name + "_" + std::to_string(n) + ".ply";
            if (sobfu_amd::write_ply(path, m)) std::printf("mesh %s: %zu triangles, %zu vertices\n", name, m.triangles(), m.vertices.size());
            else std::printf("cannot write %s\n", path.c_str());
        };
        if (!mesh_dir.empty() && mesh_format == "ply") {
            save_ply("phi_global", fusion.get_phi_global_indexed_mesh());
            if (n > 0) save_ply("phi_n", fusion.get_phi_n_indexed_mesh());
            if (n > 0 && n >= p.start_frame) {
                save_ply("phi_n_psi", fusion.get_phi_n_psi_indexed_mesh());
                save_ply("phi_global_psi_inv", fusion.get_phi_global_psi_inv_indexed_mesh());
            }
        } else if (!mesh_dir.empty()) {
            save_mesh("phi_global", fusion.get_phi_global_mesh());
            if (n > 0) save_mesh("phi_n", fusion.get_phi_n_mesh());
            if (n > 0 && n >= p.start_frame) {
                save_mesh("phi_n_psi", fusion.get_phi_n_psi_mesh());
                save_mesh("phi_global_psi_inv", fusion.get_phi_global_psi_inv_mesh());
            }
        }
        const bool solved_frame = n > 0 && n >= p.start_frame;
        if (solved_frame && (warp_mesh || fit_stats)) {
            if (!fit_stats) {
                save_ply("phi_global_warped", fusion.get_phi_global_warped_indexed_mesh());
            } else {
                sobfu_amd::IndexedMesh m = fusion.get_phi_global_indexed_mesh();
                const sobfu_amd::MeshFit before = fusion.fit_to_live(m);
                m = fusion.warp_to_live(std::move(m));
                const sobfu_amd::MeshFit f = fusion.fit_to_live(m);
                if (warp_mesh) save_ply("phi_global_warped", m);
                std::printf("fit %d: %zu vertices, %zu valid, mean |d| %.4f mm, rms %.4f mm, max %.4f mm (unwarped rms %.4f mm)\n", n, f.vertices, f.valid,
                            1e3 * f.mean_abs, 1e3 * f.rms, 1e3 * f.max, 1e3 * before.rms);
            }
        }
        if (solved_frame && warp_stats) {
            sobfu_amd::WarpStats ws;
            std::vector<float> det, res;
            const bool vols = !warp_stats_dump.empty();
            if (fusion.warp_stats(warp_stats_band, ws, vols ? &det : nullptr, vols ? &res : nullptr)) {
                std::printf("%s\n", sobfu_amd::format_warp_stats(ws, n).c_str());
                const size_t X = (size_t) ws.dims[0], Y = (size_t) ws.dims[1], Z = (size_t) ws.dims[2];
                if (vols && !sobfu_amd::write_npy(warp_stats_dump + "/detJ_" + std::to_string(n) + ".npy", det.data(), {Z, Y, X})) std::printf("cannot write detJ_%d.npy\n", n);
                if (vols && !sobfu_amd::write_npy(warp_stats_dump + "/invres_" + std::to_string(n) + ".npy", res.data(), {Z, Y, X})) std::printf("cannot write invres_%d.npy\n", n);
            }
        }
        if (solved_frame && !eval_live.empty() && !evaluate(fusion, frame_path(eval_live, n), true, n)) return 2;
        if (n == nframes - 1 && !eval_gt.empty() && !evaluate(fusion, eval_gt, false, n)) return 2;
        if (track_mesh >= 0 && n == track_mesh) tracked = fusion.get_phi_global_indexed_mesh();
        if (track_mesh >= 0 && n >= track_mesh && solved_frame) save_ply("tracked", fusion.warp_to_live(tracked));
        if (!shots.dir.empty()) {
            const bool solved = n > 0 && n >= p.start_frame;
            if (shots.write(n, fusion, solved, p.intr)) std::printf("screenshot %s/%06d.png\n", shots.dir.c_str(), n);
            else std::printf("cannot write screenshot %s/%06d.png\n", shots.dir.c_str(), n);
        }
        if (n > 0 && print_stats) {
            stats("phi_n", *fusion.phi_n);
            if (n >= p.start_frame) {
                stats("phi_n_psi", *fusion.phi_n_psi);
                stats("phi_global_psi_inv", *fusion.phi_global_psi_inv);
                const sobfu_hip_solver_report& r = fusion.solver->last_report;
                std::printf("solver: iterations=%d converged=%d last_max_update_norm=%g\n", r.iterations, r.converged, r.last_max_update_norm);
            }
        }
    }
    sobfu_amd::Trajectory tracked_poses;  // TUM trajectory format: frame tx ty tz qx qy qz qw
    for (size_t n = 0; n < fusion.getPoses().size(); ++n) tracked_poses.push_back(sobfu_amd::trajectory_pose((int) n, fusion.getPoses()[n].R, fusion.getPoses()[n].t));
    if (!poses_path.empty() && !sobfu_amd::write_tum(poses_path, tracked_poses)) {
        std::printf("cannot write %s\n", poses_path.c_str());
        return 2;
    }
    if (p.track_camera && !trajectory.empty()) {  // the tracked poses against the trajectory the frames were rendered from
        double rpe_trans = NAN, rpe_rot = NAN;
        sobfu_amd::rpe(tracked_poses, trajectory, &rpe_trans, &rpe_rot);
        std::printf("trajectory: ate=%.9g rpe_trans=%.9g rpe_rot=%.9g\n", sobfu_amd::ate(tracked_poses, trajectory), rpe_trans, rpe_rot);
    }
    if (!dump.empty() && fusion.psi) {  // .npy dumps (replace the reference's commented-out .vti writer, demo.cpp:252-283)
        cv::Vec3i d = p.volume_dims;
        const size_t n = (size_t) d[0] * d[1] * d[2], Z = (size_t) d[2], Y = (size_t) d[1], X = (size_t) d[0];
        std::vector<float4> h(n);
        std::vector<float2> t(n);
        auto field = [&](const char* name, sobfu::cuda::DeformationField& f) {
            f.get_data().download(h.data());
            if (!sobfu_amd::write_npy(dump + "/" + name + ".npy", (const float*) h.data(), {Z, Y, X, 4})) std::printf("cannot write %s\n", name);
        };
        auto volume = [&](const char* name, kfusion::cuda::TsdfVolume& v) {
            v.data().download(t.data());
            if (!sobfu_amd::write_npy(dump + "/" + name + ".npy", (const float*) t.data(), {Z, Y, X, 2})) std::printf("cannot write %s\n", name);
        };
        field("psi", *fusion.psi);
        if (fusion.psi_inv) field("psi_inv", *fusion.psi_inv);
        volume("phi_global", *fusion.phi_global);
        if (fusion.phi_n) volume("phi_n", *fusion.phi_n);
        if (fusion.phi_n_psi) volume("phi_n_psi", *fusion.phi_n_psi);
        if (fusion.phi_global_psi_inv) volume("phi_global_psi_inv", *fusion.phi_global_psi_inv);
        if (fusion.colour_global) {
            std::vector<kfusion::RGB> c(n);
            fusion.colour_global->data().download(c.data());
            if (!sobfu_amd::write_npy(dump + "/colour_global.npy", (const uint8_t*) c.data(), {Z, Y, X, 4})) std::printf("cannot write colour_global\n");
        }
    }
    return 0;
}
