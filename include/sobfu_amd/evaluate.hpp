// Reconstruction error against a ground-truth mesh (no reference counterpart; kernels and rules: sobfu_amd/csrc/mesh_distance_kernels.hip,
// DESIGN.md 4.9): a PLY reader, the triangle grid over the C ABI, the two-way vertex-to-surface comparison and its statistics.  Part of
// sobfu.hpp, which includes it after IndexedMesh, DeviceArray and sobfuSafeCall: not a header to include on its own.  The Python twins are
// sobfu_amd/mesh_io.py (read_ply) and sobfu_amd/evaluate.py (compare_meshes, align_meshes).  Automatic rigid alignment of the ground truth
// (sobfu_amd/csrc/mesh_align_kernels.hip): TriangleGrid::align, align_meshes, format_alignment.  Rays and a camera over
// the same grid (sobfu_amd/csrc/mesh_ray_kernels.hip): TriangleGrid::raycast, TriangleGrid::render.  Closed meshes as signed
// TSDF volumes and the inside / outside test (sobfu_amd/csrc/mesh_voxel_kernels.hip): TriangleGrid::voxelise,
// TriangleGrid::inside, mesh_to_tsdf, and the signed fields of compare_meshes.  Open meshes through generalised winding numbers (DESIGN.md 4.14,
// sobfu_amd/csrc/mesh_winding_kernels.hip): TriangleGrid::boundary, TriangleGrid::winding, and MeshSign on voxelise, mesh_to_tsdf and compare_meshes.
// Area-weighted surface samples and precision / recall / F-score over them (sobfu_amd/csrc/mesh_sample_kernels.hip): sample_mesh,
// distance_score, f_score, format_f_score.
#pragma once

#include "../../sobfu_amd/csrc/sobfu_rigid.hpp"  // the rigid inverse, the same lines as the kernels'

namespace sobfu_amd {

// ---- read_ply: the rules and refusals of sobfu_amd.mesh_io.read_ply -------------------------------------------------------------------
// ASCII or binary little-endian PLY 1.0 -> vertices (w = 1), normals (w = 1; empty when the file has none), faces, colours (empty when
// the file has none).  Vertex properties in any order, unknown scalar properties skipped; face lists with any integer count and index
// types.  false + *why for: polygons other than triangles, big-endian files, element counts the file is too short for, vertex indices
// out of range, a header it cannot parse.
namespace ply_detail {
struct Prop {
    std::string name;
    int type = -1, count_type = -1;  // indices into kTypes; count_type >= 0: a list
};
struct Element {
    std::string name;
    size_t count = 0;
    std::vector<Prop> props;
};
struct Type {
    const char *a, *b;
    int size;
    char kind;  // i, u, f
};
static const Type kTypes[8] = {{"char", "int8", 1, 'i'},   {"uchar", "uint8", 1, 'u'}, {"short", "int16", 2, 'i'},  {"ushort", "uint16", 2, 'u'},
                               {"int", "int32", 4, 'i'},   {"uint", "uint32", 4, 'u'}, {"float", "float32", 4, 'f'}, {"double", "float64", 8, 'f'}};
inline int type_of(const std::string& s) {
    for (int i = 0; i < 8; ++i)
        if (s == kTypes[i].a || s == kTypes[i].b) return i;
    return -1;
}
// one little-endian scalar at p (the caller has checked the bounds)
inline double scalar_at(const unsigned char* p, int type) {
    switch (type) {
        case 0: { signed char v; std::memcpy(&v, p, 1); return v; }
        case 1: return *p;
        case 2: { short v; std::memcpy(&v, p, 2); return v; }
        case 3: { unsigned short v; std::memcpy(&v, p, 2); return v; }
        case 4: { int v; std::memcpy(&v, p, 4); return v; }
        case 5: { unsigned v; std::memcpy(&v, p, 4); return v; }
        case 6: { float v; std::memcpy(&v, p, 4); return v; }
        default: { double v; std::memcpy(&v, p, 8); return v; }
    }
}
inline std::vector<std::string> words(const std::string& line) {
    std::vector<std::string> w;
    std::istringstream is(line);
    for (std::string s; is >> s;) w.push_back(s);
    return w;
}
inline bool all_digits(const std::string& s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos && s.size() <= 18; }
}  // namespace ply_detail

inline bool read_ply(const std::string& path, IndexedMesh& m, std::string* why = nullptr) {
    using namespace ply_detail;
    auto fail = [&](const std::string& msg) {
        if (why) *why = path + ": " + msg;
        return false;
    };
    m = IndexedMesh();
    std::vector<unsigned char> buf;
    {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) return fail("cannot open");
        unsigned char chunk[65536];
        for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
        std::fclose(f);
    }
    const std::string text(buf.begin(), buf.end());
    if (text.compare(0, 4, "ply\n") != 0 && text.compare(0, 4, "ply\r") != 0) return fail("not a PLY file");
    const size_t end = text.find("end_header"), nl = end == std::string::npos ? end : text.find('\n', end);
    if (nl == std::string::npos) return fail("the PLY header has no end_header line");
    std::string fmt;
    std::vector<Element> elements;
    {
        std::istringstream hs(text.substr(0, end));
        std::string line;
        std::getline(hs, line);  // "ply"
        while (std::getline(hs, line)) {
            const std::vector<std::string> w = words(line);
            if (w.empty() || w[0] == "comment" || w[0] == "obj_info") continue;
            if (w[0] == "format" && w.size() == 3) {
                if (w[1] == "binary_big_endian") return fail("big-endian PLY files are not supported");
                if ((w[1] != "ascii" && w[1] != "binary_little_endian") || w[2] != "1.0") return fail("unknown PLY format");
                fmt = w[1];
            } else if (w[0] == "element" && w.size() == 3 && all_digits(w[2])) {
                Element e;
                e.name = w[1], e.count = (size_t) std::strtoull(w[2].c_str(), nullptr, 10);
                elements.push_back(e);
            } else if (w[0] == "property" && !elements.empty() && w.size() == 3 && type_of(w[1]) >= 0) {
                Prop p;
                p.name = w[2], p.type = type_of(w[1]);
                elements.back().props.push_back(p);
            } else if (w[0] == "property" && !elements.empty() && w.size() == 5 && w[1] == "list" && type_of(w[2]) >= 0 && type_of(w[3]) >= 0) {
                Prop p;
                p.name = w[4], p.count_type = type_of(w[2]), p.type = type_of(w[3]);
                elements.back().props.push_back(p);
            } else {
                return fail("cannot read the PLY header line '" + line + "'");
            }
        }
    }
    if (fmt.empty()) return fail("the PLY header has no format line");
    const bool ascii = fmt == "ascii";
    size_t off = nl + 1;
    std::vector<std::string> tokens;
    size_t tok = 0;
    if (ascii) tokens = words(text.substr(off));
    bool have_vertex = false, have_normals = false, have_colours = false;
    for (const Element& e : elements) {
        size_t lists = 0;
        for (const Prop& p : e.props) lists += p.count_type >= 0;
        if (lists && (e.name != "face" || e.props.size() != 1)) return fail("element " + e.name + " has list properties this reader does not handle");
        const std::string too_short = "element " + e.name + " declares " + std::to_string(e.count) + " entries, more than the file holds";
        if (!lists) {  // fixed-size records
            const size_t np = e.props.size();
            size_t rec = 0;
            for (const Prop& p : e.props) rec += (size_t) kTypes[p.type].size;
            if (ascii ? (np && e.count > (tokens.size() - tok) / np) : (rec && e.count > (buf.size() - off) / rec)) return fail(too_short);
            const bool vertex = e.name == "vertex";
            int ix[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};  // x y z nx ny nz red green blue -> property index
            static const char* kNames[9] = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"};
            for (size_t j = 0; vertex && j < np; ++j)
                for (int k = 0; k < 9; ++k)
                    if (e.props[j].name == kNames[k]) ix[k] = (int) j;
            if (vertex) {
                if (ix[0] < 0 || ix[1] < 0 || ix[2] < 0) return fail("the vertex element has no x, y, z");
                have_vertex = true, have_normals = ix[3] >= 0 && ix[4] >= 0 && ix[5] >= 0, have_colours = ix[6] >= 0 && ix[7] >= 0 && ix[8] >= 0;
                m.vertices.resize(e.count);
                if (have_normals) m.normals.resize(e.count);
                if (have_colours) m.colours.resize(e.count);
            }
            std::vector<double> row(np);
            for (size_t i = 0; i < e.count; ++i) {
                for (size_t j = 0; j < np; ++j) {
                    if (ascii) {
                        char* stop = nullptr;
                        row[j] = std::strtod(tokens[tok].c_str(), &stop);
                        if (stop == tokens[tok].c_str() || *stop) return fail("element " + e.name + " holds something that is not a number");
                        ++tok;
                    } else {
                        row[j] = scalar_at(buf.data() + off, e.props[j].type);
                        off += (size_t) kTypes[e.props[j].type].size;
                    }
                }
                if (!vertex) continue;
                m.vertices[i] = make_float4((float) row[ix[0]], (float) row[ix[1]], (float) row[ix[2]], 1.f);
                if (have_normals) m.normals[i] = make_float4((float) row[ix[3]], (float) row[ix[4]], (float) row[ix[5]], 1.f);
                if (have_colours) {
                    kfusion::RGB c;
                    c.bgra = 0;
                    c.r = (unsigned char) row[ix[6]], c.g = (unsigned char) row[ix[7]], c.b = (unsigned char) row[ix[8]];
                    m.colours[i] = c;
                }
            }
            continue;
        }
        if (!have_vertex) return fail("the face element comes before the vertex element");
        const Prop& p = e.props[0];
        if (kTypes[p.count_type].kind == 'f' || kTypes[p.type].kind == 'f') return fail("the face list must have integer counts and indices");
        const size_t cs = (size_t) kTypes[p.count_type].size, is = (size_t) kTypes[p.type].size, V = m.vertices.size();
        if (ascii ? e.count > (tokens.size() - tok) / 4 : e.count > (buf.size() - off) / (cs + 3 * is)) {
            // a short file, unless its first polygon already says why the sizes do not add up
            if (!ascii && e.count && buf.size() - off >= cs && scalar_at(buf.data() + off, p.count_type) != 3.0)
                return fail("only triangles are supported, found a polygon of another size");
            return fail(too_short);
        }
        m.faces.resize(3 * e.count);
        for (size_t i = 0; i < e.count; ++i) {
            double v[4];
            for (int j = 0; j < 4; ++j) {
                if (ascii) {
                    char* stop = nullptr;
                    v[j] = (double) std::strtoll(tokens[tok].c_str(), &stop, 10);
                    if (stop == tokens[tok].c_str() || *stop) return fail("the face element holds something that is not an integer");
                    ++tok;
                } else {
                    v[j] = scalar_at(buf.data() + off, j ? p.type : p.count_type);
                    off += j ? is : cs;
                }
                if (j == 0 && v[0] != 3.0) return fail("only triangles are supported, found a polygon of another size");
            }
            for (int j = 1; j < 4; ++j) {
                if (v[j] < 0 || v[j] >= (double) V) return fail("a face refers to a vertex outside [0, " + std::to_string(V) + ")");
                m.faces[3 * i + (size_t) j - 1] = (int) v[j];
            }
        }
    }
    if (!have_vertex) return fail("no vertex element");
    return true;
}

// What sobfu_hip_mesh_align_estimate reported (sobfu_amd.ops.align_info): the status word; the updates applied; stopped by the gate;
// the solve of iteration `iterations` failed (the pose before it is kept); per iteration that ran: inliers, rms residual, |w|, |t_inc|
struct Alignment {
    int status = 0, iterations = 0;
    bool converged = false, failed = false;
    std::vector<float> trace;
};

// the inside / outside rule of voxelise, mesh_to_tsdf, compare_meshes and SobFusion::integrate_mesh: the parity of the row crossings (closed
// meshes) or the generalised winding number (any oriented mesh)
enum MeshSign { kSignParity = 0, kSignWinding = 1 };

// ---- TriangleGrid: the grid of sobfu_hip_mesh_grid_build over a mesh kept on the device ---------------------------------------------
class TriangleGrid {
public:
    // false (+ *why): a face index out of range or a non-finite corner -- there is no grid to query then
    bool build(const std::vector<float4>& vertices, const std::vector<int>& faces, float cell = 0.f, std::string* why = nullptr) {
        built_ = has_boundary_ = false;
        nb_ = 0, boundary_.release();
        nv_ = (int) vertices.size(), nt_ = (int) (faces.size() / 3);
        float bbox[6] = {0, 0, 0, 0, 0, 0};
        bool any = false;
        for (const float4& v : vertices) {
            if (!(std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z)) || nt_ == 0) continue;
            const float c[3] = {v.x, v.y, v.z};
            for (int i = 0; i < 3; ++i) {
                bbox[i]     = any ? std::min(bbox[i], c[i]) : c[i];
                bbox[3 + i] = any ? std::max(bbox[3 + i], c[i]) : c[i];
            }
            any = true;
        }
        sobfuSafeCall(sobfu_hip_mesh_grid_plan(bbox, nt_, cell, origin_, &h_, dims_));
        vertices_.release(), faces_.release();
        if (nv_) vertices_.upload(vertices);
        if (nt_) faces_.upload(faces.data(), 3 * (size_t) nt_);
        int max_refs = 8 * nt_ + 1024, refs = 0;
        for (;;) {
            workspace_.create(sobfu_hip_mesh_grid_workspace_bytes(dims_, max_refs));
            const int rc = sobfu_hip_mesh_grid_build(nv_ ? (const float*) vertices_.ptr() : nullptr, nv_, nt_ ? faces_.ptr() : nullptr, nt_, origin_, h_, dims_,
                                                     workspace_.ptr(), workspace_.size(), max_refs, &refs, nullptr);
            if (rc == SOBFU_E_UNSUPPORTED && refs > max_refs) {
                max_refs = refs;
                continue;
            }
            if (rc == SOBFU_E_BADARG) {
                if (why) *why = "the mesh has a face index out of range or a non-finite corner";
                return false;
            }
            sobfuSafeCall(rc);
            break;
        }
        references_ = refs;
        return built_ = true;
    }
    // distances (+Inf: farther than max_dist), and optionally the nearest triangles and closest points, of `points`
    void query(const std::vector<float4>& points, std::vector<float>& dist, float max_dist = 0.f, std::vector<int>* tri = nullptr,
               std::vector<float4>* closest = nullptr, int mode = SOBFU_MESH_DISTANCE_AUTO, int ring_cap = 0) {
        if (!built_) kfusion::cuda::error("TriangleGrid::query without a built grid", __FILE__, __LINE__);
        const size_t n = points.size();
        dist.assign(n, 0.f);
        if (tri) tri->assign(n, -1);
        if (closest) closest->assign(n, make_float4(0.f, 0.f, 0.f, 0.f));
        if (n == 0) return;
        kfusion::cuda::DeviceArray<float4> dp, dc;
        kfusion::cuda::DeviceArray<float> dd(n);
        kfusion::cuda::DeviceArray<int> dt(n), du(n);
        dp.upload(points);
        if (closest) dc.create(n);
        sobfuSafeCall(with_target(sobfu_hip_mesh_distance, (const float*) dp.ptr(), (int) n, max_dist, mode, ring_cap, dd.ptr(), dt.ptr(),
                                  closest ? (float*) dc.ptr() : nullptr, du.ptr(), nullptr));
        dd.download(dist);
        if (tri) dt.download(*tri);
        if (closest) dc.download(*closest);
    }
    // Point-to-plane ICP of `points` against this mesh from `pose` (row-major 4 x 4, points -> this mesh's frame), refined in place:
    // `iters` iterations enqueued as one chain, one synchronisation to read the result.  dof 6: rigid, 3: translation only; the loop
    // stops early once an update is below both eps_rot and eps_trans (0: never).  Without points: failed at iteration 0.
    Alignment align(const std::vector<float4>& points, float pose[16], int iters = 30, float max_dist = 0.f, int dof = 6, float eps_rot = 0.f,
                    float eps_trans = 0.f, int mode = SOBFU_MESH_DISTANCE_AUTO, int ring_cap = 0) {
        if (!built_) kfusion::cuda::error("TriangleGrid::align without a built grid", __FILE__, __LINE__);
        const int n = (int) points.size();
        int status = iters > 0 ? 0x10000 : 0;
        std::vector<float> trace((size_t) 4 * (size_t) std::max(iters, 1), 0.f);
        if (n > 0) {
            kfusion::cuda::DeviceArray<float4> dp;
            kfusion::cuda::DeviceArray<float> dpose, dtrace;
            kfusion::cuda::DeviceArray<int> dstatus(1);
            kfusion::cuda::DeviceArray<unsigned char> ws(sobfu_hip_mesh_align_workspace_bytes(n));
            dp.upload(points);
            dpose.upload(pose, 16);
            dtrace.upload(trace);
            sobfuSafeCall(with_target(sobfu_hip_mesh_align_estimate, (const float*) dp.ptr(), n, max_dist, mode, ring_cap, iters, dof, eps_rot, eps_trans,
                                      ws.ptr(), ws.size(), dpose.ptr(), dstatus.ptr(), dtrace.ptr(), nullptr));
            std::vector<float> got;
            std::vector<int> st;
            dstatus.download(st);
            dpose.download(got);
            dtrace.download(trace);
            std::copy(got.begin(), got.end(), pose);
            status = st[0];
        }
        Alignment a;
        a.status = status, a.failed = (status & 0x10000) != 0, a.converged = (status & 0x20000) != 0;
        a.iterations = status ? (status & 0xFFFF) : iters;
        trace.resize((size_t) 4 * (size_t) std::min(iters, a.iterations + (a.failed ? 1 : 0)));
        a.trace.swap(trace);
        return a;
    }
    // ---- rays against this mesh (sobfu_amd/csrc/mesh_ray_kernels.hip; ops.TriangleGrid.raycast / render) ----
    // per ray o + t d (d not normalised): the smallest t in (t_min, t_max] at which it meets a triangle (t_max <= 0: unlimited) and the
    // lowest triangle index there; optionally the weights (u, v) of that triangle's second and third corner and the side, +1 for the
    // face whose corners run counter-clockwise as seen from the origin, -1 for the other.  A miss is (+Inf, -1, (0, 0), 0).
    void raycast(const std::vector<float4>& origins, const std::vector<float4>& dirs, std::vector<float>& t, std::vector<int>& tri, float t_min = 0.f,
                 float t_max = 0.f, std::vector<float2>* bary = nullptr, std::vector<signed char>* side = nullptr, int mode = SOBFU_MESH_DISTANCE_AUTO) {
        if (!built_) kfusion::cuda::error("TriangleGrid::raycast without a built grid", __FILE__, __LINE__);
        if (origins.size() != dirs.size()) kfusion::cuda::error("TriangleGrid::raycast: one direction per origin", __FILE__, __LINE__);
        const size_t n = origins.size();
        t.assign(n, INFINITY), tri.assign(n, -1);
        if (bary) bary->assign(n, make_float2(0.f, 0.f));
        if (side) side->assign(n, 0);
        if (n == 0) return;
        kfusion::cuda::DeviceArray<float4> dorg, ddir;
        kfusion::cuda::DeviceArray<float> dt(n);
        kfusion::cuda::DeviceArray<int> dtri(n);
        kfusion::cuda::DeviceArray<float2> dbary;
        kfusion::cuda::DeviceArray<signed char> dside;
        dorg.upload(origins), ddir.upload(dirs);
        if (bary) dbary.create(n);
        if (side) dside.create(n);
        sobfuSafeCall(with_target(sobfu_hip_mesh_raycast, (const float*) dorg.ptr(), (const float*) ddir.ptr(), (int) n, t_min, t_max, mode, dt.ptr(),
                                  dtri.ptr(), bary ? (float*) dbary.ptr() : nullptr, side ? (int8_t*) dside.ptr() : nullptr, nullptr));
        dt.download(t), dtri.download(tri);
        if (bary) dbary.download(*bary);
        if (side) dside.download(*side);
    }
    // The mesh seen by a pinhole camera: (R row-major, t) takes the mesh's frame to the camera frame (the pose of sobfu_hip_raycast), depths
    // limited to (z_min, z_max] (z_max <= 0: unlimited).  Every output is optional: depth, uint16 millimetres, 0 for a miss; points and
    // normals in sobfu_hip_raycast's format; colour (needs vertex_colours, one per vertex), BGRA with alpha 255 on a hit; tri, -1 for a
    // miss.  vertex_normals (one per vertex) are mixed over the face; without them the face's own normal is used.
    struct Camera {
        float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
        float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
        int rows = 0, cols = 0;
        float z_min = 0.f, z_max = 0.f;
    };
    void render(const Camera& cam, kfusion::cuda::Depth* depth, kfusion::cuda::DeviceArray2D<kfusion::RGB>* colour = nullptr,
                const std::vector<kfusion::RGB>* vertex_colours = nullptr, kfusion::cuda::DeviceArray2D<float4>* points = nullptr,
                kfusion::cuda::DeviceArray2D<float4>* normals = nullptr, const std::vector<float4>* vertex_normals = nullptr,
                kfusion::cuda::DeviceArray2D<int>* tri = nullptr) {
        if (!built_) kfusion::cuda::error("TriangleGrid::render without a built grid", __FILE__, __LINE__);
        if ((vertex_colours && (int) vertex_colours->size() != nv_) || (vertex_normals && (int) vertex_normals->size() != nv_) || (colour && !vertex_colours))
            kfusion::cuda::error("TriangleGrid::render: one normal / colour per vertex, and colours for a colour image", __FILE__, __LINE__);
        kfusion::cuda::DeviceArray<kfusion::RGB> dcol;
        kfusion::cuda::DeviceArray<float4> dnrm;
        if (vertex_colours && nv_) dcol.upload(*vertex_colours);
        if (vertex_normals && nv_) dnrm.upload(*vertex_normals);
        if (depth) depth->create(cam.rows, cam.cols);
        if (colour) colour->create(cam.rows, cam.cols);
        if (points) points->create(cam.rows, cam.cols);
        if (normals) normals->create(cam.rows, cam.cols);
        if (tri) tri->create(cam.rows, cam.cols);
        sobfuSafeCall(with_target(sobfu_hip_mesh_render, vertex_normals && nv_ ? (const float*) dnrm.ptr() : nullptr,
                                  vertex_colours && nv_ ? (const uint8_t*) dcol.ptr() : nullptr, cam.R, cam.t, cam.fx, cam.fy, cam.cx, cam.cy, cam.rows, cam.cols,
                                  cam.z_min, cam.z_max, depth ? depth->ptr() : nullptr, depth ? (int) depth->step() : 0,
                                  points ? (float*) points->ptr() : nullptr, points ? (int) points->step() : 0,
                                  normals ? (float*) normals->ptr() : nullptr, normals ? (int) normals->step() : 0,
                                  colour ? (uint8_t*) colour->ptr() : nullptr, colour ? (int) colour->step() : 0, tri ? tri->ptr() : nullptr,
                                  tri ? (int) tri->step() : 0, nullptr));
        sobfuSafeCall(hipDeviceSynchronize());  // the vertex attributes uploaded above are released on return
    }
    // ---- this mesh, closed, as a signed TSDF volume and an inside / outside test (sobfu_amd/csrc/mesh_voxel_kernels.hip, DESIGN.md 4.12;
    // ops.TriangleGrid.voxelise / inside) ----
    // d_vol: dims[0] x dims[1] x dims[2] float2 {tsdf, weight} on the device, the mesh's vertices being in the volume's frame: voxel i of
    // an axis has its centre at i vs + vs / 2; tsdf = clamp(s / trunc, -1, 1), s the exact distance to the mesh, negative inside; weight =
    // s > -eta.  -> the number of rows along x that cross the mesh an odd number of times: 0 for a closed mesh (synchronises).
    // sign: kSignParity (a closed mesh: inside iff the row crosses it an odd number of times beyond the voxel) or kSignWinding (any oriented
    // mesh, open ones included: inside iff the generalised winding number exceeds 1 / 2; the count returned is then only
    // information); d_winding (kSignWinding, may be NULL): dims[0] x dims[1] x dims[2] floats on the device, w at every voxel centre
    int voxelise(float* d_vol, const int dims[3], const float vs[3], float trunc, float eta, int mode = SOBFU_MESH_DISTANCE_AUTO, int sign = kSignParity,
                 float* d_winding = nullptr) {
        if (!built_) kfusion::cuda::error("TriangleGrid::voxelise without a built grid", __FILE__, __LINE__);
        const bool winding = sign == kSignWinding;
        if (!winding && (sign != kSignParity || d_winding))
            kfusion::cuda::error("TriangleGrid::voxelise: unknown sign, or d_winding without kSignWinding", __FILE__, __LINE__);
        const size_t bytes = (winding ? sobfu_hip_mesh_voxelise_winding_workspace_bytes : sobfu_hip_mesh_voxelise_workspace_bytes)(dims[0], dims[1], dims[2]);
        if (bytes == 0) kfusion::cuda::error("TriangleGrid::voxelise: at most 512 voxels along x", __FILE__, __LINE__);
        if (winding) boundary();
        kfusion::cuda::DeviceArray<unsigned char> ws(bytes);
        kfusion::cuda::DeviceArray<int> open_rows(1);
        // the winding entry point takes the boundary behind the target and d_winding ahead of the stream
        if (winding)
            sobfuSafeCall(with_target(sobfu_hip_mesh_voxelise_winding, nb_ ? (const float*) boundary_.ptr() : nullptr, nb_, d_vol, dims[0], dims[1], dims[2], vs, trunc,
                                      eta, mode, ws.ptr(), ws.size(), open_rows.ptr(), d_winding, nullptr));
        else
            sobfuSafeCall(with_target(sobfu_hip_mesh_voxelise, d_vol, dims[0], dims[1], dims[2], vs, trunc, eta, mode, ws.ptr(), ws.size(), open_rows.ptr(), nullptr));
        std::vector<int> n;
        open_rows.download(n);
        return n[0];
    }
    // per point: inside = 1 where the row from it along +x crosses the mesh an odd number of times; open = 1 where its whole row does
    void inside(const std::vector<float4>& points, std::vector<unsigned char>& inside, std::vector<unsigned char>& open, int mode = SOBFU_MESH_DISTANCE_AUTO) {
        if (!built_) kfusion::cuda::error("TriangleGrid::inside without a built grid", __FILE__, __LINE__);
        const size_t n = points.size();
        inside.assign(n, 0), open.assign(n, 0);
        if (n == 0) return;
        kfusion::cuda::DeviceArray<float4> dp;
        kfusion::cuda::DeviceArray<unsigned char> di(n), dopen(n);
        dp.upload(points);
        sobfuSafeCall(with_target(sobfu_hip_mesh_inside, (const float*) dp.ptr(), (int) n, di.ptr(), dopen.ptr(), mode, nullptr));
        di.download(inside), dopen.download(open);
    }
    // ---- generalised winding numbers (sobfu_amd/csrc/mesh_winding_kernels.hip; ops.TriangleGrid.winding) ----
    // the boundary chain, computed once and kept on the device: two float4 per edge, (u, k) and (v, 0) -> the number of edges (0: closed)
    int boundary() {
        if (!built_) kfusion::cuda::error("TriangleGrid::boundary without a built grid", __FILE__, __LINE__);
        if (has_boundary_) return nb_;
        std::vector<int> faces, edges;
        std::vector<float4> vertices;
        if (nt_) faces_.download(faces);
        if (nv_) vertices_.download(vertices);
        int count = 0;
        sobfuSafeCall(sobfu_hip_mesh_boundary(nt_ ? faces.data() : nullptr, nt_, nv_, nullptr, 0, &count));
        edges.resize(3 * (size_t) count);
        if (count) sobfuSafeCall(sobfu_hip_mesh_boundary(faces.data(), nt_, nv_, edges.data(), count, &count));
        std::vector<float4> pairs(2 * (size_t) count);
        for (int e = 0; e < count; ++e) {
            const float4 &u = vertices[edges[3 * e]], &v = vertices[edges[3 * e + 1]];
            pairs[2 * e] = make_float4(u.x, u.y, u.z, (float) edges[3 * e + 2]), pairs[2 * e + 1] = make_float4(v.x, v.y, v.z, 0.f);
        }
        if (count) boundary_.upload(pairs);
        nb_ = count, has_boundary_ = true;
        return nb_;
    }
    // per point: the winding number -- 1 inside and 0 outside a closed, outward-oriented mesh, smooth across holes; inside iff > 1 / 2.
    // mode: SOBFU_MESH_WINDING_BOUNDARY (crossings + boundary strips) or _SUM (the definition); walk: the crossing walk, never changes a bit
    void winding(const std::vector<float4>& points, std::vector<float>& w, int mode = SOBFU_MESH_WINDING_BOUNDARY, int walk = SOBFU_MESH_DISTANCE_AUTO) {
        if (!built_) kfusion::cuda::error("TriangleGrid::winding without a built grid", __FILE__, __LINE__);
        const size_t n = points.size();
        w.assign(n, 0.f);
        if (n == 0) return;
        boundary();
        kfusion::cuda::DeviceArray<float4> dp;
        kfusion::cuda::DeviceArray<float> dw(n);
        dp.upload(points);
        sobfuSafeCall(with_target(sobfu_hip_mesh_winding, nb_ ? (const float*) boundary_.ptr() : nullptr, nb_, (const float*) dp.ptr(), (int) n, dw.ptr(), mode,
                                  walk, nullptr));
        dw.download(w);
    }
    bool built() const { return built_; }
    int references() const { return references_; }
    const int* dims() const { return dims_; }
    float cell() const { return h_; }

private:
    // a mesh entry point of the C ABI, called with its nine leading arguments (the grid's workspace, the mesh, the plan) ahead of the caller's
    template <class F, class... A>
    int with_target(F f, A... a) {
        return f(workspace_.ptr(), workspace_.size(), nv_ ? (const float*) vertices_.ptr() : nullptr, nv_, nt_ ? faces_.ptr() : nullptr, nt_, origin_, h_,
                 dims_, a...);
    }
    kfusion::cuda::DeviceArray<float4> vertices_;
    kfusion::cuda::DeviceArray<int> faces_;
    kfusion::cuda::DeviceArray<unsigned char> workspace_;
    kfusion::cuda::DeviceArray<float4> boundary_;
    float origin_[3] = {0, 0, 0}, h_ = 0.f;
    int dims_[3] = {1, 1, 1}, nv_ = 0, nt_ = 0, references_ = 0, nb_ = 0;
    bool built_ = false, has_boundary_ = false;
};

// ---- the depth sensor model (sobfu_amd/csrc/depth_sensor_kernels.hip; ops.SensorModel / ops.depth_sensor) ---------------
// The fields of sobfu_hip_sensor_params but seed and frame; include/sobfu_hip.h states the rule they enter.
struct SensorModel {
    float lateral = 0.f, z_min = 0.f, z_max = INFINITY, cos_min = 0.f;
    int edge_radius = 0;
    float edge_jump = 0.f, edge_drop = 0.f, drop = 0.f, a0 = 0.f, a1 = 0.f, z0 = 0.f, a2 = 0.f, disparity = 0.f;
    // the identity: the frame is the renderer's own depth image
    static SensorModel ideal() { return SensorModel(); }
    // a first-generation structured-light camera (disparity: 8 sub-pixel levels x 0.075 m x 580 px)
    static SensorModel kinect() {
        SensorModel m;
        m.lateral = 0.8f, m.z_min = 0.4f, m.z_max = 4.f, m.cos_min = 0.2f, m.edge_radius = 1, m.edge_jump = 0.05f, m.edge_drop = 0.5f, m.drop = 0.f;
        m.a0 = 0.0012f, m.a1 = 0.0019f, m.z0 = 0.4f, m.a2 = 0.0001f, m.disparity = 348.f;
        return m;
    }
    // a field by its name in the struct; false: no such field
    bool set(const std::string& name, double value) {
        float* const fields[] = {&lateral, &z_min, &z_max, &cos_min, &edge_jump, &edge_drop, &drop, &a0, &a1, &z0, &a2, &disparity};
        const char* const names[] = {"lateral", "z_min", "z_max", "cos_min", "edge_jump", "edge_drop", "drop", "a0", "a1", "z0", "a2", "disparity"};
        if (name == "edge_radius") return edge_radius = (int) value, true;
        for (int i = 0; i < 12; ++i)
            if (name == names[i]) return *fields[i] = (float) value, true;
        return false;
    }
    sobfu_hip_sensor_params params(uint64_t seed, uint32_t frame) const {
        return sobfu_hip_sensor_params{seed, frame, lateral, z_min, z_max, cos_min, edge_radius, edge_jump, edge_drop, drop, a0, a1, z0, a2, disparity};
    }
};
// What the sensor `model` reports of a clean render (points and normals as TriangleGrid::render and TsdfVolume::raycast give them): depth,
// uint16 millimetres, 0 where there is no reading; flags (optional), SOBFU_SENSOR_* per pixel.  The same (seed, frame) gives the same frame.
// false: a parameter of the model is out of its range
inline bool depth_sensor(const kfusion::cuda::DeviceArray2D<float4>& points, const kfusion::cuda::DeviceArray2D<float4>& normals, const SensorModel& model,
                         uint64_t seed, uint32_t frame, kfusion::cuda::Depth& depth, kfusion::cuda::DeviceArray2D<unsigned char>* flags = nullptr) {
    if (points.rows() != normals.rows() || points.cols() != normals.cols())
        kfusion::cuda::error("depth_sensor: points and normals differ in size", __FILE__, __LINE__);
    depth.create(points.rows(), points.cols());
    if (flags) flags->create(points.rows(), points.cols());
    const sobfu_hip_sensor_params p = model.params(seed, frame);
    const int rc = sobfu_hip_depth_sensor((const float*) points.ptr(), (int) points.step(), (const float*) normals.ptr(), (int) normals.step(), points.rows(),
                                          points.cols(), &p, depth.ptr(), (int) depth.step(), flags ? flags->ptr() : nullptr,
                                          flags ? (int) flags->step() : 0, nullptr);
    if (rc == SOBFU_E_BADARG) return false;
    sobfuSafeCall(rc);
    return true;
}

// ---- compare_meshes: float64 statistics over the finite distances, as sobfu_amd.evaluate.distance_stats ------------------------------
struct DistanceStats {
    size_t n = 0, within = 0;
    double mean = 0, rms = 0, median = 0, max = 0;
    // compare_meshes(..., with_signs): the mean over the finite distances, each negative where its vertex is inside the other mesh; how
    // many of those vertices are inside; how many of ALL the vertices lie on a row that crosses the other mesh an odd number of times
    bool has_signs = false;
    double signed_mean = 0;
    size_t inside = 0, open = 0;
};
struct MeshComparison {
    DistanceStats a_to_b, b_to_a;
    double chamfer = 0, hausdorff = 0;  // the mean of the two means; the larger of the two maxima
};
inline DistanceStats distance_stats(const std::vector<float>& dist) {
    DistanceStats s;
    s.n = dist.size();
    std::vector<double> f;
    for (float d : dist)
        if (std::isfinite(d)) f.push_back((double) d);
    if (f.empty()) return s;
    double s1 = 0, s2 = 0;
    for (double d : f) s1 += d, s2 += d * d, s.max = std::max(s.max, d);
    s.within = f.size();
    s.mean = s1 / (double) f.size(), s.rms = std::sqrt(s2 / (double) f.size());
    std::sort(f.begin(), f.end());
    s.median = f.size() % 2 ? f[f.size() / 2] : 0.5 * (f[f.size() / 2 - 1] + f[f.size() / 2]);
    return s;
}
// a = the model, b = the ground truth, by convention; vertex-to-surface both ways.  false: one of the meshes is refused (TriangleGrid::build)
// grid_b (optional): a grid already built over b -- the one its depth frame was rendered through -- used instead of building another
inline void add_signs(DistanceStats& s, const std::vector<float>& dist, const std::vector<unsigned char>& inside, const std::vector<unsigned char>& open) {
    double sum = 0;
    s.has_signs = true, s.signed_mean = 0, s.inside = s.open = 0;
    for (size_t i = 0; i < dist.size(); ++i) {
        s.open += open[i] != 0;
        if (!std::isfinite(dist[i])) continue;
        sum += inside[i] ? -(double) dist[i] : (double) dist[i];
        s.inside += inside[i] != 0;
    }
    if (s.within) s.signed_mean = sum / (double) s.within;
}
// with_signs: each direction gains signed_mean, inside and open -- the sign of the query vertex against the OTHER mesh (TriangleGrid::inside),
// which should be closed; the unsigned fields are the same with and without.  sign = kSignWinding: inside iff the other mesh's winding number
// exceeds 1 / 2 (TriangleGrid::winding), which is defined for open meshes too; `open` is counted as before
inline bool compare_meshes(const IndexedMesh& a, const IndexedMesh& b, float max_dist, MeshComparison& out, std::vector<float>* d_ab = nullptr,
                           std::vector<float>* d_ba = nullptr, std::string* why = nullptr, TriangleGrid* grid_b = nullptr, bool with_signs = false,
                           int sign = kSignParity) {
    TriangleGrid ga, own;
    if (!grid_b && !own.build(b.vertices, b.faces, 0.f, why)) return false;
    TriangleGrid& gb = grid_b ? *grid_b : own;
    if (!ga.build(a.vertices, a.faces, 0.f, why)) return false;
    std::vector<float> ab, ba;
    gb.query(a.vertices, ab, max_dist);
    ga.query(b.vertices, ba, max_dist);
    out.a_to_b = distance_stats(ab), out.b_to_a = distance_stats(ba);
    out.chamfer = 0.5 * (out.a_to_b.mean + out.b_to_a.mean), out.hausdorff = std::max(out.a_to_b.max, out.b_to_a.max);
    if (with_signs) {
        std::vector<unsigned char> in, open;
        std::vector<float> w;
        auto by_winding = [&](TriangleGrid& g, const std::vector<float4>& p) {
            if (sign != kSignWinding) return;
            g.winding(p, w);
            for (size_t i = 0; i < w.size(); ++i) in[i] = w[i] > 0.5f;
        };
        gb.inside(a.vertices, in, open);
        by_winding(gb, a.vertices);
        add_signs(out.a_to_b, ab, in, open);
        ga.inside(b.vertices, in, open);
        by_winding(ga, b.vertices);
        add_signs(out.b_to_a, ba, in, open);
    }
    if (d_ab) d_ab->swap(ab);
    if (d_ba) d_ba->swap(ba);
    return true;
}
// one line, every field at %.9g (sobfu_amd.evaluate.format_result); digits: another precision (17 round-trips a double)
inline std::string format_comparison(const MeshComparison& r, int digits = 9) {
    char line[2048];
    int at = 0;
    const DistanceStats* sides[2] = {&r.a_to_b, &r.b_to_a};
    for (int k = 0; k < 2; ++k) {  // the signed fields follow each side's own, where the comparison has them
        const DistanceStats& x = *sides[k];
        const char* s = k ? "b_to_a" : "a_to_b";
        at += std::snprintf(line + at, sizeof line - (size_t) at, "%s.n=%zu %s.within=%zu %s.mean=%.*g %s.rms=%.*g %s.median=%.*g %s.max=%.*g ", s, x.n, s,
                            x.within, s, digits, x.mean, s, digits, x.rms, s, digits, x.median, s, digits, x.max);
        if (x.has_signs)
            at += std::snprintf(line + at, sizeof line - (size_t) at, "%s.signed_mean=%.*g %s.inside=%zu %s.open=%zu ", s, digits, x.signed_mean, s, x.inside, s,
                                x.open);
    }
    std::snprintf(line + at, sizeof line - (size_t) at, "chamfer=%.*g hausdorff=%.*g", digits, r.chamfer, digits, r.hausdorff);
    return line;
}
// (n, 4) points through a row-major 4 x 4 transform in float32: ((m0 x + m1 y) + m2 z) + t per row, w = 1 (sobfu_amd.fusion.transform_points)
inline void transform_points(std::vector<float4>& points, const float pose[16]) {
    for (float4& p : points) {
        float o[3];
        for (int i = 0; i < 3; ++i) {
            const volatile float xy = pose[4 * i] * p.x + pose[4 * i + 1] * p.y;  // volatile: no contraction into an fma, whatever the flags
            const volatile float xyz = xy + pose[4 * i + 2] * p.z;
            o[i] = xyz + pose[4 * i + 3];
        }
        p = make_float4(o[0], o[1], o[2], 1.f);
    }
}
// Refines the pose that carries a ground-truth mesh into the model's frame (sobfu_amd.evaluate.align_meshes): point-to-plane ICP of the
// model's vertices (the source: a partial surface) against the ground truth (the target: complete; its grid is built once).  pose: in, the
// caller's ground-truth-to-model guess, whose rigid inverse starts the loop; out, the rigid inverse of the result -- the pose to apply to
// the ground truth.  false (+ *why): the ground truth is refused.  A refinement within ICP's basin, not a global registration.
inline bool align_meshes(const std::vector<float4>& model_vertices, const IndexedMesh& gt, float pose[16], Alignment& info, int iters = 30,
                         float max_dist = 0.f, int dof = 6, float eps_rot = 0.f, float eps_trans = 0.f, std::string* why = nullptr) {
    TriangleGrid grid;
    if (!grid.build(gt.vertices, gt.faces, 0.f, why)) return false;
    float start[16];
    sobfu_hip::rigid_inverse(pose, start);
    info = grid.align(model_vertices, start, iters, max_dist, dof, eps_rot, eps_trans);
    sobfu_hip::rigid_inverse(start, pose);
    return true;
}
// one line (sobfu_amd.evaluate.format_alignment): status, iterations, the inliers and rms residual of the last iteration that ran, the pose
inline std::string format_alignment(const Alignment& a, const float pose[16]) {
    char line[1024];
    const size_t rows = a.trace.size() / 4;
    int at = std::snprintf(line, sizeof line, "status=0x%x iterations=%d inliers=%d rms=%.9g pose=", a.status, a.iterations,
                           rows ? (int) a.trace[4 * (rows - 1)] : 0, rows ? (double) a.trace[4 * (rows - 1) + 1] : 0.0);
    for (int k = 0; k < 16; ++k) at += std::snprintf(line + at, sizeof line - (size_t) at, k ? ",%.9g" : "%.9g", (double) pose[k]);
    return line;
}
// what SobFusion::evaluate_canonical is to align first: in, the guess and the loop's settings; out, the refined pose and the report
struct AlignRequest {
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // ground truth -> model
    int iters = 30, dof = 6;
    Alignment info;
};
// ---- area-weighted samples, precision, recall and F-score (sobfu_amd/csrc/mesh_sample_kernels.hip; ops.mesh_sample,
// ops.distance_score, sobfu_amd.evaluate.f_score) -----------------------------------------------------------------------------------------
// the sum of doubles, exactly rounded and so independent of their order: Python's math.fsum (Shewchuk's non-overlapping partials, the
// last step rounded half to even), for finite values whose sum does not overflow
inline double exact_sum(const std::vector<double>& values) {
    std::vector<double> partials;
    for (double x : values) {
        size_t i = 0;
        for (double y : partials) {
            if (std::fabs(x) < std::fabs(y)) std::swap(x, y);
            const volatile double hi = x + y;  // volatile: each step is rounded to double, whatever the flags
            const volatile double back = hi - x;
            const double lo = y - back;
            if (lo != 0.0) partials[i++] = lo;
            x = hi;
        }
        partials.resize(i);
        partials.push_back(x);
    }
    size_t n = partials.size();
    if (n == 0) return 0.0;
    double hi = partials[--n], lo = 0.0;
    while (n > 0) {
        const double x = hi, y = partials[--n];
        const volatile double sum = x + y;
        const volatile double back = sum - x;
        hi = sum, lo = y - back;
        if (lo != 0.0) break;
    }
    if (n > 0 && ((lo < 0.0 && partials[n - 1] < 0.0) || (lo > 0.0 && partials[n - 1] > 0.0))) {
        const double y = lo * 2.0;
        const volatile double x = hi + y;
        const volatile double back = x - hi;
        if (y == back) hi = x;
    }
    return hi;
}
struct MeshSamples {
    std::vector<float4> points;  // (x, y, z, 1), ordered by triangle
    std::vector<int> tri;        // each sample's triangle (on request)
    std::vector<float2> bary;    // the weights of that triangle's second and third corner (on request)
    std::vector<double> areas;   // per triangle (on request)
};
// Points drawn uniformly per unit area at `density` samples per square metre (ops.mesh_sample): triangle t receives floor(area_t density)
// samples plus one more with probability frac(area_t density); the result depends on the mesh, the density and the seed alone, bit for bit.
// false (+ *why): a face index out of range, a non-finite corner, a density that is not finite and >= 0, or more than INT32_MAX samples
inline bool sample_mesh(const IndexedMesh& m, double density, uint64_t seed, MeshSamples& out, bool with_tri = false, bool with_bary = false,
                        bool with_areas = false, std::string* why = nullptr) {
    out = MeshSamples();
    const int nv = (int) m.vertices.size(), nt = (int) (m.faces.size() / 3);
    if (!(std::isfinite(density) && density >= 0.0)) {
        if (why) *why = "the sampling density must be finite and >= 0";
        return false;
    }
    kfusion::cuda::DeviceArray<float4> dv, dp;
    kfusion::cuda::DeviceArray<int> df, dt;
    kfusion::cuda::DeviceArray<float2> db;
    kfusion::cuda::DeviceArray<double> da;
    kfusion::cuda::DeviceArray<unsigned char> ws(sobfu_hip_mesh_sample_workspace_bytes(nt));
    if (nv) dv.upload(m.vertices);
    if (nt) df.upload(m.faces.data(), 3 * (size_t) nt);
    if (with_areas && nt) da.create((size_t) nt);
    long long total = 0;
    const float* vp = nv ? (const float*) dv.ptr() : nullptr;
    const int* fp   = nt ? df.ptr() : nullptr;
    const int rc = sobfu_hip_mesh_sample_count(vp, nv, fp, nt, density, seed, ws.ptr(), ws.sizeBytes(), with_areas && nt ? da.ptr() : nullptr, &total, nullptr);
    if (rc == SOBFU_E_BADARG || rc == SOBFU_E_UNSUPPORTED) {
        if (why) *why = rc == SOBFU_E_BADARG ? "the mesh has a face index out of range or a non-finite corner" : "more than INT32_MAX samples (" + std::to_string(total) + ")";
        return false;
    }
    sobfuSafeCall(rc);
    if (with_areas && nt) da.download(out.areas);
    const size_t n = (size_t) total;
    if (n) {
        dp.create(n);
        if (with_tri) dt.create(n);
        if (with_bary) db.create(n);
        sobfuSafeCall(sobfu_hip_mesh_sample_generate(vp, nv, fp, nt, seed, ws.ptr(), ws.sizeBytes(), (float*) dp.ptr(), with_tri ? dt.ptr() : nullptr,
                                                     with_bary ? (float*) db.ptr() : nullptr, (int) n, nullptr));
        dp.download(out.points);
        if (with_tri) dt.download(out.tri);
        if (with_bary) db.download(out.bary);
    }
    return true;
}
// the mesh's area: exact_sum of the triangles' fp64 areas (the denominator of "n samples": density = n / area)
inline bool mesh_area(const IndexedMesh& m, double& area, std::string* why = nullptr) {
    MeshSamples s;
    if (!sample_mesh(m, 0.0, 0, s, false, false, true, why)) return false;
    area = exact_sum(s.areas);
    return true;
}
// within[k] = how many distances are finite and <= thresholds[k] (1 to 16 of them, any order); finite = how many are finite at all
inline void distance_score(const std::vector<float>& dist, const std::vector<float>& thresholds, std::vector<long long>& within, long long& finite) {
    if (thresholds.empty() || thresholds.size() > 16) kfusion::cuda::error("distance_score: 1 to 16 thresholds", __FILE__, __LINE__);
    kfusion::cuda::DeviceArray<float> dd;
    kfusion::cuda::DeviceArray<long long> dc(thresholds.size() + 1);
    if (!dist.empty()) dd.upload(dist);
    sobfuSafeCall(sobfu_hip_distance_score(dist.empty() ? nullptr : dd.ptr(), (int) dist.size(), thresholds.data(), (int) thresholds.size(), dc.ptr(), nullptr));
    dc.download(within);
    finite = within.back();
    within.pop_back();
}
// what f_score is to do: the thresholds (metres); density > 0: samples per square metre, else `samples` over the larger of the two areas;
// mesh a draws with `seed`, mesh b with seed + 1
struct ScoreRequest {
    std::vector<float> thresholds;
    double density    = 0.0;
    long long samples = 200000;
    uint64_t seed     = 0;
};
struct MeshScore {
    std::vector<float> thresholds;
    std::vector<double> precision, recall, f;  // one entry per threshold; f = 2 P R / (P + R), 0 when P + R = 0
    size_t a_samples = 0, b_samples = 0;
    DistanceStats a_to_b, b_to_a;  // of the sampled distances
    double chamfer = 0, hausdorff = 0;
};
// sobfu_amd.evaluate.f_score: a = the model, b = the ground truth, both sampled at one density; each sample set is sent to the other mesh's
// surface and scored.  The denominators are all the samples: one farther than max_dist (> 0) has no match and is a miss.  false (+ *why):
// a mesh is refused.  grid_b (optional): a grid already built over b
inline bool f_score(const IndexedMesh& a, const IndexedMesh& b, const ScoreRequest& request, float max_dist, MeshScore& out, std::string* why = nullptr,
                    TriangleGrid* grid_b = nullptr) {
    out = MeshScore();
    out.thresholds = request.thresholds;
    TriangleGrid ga, own;
    if (!grid_b && !own.build(b.vertices, b.faces, 0.f, why)) return false;
    TriangleGrid& gb = grid_b ? *grid_b : own;
    if (!ga.build(a.vertices, a.faces, 0.f, why)) return false;
    double density = request.density;
    if (!(density > 0.0)) {
        double area_a = 0, area_b = 0;
        if (!mesh_area(a, area_a, why) || !mesh_area(b, area_b, why)) return false;
        const double larger = std::max(area_a, area_b);
        density = larger > 0.0 ? (double) request.samples / larger : 0.0;
    }
    MeshSamples sa, sb;
    if (!sample_mesh(a, density, request.seed, sa, false, false, false, why) || !sample_mesh(b, density, request.seed + 1, sb, false, false, false, why)) return false;
    std::vector<float> ab, ba;
    gb.query(sa.points, ab, max_dist);
    ga.query(sb.points, ba, max_dist);
    std::vector<long long> wa, wb;
    long long finite = 0;
    distance_score(ab, request.thresholds, wa, finite);
    distance_score(ba, request.thresholds, wb, finite);
    out.a_samples = sa.points.size(), out.b_samples = sb.points.size();
    for (size_t k = 0; k < request.thresholds.size(); ++k) {
        const double p = out.a_samples ? (double) wa[k] / (double) out.a_samples : 0.0, r = out.b_samples ? (double) wb[k] / (double) out.b_samples : 0.0;
        out.precision.push_back(p), out.recall.push_back(r), out.f.push_back(p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0);
    }
    out.a_to_b = distance_stats(ab), out.b_to_a = distance_stats(ba);
    out.chamfer = 0.5 * (out.a_to_b.mean + out.b_to_a.mean), out.hausdorff = std::max(out.a_to_b.max, out.b_to_a.max);
    return true;
}
// one line (sobfu_amd.evaluate.format_f_score): the two sample counts, tau, precision, recall and f per threshold, then format_comparison's
// fields; every float at %.9g
inline std::string format_f_score(const MeshScore& r) {
    char part[256];
    std::snprintf(part, sizeof part, "a_samples=%zu b_samples=%zu ", r.a_samples, r.b_samples);
    std::string line = part;
    for (size_t k = 0; k < r.thresholds.size(); ++k) {
        std::snprintf(part, sizeof part, "tau=%.9g precision=%.9g recall=%.9g f=%.9g ", (double) r.thresholds[k], r.precision[k], r.recall[k], r.f[k]);
        line += part;
    }
    MeshComparison c;
    c.a_to_b = r.a_to_b, c.b_to_a = r.b_to_a, c.chamfer = r.chamfer, c.hausdorff = r.hausdorff;
    return line + format_comparison(c);
}
// ---- mesh_to_tsdf: a closed mesh as the full 3-D signed TSDF of a volume (sobfu_amd.mesh_voxelise.mesh_to_tsdf) ---------------------------
// the pose of the meshes the project writes and evaluates against, mesh frame -> camera frame: (x, -y, -z)
inline cv::Affine3f mesh_frame() {
    cv::Affine3f a = cv::Affine3f::Identity();
    a.R[4] = a.R[8] = -1.f;
    return a;
}
// mesh.vertices in the mesh frame -> the volume's frame: mesh -> camera by mesh2cam, camera -> volume by the inverse of vol2cam (a voxel
// centre v is seen at R v + t), composed in double and applied once per vertex in double
inline void mesh_to_volume_frame(std::vector<float4>& vertices, const cv::Affine3f& mesh2cam, const cv::Affine3f& vol2cam) {
    double M[9], m[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            M[3 * i + j] = 0;
            for (int k = 0; k < 3; ++k) M[3 * i + j] += (double) vol2cam.R[3 * k + i] * (double) mesh2cam.R[3 * k + j];
        }
        m[i] = 0;
        for (int k = 0; k < 3; ++k) m[i] += (double) vol2cam.R[3 * k + i] * ((double) mesh2cam.t[k] - (double) vol2cam.t[k]);
    }
    for (float4& v : vertices) {
        const double x = v.x, y = v.y, z = v.z;
        v = make_float4((float) (M[0] * x + M[1] * y + M[2] * z + m[0]), (float) (M[3] * x + M[4] * y + M[5] * z + m[1]),
                        (float) (M[6] * x + M[7] * y + M[8] * z + m[2]), 1.f);
    }
}
// Fills `vol` (its dims, voxel size, truncation distance and eta) with the mesh: the vertices are transformed once and the triangle grid is
// built with a cell edge of `cell` (0: four voxels, half a brick -- profiles/mesh_voxelise.md).  *open_rows: the rows
// that cross the mesh an odd number of times, 0 for a closed mesh.  false (+ *why): the mesh is refused (TriangleGrid::build).  sign: MeshSign
inline bool mesh_to_tsdf(const IndexedMesh& mesh, const cv::Affine3f& mesh2cam, const cv::Affine3f& vol2cam, kfusion::cuda::TsdfVolume& vol, int* open_rows,
                         std::string* why = nullptr, float cell = 0.f, int mode = SOBFU_MESH_DISTANCE_AUTO, int sign = kSignParity) {
    std::vector<float4> v = mesh.vertices;
    mesh_to_volume_frame(v, mesh2cam, vol2cam);
    TriangleGrid grid;
    const cv::Vec3i d  = vol.getDims();
    const cv::Vec3f s  = vol.getVoxelSize();
    if (!grid.build(v, mesh.faces, cell > 0.f ? cell : 4.f * std::max(s[0], std::max(s[1], s[2])), why)) return false;
    const int dims[3]  = {d[0], d[1], d[2]};
    const float vs[3]  = {s[0], s[1], s[2]};
    const int open     = grid.voxelise(vol.data().ptr<float>(), dims, vs, vol.getTruncDist(), vol.getEta(), mode, sign);
    if (open_rows) *open_rows = open;
    return true;
}

// Vertex colours by error: a fixed ramp from blue (0) to red (max_dist and beyond), r = round(255 t), b = round(255 (1 - t)), g = 0 with
// t = clamp(d / max_dist, 0, 1) in double; grey (128, 128, 128) where there is no match
inline void error_colours(const std::vector<float>& dist, float max_dist, std::vector<kfusion::RGB>& colours) {
    colours.resize(dist.size());
    for (size_t i = 0; i < dist.size(); ++i) {
        kfusion::RGB c;
        c.bgra = 0;
        if (!std::isfinite(dist[i]) || !(max_dist > 0.f)) {
            c.r = c.g = c.b = 128;
        } else {
            const double t = std::min(1.0, std::max(0.0, (double) dist[i] / (double) max_dist));
            c.r = (unsigned char) (255.0 * t + 0.5), c.g = 0, c.b = (unsigned char) (255.0 * (1.0 - t) + 0.5);
        }
        colours[i] = c;
    }
}

}  // namespace sobfu_amd
