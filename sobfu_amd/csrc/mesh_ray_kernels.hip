// Rays against an indexed triangle mesh on gfx950: for every ray the nearest triangle it meets, and a pinhole camera that turns a mesh
// into depth, points, normals, colour and triangle-index images.  The reference has no such step; the rules are this
// project's, and tests/mesh_ray_reference.py restates them (the ray-triangle rule operation by operation: sobfu_mesh_ray.hpp).  The
// kernels only read the grid that sobfu_hip_mesh_grid_build made for the distance query; the grid's view, the mesh record, the corner and
// staging loads, the mode and the check of the leading arguments are the mesh side's shared ones (sobfu_mesh.hpp).
//
//   answer   per ray: min over all triangles of t (ray_triangle, t_min < t <= t_max), the LOWEST triangle index attaining it, that
//            triangle's barycentrics and side.  A miss: (+Inf, -1, (0, 0), 0).  The answer does not depend on the path that finds it: grid
//            and brute force agree bit for bit, run after run, whatever the cells and the order of the references inside them.
//   walk     one lane per ray.  margin = kRayMargin L, L = the largest coordinate magnitude of the box and the ray's origin: an absolute
//            bound on the fp32 error of one hit, |d| t measured <= 9.6e-7 L (tests/test_mesh_ray_cpu.py); mt = margin / |d[kz]| is the
//            same in units of t.  The ray is clipped by slabs to the box grown by margin (an axis with d = 0 only asks whether o lies
//            between its two planes).  It then steps cell by cell along its major axis kz, the DDA's driving axis: layer k is entered
//            at ta = (plane_k - o[kz]) / d[kz] and left at tb.  Over [ta - mt, tb + mt] the ray spans an interval on each minor axis
//            (o + t d at the two ends, d = 0: o); grown by margin, it gives the cells of the layer to visit -- one or two per axis
//            (|d[minor]| <= |d[kz]|), three where the ray passes within margin of a lattice edge or corner, so the order in which fp32
//            would cross two planes that it reaches together never matters: the cells on all sides are visited.  Every triangle a
//            visited cell references is tested against the whole ray; no hit is accepted or refused by where it lies.
//   stop     before layer k when best_t + mt <= ta: a triangle not yet seen is referenced from layers >= k only, so its hit (which
//            never leaves the triangle's extent along kz) has t >= ta up to rounding and can neither beat nor tie the best one.
//   brute    a 256-lane workgroup per 256 rays, the triangles staged through LDS 256 at a time (48 B each), every lane testing the same
//            triangle (a broadcast LDS read) in ascending index order.  The whole call for mode brute and for tiny meshes in mode auto.
//   camera   a 16 x 16 workgroup, each of its four waves an 8 x 8 pixel tile: the lanes of a wave walk neighbouring cells.  Pixel (u, v)
//            casts ((u - cx) / fx, (v - cy) / fy, 1) =: (dx, dy, 1) from the camera of (R, t), mesh frame -> camera frame: in the mesh
//            frame o = -R^T t (fp64 on the host, rounded once), d_i = (R_0i dx + R_1i dy) + R_2i.  d is not normalised: t is the depth z.
//              depth    rint(1000 z) as uint16 when it lies in [1, 65535], else 0
//              points   (z dx, z dy, z, 0)
//              normals  with w = (1 - u) - v: n = (w n_a + u n_b) + v n_c of the vertex normals, or the face's (b - a) x (c - a); negated
//                       when n . d > 0; rotated, c_i = (R_i0 n_x + R_i1 n_y) + R_i2 n_z; divided by its length sqrt((c_x^2 + c_y^2) +
//                       c_z^2) when that is > 0 (else 0); the fourth component is 1
//              colour   per channel b, g, r: floor(((w c_a + u c_b) + v c_c) + 0.5) clamped to [0, 255]; alpha 255
//              tri      the triangle's index
//            a miss is 0 everywhere and tri = -1.
#include "sobfu_hip.h"
#include "sobfu_frame.hpp"
#include "sobfu_mesh.hpp"
#include "sobfu_mesh_ray.hpp"

using namespace sobfu_hip;

namespace {

constexpr float kRayMargin = 1e-4f;

struct Best {
    float t;
    int tri;
    float u, v;
    int side;
};

SOBFU_DEV Best no_hit() { return Best{INFINITY, -1, 0.f, 0.f, 0}; }
SOBFU_DEV float pickf(float x, float y, float z, int k) { return k == 0 ? x : k == 1 ? y : z; }
SOBFU_DEV int picki(int x, int y, int z, int k) { return k == 0 ? x : k == 1 ? y : z; }

SOBFU_DEV void visit_cell(const Grid& g, const Mesh& m, const Ray& r, float t_min, float t_max, int cell, Best& best) {
    const int end = g.start[cell + 1];
    for (int k = g.start[cell]; k < end; ++k) {
        const int t = g.refs[k];
        const Corners v = corners_of(m, t);
        const RayHit h  = ray_triangle(r, p3(v.a), p3(v.b), p3(v.c), t_min, t_max);
        if (h.t < best.t || (h.t == best.t && t < best.tri)) best = Best{h.t, t, h.u, h.v, h.side};
    }
}

// [t0, t1] &= the parameters at which o + t d lies in [lo, hi]; false: never (d == 0: all or nothing)
SOBFU_DEV bool clip_axis(float o, float d, float lo, float hi, float& t0, float& t1) {
    if (d == 0.f) return o >= lo && o <= hi;
    const float ta = (lo - o) / d, tb = (hi - o) / d;
    t0 = fmaxf(t0, fminf(ta, tb)), t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}

// the grid walk of one ray.  Every cell index comes out of cell_of, which clamps into the grid, and the layers are counted: whatever the
// floating-point values, the walk stays inside the workspace and ends.
SOBFU_DEV Best walk_grid(const Grid& g, const Mesh& m, float box_l, const P3& o, const P3& d, float t_min, float t_max) {
    Best best = no_hit();
    const Ray r = ray_setup(o, d);
    if (!r.valid) return best;
    const float L      = fmaxf(fmaxf(box_l, fabsf(o.x)), fmaxf(fabsf(o.y), fabsf(o.z)));
    const float margin = kRayMargin * L, mt = margin * fabsf(r.Sz);
    float t0 = t_min, t1 = t_max;
    if (!clip_axis(o.x, d.x, g.ox - margin, (g.ox + (float) g.dx * g.h) + margin, t0, t1)) return best;
    if (!clip_axis(o.y, d.y, g.oy - margin, (g.oy + (float) g.dy * g.h) + margin, t0, t1)) return best;
    if (!clip_axis(o.z, d.z, g.oz - margin, (g.oz + (float) g.dz * g.h) + margin, t0, t1)) return best;
    if (!(t0 <= t1)) return best;

    const int kz = r.kz, k1 = kz == 2 ? 0 : kz + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const float oz = mr_pick(o, kz), dz = mr_pick(d, kz), o1 = mr_pick(o, k1), d1 = mr_pick(d, k1), o2 = mr_pick(o, k2), d2 = mr_pick(d, k2);
    const float gz = pickf(g.ox, g.oy, g.oz, kz), g1 = pickf(g.ox, g.oy, g.oz, k1), g2 = pickf(g.ox, g.oy, g.oz, k2);
    const int nz = picki(g.dx, g.dy, g.dz, kz), n1 = picki(g.dx, g.dy, g.dz, k1), n2 = picki(g.dx, g.dy, g.dz, k2);
    const int sz = picki(1, g.dx, g.dx * g.dy, kz), s1 = picki(1, g.dx, g.dx * g.dy, k1), s2 = picki(1, g.dx, g.dx * g.dy, k2);
    const int step = dz > 0.f ? 1 : -1;
    const float fs = (float) step;
    const int first = cell_of((oz + t0 * dz) - fs * margin, gz, g.h, nz), last = cell_of((oz + t1 * dz) + fs * margin, gz, g.h, nz);
    const int count = max((last - first) * step, 0);
    for (int i = 0; i <= count; ++i) {
        const int k    = first + i * step;
        const float ta = ((gz + (float) (step > 0 ? k : k + 1) * g.h) - oz) * r.Sz, tb = ((gz + (float) (step > 0 ? k + 1 : k) * g.h) - oz) * r.Sz;
        if (i > 0 && best.t + mt <= ta) break;
        const float a = (i == 0 ? t0 : fmaxf(ta, t0)) - mt, b = (i == count ? t1 : fminf(tb, t1)) + mt;
        const float xa = d1 == 0.f ? o1 : o1 + a * d1, xb = d1 == 0.f ? o1 : o1 + b * d1;
        const float ya = d2 == 0.f ? o2 : o2 + a * d2, yb = d2 == 0.f ? o2 : o2 + b * d2;
        const int x0 = cell_of(fminf(xa, xb) - margin, g1, g.h, n1), x1 = cell_of(fmaxf(xa, xb) + margin, g1, g.h, n1);
        const int y0 = cell_of(fminf(ya, yb) - margin, g2, g.h, n2), y1 = cell_of(fmaxf(ya, yb) + margin, g2, g.h, n2);
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) visit_cell(g, m, r, t_min, t_max, k * sz + x * s1 + y * s2, best);
    }
    return best;
}

struct RayArgs {
    Mesh mesh;
    const float4* origins;
    const float4* dirs;
    int n;
    float t_min, t_max;  // t_max +Inf: unlimited
    float box_l;         // the largest coordinate magnitude of the grid's box
    float* t;
    int* tri;
    float2* bary;       // may be null
    signed char* side;  // may be null
};

SOBFU_DEV void write_answer(const RayArgs& a, int i, const Best& b) {
    a.t[i]   = b.t;
    a.tri[i] = b.tri;
    if (a.bary) a.bary[i] = make_float2(b.u, b.v);
    if (a.side) a.side[i] = (signed char) b.side;
}

__global__ void __launch_bounds__(256) ray_grid_kernel(Grid g, RayArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    Best best = no_hit();
    if (g.hdr[kHdrBuilt] == 1) best = walk_grid(g, a.mesh, a.box_l, p3(a.origins[i]), p3(a.dirs[i]), a.t_min, a.t_max);
    write_answer(a, i, best);
}

__global__ void __launch_bounds__(256) ray_brute_kernel(const int* __restrict__ hdr, RayArgs a) {
    __shared__ float4 sa[256], sb[256], sc[256];
    const int i       = blockIdx.x * 256 + threadIdx.x;
    const bool active = i < a.n;
    const bool built  = hdr[kHdrBuilt] == 1;
    const int j       = active ? i : a.n - 1;
    const Ray r       = ray_setup(p3(a.origins[j]), p3(a.dirs[j]));
    Best best = no_hit();
    for (int t0 = 0; built && t0 < a.mesh.n_triangles; t0 += 256) {
        __syncthreads();  // the previous chunk has been read
        stage_triangles(a.mesh, t0, sa, sb, sc);
        __syncthreads();
        const int m = min(256, a.mesh.n_triangles - t0);
        for (int k = 0; r.valid && k < m; ++k) {
            const RayHit h = ray_triangle(r, p3(sa[k]), p3(sb[k]), p3(sc[k]), a.t_min, a.t_max);
            if (h.t < best.t) best = Best{h.t, t0 + k, h.u, h.v, h.side};  // ascending index: the first minimum is the lowest
        }
    }
    if (active) write_answer(a, i, best);
}

struct RenderArgs {
    Mesh mesh;
    const float4* vertex_normals;  // may be null: the face normal
    const uchar4* vertex_colours;  // may be null
    float R[9];                    // mesh frame -> camera frame
    float o[3];                    // -R^T t: the camera centre in the mesh frame
    float fx, fy, cx, cy;
    int rows, cols;
    float z_min, z_max;
    float box_l;
    unsigned short* depth;  // every output may be null
    int depth_step;
    float4* points;
    int points_step;
    float4* normals;
    int normals_step;
    uchar4* colour;
    int colour_step;
    int* tri;
    int tri_step;
};

SOBFU_DEV float mix3(float w, float u, float v, float a, float b, float c) { return (w * a + u * b) + v * c; }

__global__ void __launch_bounds__(256) mesh_render_kernel(Grid g, RenderArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= a.cols || v >= a.rows) return;
    const float dx = ((float) u - a.cx) / a.fx, dy = ((float) v - a.cy) / a.fy;
    const P3 o{a.o[0], a.o[1], a.o[2]};
    const P3 d{(a.R[0] * dx + a.R[3] * dy) + a.R[6], (a.R[1] * dx + a.R[4] * dy) + a.R[7], (a.R[2] * dx + a.R[5] * dy) + a.R[8]};
    Best best = no_hit();
    if (g.hdr[kHdrBuilt] == 1) best = walk_grid(g, a.mesh, a.box_l, o, d, a.z_min, a.z_max);
    const bool hit = best.tri >= 0;
    const float z  = best.t;
    if (a.depth) {
        const float mm = rintf(1000.f * z);
        row_ptr(a.depth, a.depth_step, v)[u] = hit && mm >= 1.f && mm <= 65535.f ? (unsigned short) mm : (unsigned short) 0;
    }
    if (a.tri) row_ptr(a.tri, a.tri_step, v)[u] = best.tri;
    if (a.points) row_ptr(a.points, a.points_step, v)[u] = hit ? make_float4(z * dx, z * dy, z, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (!a.normals && !a.colour) return;
    int3 f = make_int3(0, 0, 0);
    if (hit) f = face_of(a.mesh, best.tri);
    const float bu = best.u, bv = best.v, bw = (1.f - bu) - bv;
    if (a.normals) {
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hit) {
            float nx, ny, nz;
            if (a.vertex_normals) {
                const float4 na = a.vertex_normals[f.x], nb = a.vertex_normals[f.y], nc = a.vertex_normals[f.z];
                nx = mix3(bw, bu, bv, na.x, nb.x, nc.x), ny = mix3(bw, bu, bv, na.y, nb.y, nc.y), nz = mix3(bw, bu, bv, na.z, nb.z, nc.z);
            } else {
                const Corners t = corners_of(a.mesh, f);
                const P3 pa = p3(t.a), e1 = md_sub(p3(t.b), pa), e2 = md_sub(p3(t.c), pa);
                nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
            }
            if ((nx * d.x + ny * d.y) + nz * d.z > 0.f) nx = -nx, ny = -ny, nz = -nz;
            const float cx = (a.R[0] * nx + a.R[1] * ny) + a.R[2] * nz, cy = (a.R[3] * nx + a.R[4] * ny) + a.R[5] * nz;
            const float cz  = (a.R[6] * nx + a.R[7] * ny) + a.R[8] * nz;
            const float len = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
            out = len > 0.f ? make_float4(cx / len, cy / len, cz / len, 1.f) : make_float4(0.f, 0.f, 0.f, 1.f);
        }
        row_ptr(a.normals, a.normals_step, v)[u] = out;
    }
    if (a.colour) {
        uchar4 out = make_uchar4(0, 0, 0, 0);
        if (hit) {
            const uchar4 ca = a.vertex_colours[f.x], cb = a.vertex_colours[f.y], cc = a.vertex_colours[f.z];
            out = make_uchar4(to_byte(mix3(bw, bu, bv, (float) ca.x, (float) cb.x, (float) cc.x)),
                              to_byte(mix3(bw, bu, bv, (float) ca.y, (float) cb.y, (float) cc.y)),
                              to_byte(mix3(bw, bu, bv, (float) ca.z, (float) cb.z, (float) cc.z)), 255);
        }
        row_ptr(a.colour, a.colour_step, v)[u] = out;
    }
}

// a pitched output image that may be absent: room for cols elements of `size` bytes per row, aligned to `to`
bool image_ok(const void* p, int step, int cols, int size, int to) { return !p || ((long long) step >= (long long) cols * size && aligned(p, step, to)); }
float unlimited(float t_max) { return t_max > 0.f ? t_max : INFINITY; }

}  // namespace

extern "C" {

int sobfu_hip_mesh_raycast(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                           const float origin[3], float h, const int dims[3], const float* d_origins, const float* d_dirs, int n, float t_min,
                           float t_max, int mode, float* d_t, int* d_tri, float* d_bary, int8_t* d_side, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_workspace, workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(d_origins && d_dirs && d_t && d_tri && n >= 0 && aligned(d_origins, 0, 16) && aligned(d_dirs, 0, 16) && aligned(d_t, 0, 4) &&
                     aligned(d_tri, 0, 4) && aligned(d_bary, 0, 8));
    SOBFU_CHECK_ARGS(std::isfinite(t_min) && !std::isnan(t_max) && mode_ok(mode));
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    const RayArgs a{tg.mesh, (const float4*) d_origins, (const float4*) d_dirs, n, t_min, unlimited(t_max), tg.box_l, d_t, d_tri, (float2*) d_bary,
                    (signed char*) d_side};
    const dim3 blocks((unsigned) (((long long) n + 255) / 256));
    if (is_brute(mode, n_triangles)) hipLaunchKernelGGL(ray_brute_kernel, blocks, dim3(256), 0, st, (const int*) tg.grid.hdr, a);
    else hipLaunchKernelGGL(ray_grid_kernel, blocks, dim3(256), 0, st, tg.grid, a);
    return (int) hipGetLastError();
}

int sobfu_hip_mesh_render(void* d_workspace, size_t workspace_bytes, const float* d_vertices, int n_vertices, const int* d_faces, int n_triangles,
                          const float origin[3], float h, const int dims[3], const float* d_vertex_normals, const uint8_t* d_vertex_colours,
                          const float R[9], const float t[3], float fx, float fy, float cx, float cy, int rows, int cols, float z_min, float z_max,
                          uint16_t* d_depth, int depth_step, float* d_points, int points_step, float* d_normals, int normals_step, uint8_t* d_colour,
                          int colour_step, int32_t* d_tri, int tri_step, void* stream) {
    MeshTarget tg;
    SOBFU_CHECK_ARGS(mesh_target(d_workspace, workspace_bytes, d_vertices, n_vertices, d_faces, n_triangles, origin, h, dims, 0, &tg));
    SOBFU_CHECK_ARGS(R && t && finite_all(R, 9) && finite_all(t, 3) && intr_ok(fx, fy, cx, cy) && rows >= 1 && cols >= 1);
    SOBFU_CHECK_ARGS(std::isfinite(z_min) && !std::isnan(z_max) && aligned(d_vertex_normals, 0, 16) && aligned(d_vertex_colours, 0, 4));
    SOBFU_CHECK_ARGS(image_ok(d_depth, depth_step, cols, 2, 2) && image_ok(d_points, points_step, cols, 16, 16) &&
                     image_ok(d_normals, normals_step, cols, 16, 16) && image_ok(d_colour, colour_step, cols, 4, 4) &&
                     image_ok(d_tri, tri_step, cols, 4, 4));
    SOBFU_CHECK_ARGS(!d_colour || d_vertex_colours);
    if (!d_depth && !d_points && !d_normals && !d_colour && !d_tri) return 0;
    RenderArgs a{tg.mesh, (const float4*) d_vertex_normals, (const uchar4*) d_vertex_colours, {}, {}, fx, fy, cx, cy, rows, cols, z_min, unlimited(z_max),
                 tg.box_l, d_depth, depth_step, (float4*) d_points, points_step, (float4*) d_normals, normals_step, (uchar4*) d_colour, colour_step, d_tri,
                 tri_step};
    fill_pose(R, t, a.R, nullptr, nullptr);
    for (int i = 0; i < 3; ++i) {
        double o = 0.0;
        for (int j = 0; j < 3; ++j) o -= (double) R[3 * j + i] * (double) t[j];
        a.o[i] = (float) o;
    }
    hipLaunchKernelGGL(mesh_render_kernel, dim3((unsigned) ((cols + 15) / 16), (unsigned) ((rows + 15) / 16)), dim3(256), 0, (hipStream_t) stream, tg.grid, a);
    return (int) hipGetLastError();
}

}  // extern "C"
