"""The per-frame pipeline of the reference's SobFusion::operator() (src/sobfu/sob_fusion.cpp:71-145) on one GPU, through the C ABI:
depth pre-steps -> frame 0: integrate into phi_global | frame n: clear + integrate phi_n, estimate_psi (iterations + 48-sweep
inverse + canonical warp), fuse phi_n o psi into phi_global.  Optional colour frames are fused into colour_global through the TSDF
that is fused in the same frame and psi (sobfu_amd/csrc/colour_kernels.hip).  The Python twin of sobfu::SobFusion in include/sobfu_amd/sobfu.hpp
(what apps/sobfu_headless drives); bench.py times it for the frames/s figures (BASELINE config 5)."""
from __future__ import annotations

import numpy as np

MESH_FRAME = (np.diag([1.0, -1.0, -1.0]).astype(np.float32), np.zeros(3, np.float32))  # mesh_render.MESH_FRAME


def affine_mul(a, b):
    """a o b of two rigid 4 x 4 transforms in float32, in the operation order of cv::Affine3f's stand-in (include/sobfu_amd/sobfu.hpp)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    r = np.eye(4, dtype=np.float32)
    for i in range(3):
        for j in range(3):
            acc = np.float32(0)
            for k in range(3):
                acc = np.float32(acc + a[i, k] * b[k, j])
            r[i, j] = acc
        r[i, 3] = np.float32(np.float32(np.float32(a[i, 0] * b[0, 3]) + np.float32(a[i, 1] * b[1, 3])) + np.float32(a[i, 2] * b[2, 3])) + a[i, 3]
    return r


def affine_inv(a):
    """R^T, -R^T t in float32 (cv::Affine3f::inv of the stand-in)"""
    a = np.asarray(a, np.float32)
    r = np.eye(4, dtype=np.float32)
    r[:3, :3] = a[:3, :3].T
    for i in range(3):
        r[i, 3] = -(np.float32(np.float32(r[i, 0] * a[0, 3]) + np.float32(r[i, 1] * a[1, 3])) + np.float32(r[i, 2] * a[2, 3]))
    return r


def transform_points(points, pose):
    """(n, 4) float32 points through a 4 x 4 transform, in float32: ((m0 x + m1 y) + m2 z) + t per row; w = 1 (the order of
    sobfu_amd::transform_points in include/sobfu_amd/evaluate.hpp)"""
    p, m = np.asarray(points, np.float32), np.asarray(pose, np.float32).reshape(4, 4)
    out = np.ones((len(p), 4), np.float32)
    for i in range(3):
        out[:, i] = ((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3]
    return out


class SobFusion:
    """params: a dict as sobfu_amd.params.read_ini returns (dims, vs, trunc, eta, max_weight, intr, R, t, start_frame, bilateral,
    trunc_depth, max_iter, max_update_norm, s, lam, alpha, w_reg; track_camera and the icp_* settings for camera tracking)."""

    def __init__(self, params, max_iter=None):
        from . import ops

        self.ops, self.P = ops, params
        self.max_iter = int(params["max_iter"] if max_iter is None else max_iter)
        self.frame = 0
        self.phi_global = self.phi_global_psi_inv = self.phi_n = self.phi_n_psi = self.psi = self.psi_inv = self.solver = None
        self.last_report = None
        self.colour_global = None  # (Z, Y, X, 4) uint8 (b, g, r, weight), allocated on the first colour frame
        self.image_shape = None  # (rows, cols) of the depth frames: the camera render() draws with
        self.track = bool(params.get("track_camera", False))
        self.pose = np.eye(4, dtype=np.float32)  # the current frame's camera pose (camera -> frame 0's camera); identity unless tracking
        self.poses = []  # one 4 x 4 float32 pose per frame
        self.icp = None
        self._prev = None  # the previous frame's (points, normals) pyramid

    def vol2cam(self):
        """(R, t) of the volume in the current camera frame: pose^-1 * volume_pose (the volume pose itself without tracking)"""
        P = self.P
        if not self.track:
            return P["R"], P["t"]
        vp = np.eye(4, dtype=np.float32)
        vp[:3, :3], vp[:3, 3] = P["R"], P["t"]
        m = affine_mul(affine_inv(self.pose), vp)
        return m[:3, :3], m[:3, 3]

    def _track(self, d):
        """camera tracking of frame n against frame n-1 (the rules of SobFusion::track in include/sobfu_amd/sobfu.hpp)"""
        ops, P = self.ops, self.P
        if self.icp is None:
            self.icp = ops.ICP(P["icp_dist_thres"], P["icp_angle_thres"], P["icp_iter_num"])
        levels = max(1, self.icp.used_levels())
        depth = [d]
        for _ in range(1, levels):
            depth.append(ops.depth_pyramid(depth[-1], P["bilateral"][2]))
        curr = [ops.point_normals(x, tuple(float(np.float32(np.float32(v) / np.float32(1 << l))) for v in P["intr"])) for l, x in enumerate(depth)]
        prev, self._prev = self._prev, curr
        if prev is None:
            return
        ok, aff = self.icp.estimate(P["intr"], [c[0] for c in curr], [c[1] for c in curr], [p[0] for p in prev], [p[1] for p in prev])
        if ok:
            self.pose = affine_mul(self.pose, aff)
        else:
            level, it = self.icp.failure()
            print(f"camera tracking failed on frame {self.frame} (level {level}, iteration {it}): keeping the previous pose")

    def __call__(self, depth_u16, colour=None):
        """colour (optional): a (rows, cols, 4) uint8 BGRA frame registered to depth_u16, of its size; None = the geometry-only path"""
        ops, P = self.ops, self.P
        if colour is not None and tuple(colour.shape) != tuple(depth_u16.shape) + (4,):
            raise ValueError(f"colour frame {tuple(colour.shape)} does not match the depth frame {tuple(depth_u16.shape)}")
        self.image_shape = tuple(depth_u16.shape)
        vs = tuple(float(v) for v in P["vs"])
        ks, ss, sd = P["bilateral"]
        d = ops.bilateral_filter(depth_u16, ks, ss, sd)                                       # sob_fusion.cpp:78
        ops.truncate_depth(d, P["trunc_depth"])                                               # :85
        dists = ops.compute_dists(d, P["intr"])                                               # :91
        if self.track:
            self._track(d)
        self.poses.append(self.pose.copy())
        R, t = self.vol2cam()

        def integrate(vol, fresh):
            if not fresh:
                ops.clear_volume(vol)                                                         # :129
            ops.integrate_depth(dists, vol, vs, P["trunc"], P["eta"], R, t, P["intr"])        # :112, :130

        return self._frame(integrate, colour)

    def integrate_mesh(self, vertices, faces, pose=MESH_FRAME, allow_open=False, sign="parity"):
        """A frame whose phi_n is the closed mesh itself, voxelised (sobfu_amd.mesh_voxelise.mesh_to_tsdf: exact signed distances on both
        sides of the surface, no sensor model) in place of bilateral -> truncate -> dists -> integrate_depth; everything after that is
        __call__'s.  vertices (V, 3 | 4), faces (F, 3) in the mesh frame; pose = (R, t): mesh frame -> camera frame (MESH_FRAME: the
        meshes the project writes).  Camera tracking does not apply: the pose is appended unchanged.  A mesh that is not closed (rows
        that cross it an odd number of times) raises ValueError before anything is fused, unless allow_open.  sign="winding": inside
        iff the mesh's generalised winding number exceeds 1 / 2, which is defined for open meshes too: none is refused."""
        from .mesh_voxelise import mesh_to_tsdf

        ops, P = self.ops, self.P
        R, t = self.vol2cam()
        target = ops.new_volume(P["dims"]) if self.frame == 0 else self.phi_n
        _, open_rows = mesh_to_tsdf(vertices, faces, dict(P, R=R, t=t), pose=pose, out=target, sign=sign)
        if sign != "winding" and int(open_rows) > 0 and not allow_open:
            raise ValueError(f"the mesh is not closed: {int(open_rows)} rows of the volume cross it an odd number of times")
        self.poses.append(self.pose.copy())

        def integrate(vol, fresh):
            if vol is not target:
                vol.copy_(target)

        return self._frame(integrate, None)

    def _frame(self, integrate, colour):
        """frame 0: integrate(phi_global) | frame n: integrate(phi_n), estimate_psi, fuse (sob_fusion.cpp:93-145).  integrate(vol, fresh)
        fills a volume with the frame's TSDF; fresh: newly allocated, all zero"""
        ops, P = self.ops, self.P
        dims = P["dims"]
        if self.frame == 0:                                                                   # :93-123
            self.phi_global = ops.new_volume(dims)
            integrate(self.phi_global, True)
            self._colour(colour, self.phi_global, None)
            self.phi_global_psi_inv, self.phi_n, self.phi_n_psi = ops.new_volume(dims), ops.new_volume(dims), ops.new_volume(dims)
            self.psi, self.psi_inv = ops.new_field(dims), ops.new_field(dims)
            ops.init_identity(self.psi)
            ops.init_identity(self.psi_inv)
            self.solver = ops.Solver(dims, max_iter=self.max_iter, alpha=P["alpha"], w_reg=P["w_reg"], s=P["s"], lam=P["lam"],
                                     max_update_norm=P["max_update_norm"])
            self.frame += 1
            return None
        integrate(self.phi_n, False)
        if self.frame < P["start_frame"]:                                                     # :136-139
            self._colour(colour, self.phi_n, None)
            ops.integrate_fuse(self.phi_global, self.phi_n, P["max_weight"])
        else:
            self.last_report = self.solver.estimate_psi(self.phi_global, self.phi_global_psi_inv, self.phi_n, self.phi_n_psi, self.psi,
                                                        self.psi_inv)                        # :141
            self._colour(colour, self.phi_n_psi, self.psi)
            ops.integrate_fuse(self.phi_global, self.phi_n_psi, P["max_weight"])              # :142
        self.frame += 1
        return self.last_report

    def _colour(self, colour, tsdf, psi):
        if colour is None:
            return
        P = self.P
        if self.colour_global is None:
            self.colour_global = self.ops.new_colour_volume(P["dims"])
        R, t = self.vol2cam()
        self.ops.integrate_colour(colour, tsdf, psi, self.colour_global, P["vs"], R, t, P["intr"],
                                  self.ops.colour_weight_cap(P["max_weight"]))

    def warp_stats(self, band=1.0, **kw):
        """Diagnostics of the last solved deformation (ops.warp_stats): det J, folds and displacement over the voxels of
        phi_global within `band` (units of the truncation distance) of the surface, and the residual of psi o psi_inv over those of
        phi_global o psi_inv; lengths in metres.  kw: edges, res_tol, volumes.  None before the first solve."""
        if self.last_report is None:
            return None
        return self.ops.warp_stats(self.psi, self.psi_inv, mask=self.phi_global, mask_inv=self.phi_global_psi_inv,
                                   voxel_size=tuple(float(v) for v in self.P["vs"]), band=band, **kw)

    def colour_global_psi_inv(self):
        """the canonical colour warped to live, colour_global o psi_inv (computed on request); None without colour"""
        import torch

        if self.colour_global is None:
            return None
        return self.ops.apply_colour(self.colour_global, torch.empty_like(self.colour_global), self.psi_inv)

    def render(self, which="phi_global", light=(0.0, 0.0, 0.0), colour=True):
        """Raycast + shade one of the volumes ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi") from the sequence's own depth
        camera (the current tracked pose -- identity without tracking -- and the intrinsics its frames are integrated with) -> (rows, cols, 4) uint8 BGRA image; light in the camera frame.
        With colour frames fused and colour=True, the canonical volumes phi_global and phi_global_psi_inv are shaded in colour
        (colour_global, colour_global o psi_inv); the live volumes are always grey."""
        if which not in ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi"):
            raise ValueError(f"unknown volume {which!r}")
        vol = getattr(self, which)
        if vol is None:
            raise RuntimeError(f"{which} does not exist before the first frame")
        P, (rows, cols) = self.P, self.image_shape
        R, t = self.vol2cam()
        pts, nrm = self.ops.raycast(vol, P["vs"], P["trunc"], R, t, P["intr"], rows=rows, cols=cols)
        if colour and self.colour_global is not None and which in ("phi_global", "phi_global_psi_inv"):
            col = self.colour_global if which == "phi_global" else self.colour_global_psi_inv()
            return self.ops.render_colour(pts, nrm, self.ops.sample_colour(col, P["vs"], R, t, pts, nrm), light)
        return self.ops.render_image(pts, nrm, light)

    def render_model_depth(self, sensor=None, seed=0):
        """The fused model phi_global seen from the current pose (render's camera), as a (rows, cols) int16 tensor holding the bits of
        uint16 millimetres: ops.raycast, then ops.depth_sensor -- what the depth sensor `sensor` (an ops.SensorModel; None: the ideal one,
        rint(1000 z) of every hit) would report of the reconstruction.  The frame number of the draws is the number of frames fused."""
        if self.phi_global is None or self.image_shape is None:
            raise RuntimeError("there is no model and no depth camera before the first depth frame")
        P, (rows, cols) = self.P, self.image_shape
        R, t = self.vol2cam()
        pts, nrm = self.ops.raycast(self.phi_global, P["vs"], P["trunc"], R, t, P["intr"], rows=rows, cols=cols)
        return self.ops.depth_sensor(pts, nrm, self.ops.SensorModel.ideal() if sensor is None else sensor, seed, self.frame)

    def warp_to_live(self, vertices, normals=None):
        """Carries marching-cubes vertices of the canonical model (ops.marching_cubes_indexed of phi_global at the volume pose), and their
        normals when given, to the live frame through the current psi: vertex i stays the same surface point from frame to frame.
        -> vertices, or (vertices, normals), new tensors.  Before the first solved frame (psi is still the identity) the input is returned."""
        if self.last_report is None:
            return vertices if normals is None else (vertices, normals)
        P = self.P
        return self.ops.warp_points(self.psi, P["vs"], P["R"], P["t"], vertices, normals, mc_vertices=True)

    def fit(self, vertices):
        """How well marching-cubes vertices (at the volume pose) fit the current frame: phi_n sampled at them, in metres (TSDF x truncation
        distance: the TSDF's own projective metric, not a Euclidean point-to-surface distance), over the samples whose eight corners
        were all observed -> dict(valid, mean_abs, rms, max)."""
        if self.phi_n is None:
            raise RuntimeError("phi_n does not exist before the second frame")
        P = self.P
        d = self.ops.sample_tsdf(self.phi_n, P["vs"], P["R"], P["t"], vertices, mc_vertices=True).cpu().numpy().astype(np.float64)
        d = np.abs(d[~np.isnan(d)]) * float(P["trunc"])
        if d.size == 0:
            return dict(valid=0, mean_abs=0.0, rms=0.0, max=0.0)
        return dict(valid=int(d.size), mean_abs=float(d.mean()), rms=float(np.sqrt((d * d).mean())), max=float(d.max()))

    def evaluate(self, gt_vertices, gt_faces, which="canonical", max_dist=None, pose=None, return_meshes=False, align=False, align_dof=6,
                 align_iters=30, signed=False, f_score=None):
        """The reconstruction against a ground-truth mesh (vertices (V, 4), faces (F, 3)) in the frame of the meshes the app writes
        (marching-cubes vertices, (x, -y, -z)): exact vertex-to-surface distances both ways (sobfu_amd.evaluate.compare_meshes; a = the
        model, b = the ground truth), in metres.  which: "canonical" meshes phi_global (ops.marching_cubes_indexed at the volume pose),
        "live" carries that mesh through psi (warp_to_live).  pose: a 4 x 4 transform applied to the ground truth first (float32, row by
        row: (r0 x + r1 y) + r2 z + t).  Reads the volumes only.  return_meshes: -> (dict, model vertices, model faces, gt vertices).
        align (canonical only): `pose` (default: the identity) is first refined by sobfu_amd.evaluate.align_meshes -- align_iters
        iterations, align_dof 6 (rigid) or 3 (translation only: symmetric objects) -- and the dict gains "pose" (the refined 4 x 4) and
        "align" (the alignment's info).  The live mesh is never aligned: that would hide the tracking error evaluation measures.
        signed: each direction gains signed_mean, inside and open (compare_meshes): a_to_b.signed_mean > 0 says the model lies outside
        the (closed) ground truth on average.
        f_score: a dict of sobfu_amd.evaluate.f_score's arguments (thresholds, and density or n, seed, max_dist); the dict then gains
        "f_score", that function's result on the same (posed, aligned) meshes.  Without it the result is unchanged."""
        import torch

        from . import evaluate as E

        if which not in ("canonical", "live"):
            raise ValueError(f"which is 'canonical' or 'live', not {which!r}")
        if self.phi_global is None:
            raise RuntimeError("phi_global does not exist before the first frame")
        P = self.P
        v, _, f = self.ops.marching_cubes_indexed(self.phi_global, P["size"], P["R"], P["t"])
        if which == "live":
            v = self.warp_to_live(v)
        gv = E.device_tensor(gt_vertices, torch.float32)
        info = None
        if align:
            if which != "canonical":
                raise ValueError("align refines the pose of the canonical evaluation only")
            pose, info = E.align_meshes(v, gv, gt_faces, pose, iters=align_iters, max_dist=max_dist, dof=align_dof)
        if pose is not None:
            gv = E.device_tensor(transform_points(gv.cpu().numpy(), pose), torch.float32)
        r = E.compare_meshes(v, f, gv, gt_faces, max_dist, signed=signed)
        if align:
            r["pose"], r["align"] = pose, info
        if f_score is not None:
            r["f_score"] = E.f_score(v, f, gv, gt_faces, **f_score)
        return (r, v, f, gv) if return_meshes else r

    def close(self):
        if self.solver is not None:
            self.solver.close()
            self.solver = None
