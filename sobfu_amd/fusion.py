"""The per-frame pipeline of the reference's SobFusion::operator() (src/sobfu/sob_fusion.cpp:71-145) on one GPU, through the C ABI:
depth pre-steps -> frame 0: integrate into phi_global | frame n: clear + integrate phi_n, estimate_psi (iterations + 48-sweep
inverse + canonical warp), fuse phi_n o psi into phi_global.  Optional colour frames are fused into colour_global through the TSDF
that is fused in the same frame and psi (sobfu_amd/csrc/colour_kernels.hip).  The Python twin of sobfu::SobFusion in include/sobfu_amd/sobfu.hpp
(what apps/sobfu_headless drives); bench.py times it for the frames/s figures (BASELINE config 5)."""
from __future__ import annotations


class SobFusion:
    """params: a dict as sobfu_amd.params.read_ini returns (dims, vs, trunc, eta, max_weight, intr, R, t, start_frame, bilateral,
    trunc_depth, max_iter, max_update_norm, s, lam, alpha, w_reg)."""

    def __init__(self, params, max_iter=None):
        from . import ops

        self.ops, self.P = ops, params
        self.max_iter = int(params["max_iter"] if max_iter is None else max_iter)
        self.frame = 0
        self.phi_global = self.phi_global_psi_inv = self.phi_n = self.phi_n_psi = self.psi = self.psi_inv = self.solver = None
        self.last_report = None
        self.colour_global = None  # (Z, Y, X, 4) uint8 (b, g, r, weight), allocated on the first colour frame
        self.image_shape = None  # (rows, cols) of the depth frames: the camera render() draws with

    def __call__(self, depth_u16, colour=None):
        """colour (optional): a (rows, cols, 4) uint8 BGRA frame registered to depth_u16, of its size; None = the geometry-only path"""
        ops, P = self.ops, self.P
        if colour is not None and tuple(colour.shape) != tuple(depth_u16.shape) + (4,):
            raise ValueError(f"colour frame {tuple(colour.shape)} does not match the depth frame {tuple(depth_u16.shape)}")
        self.image_shape = tuple(depth_u16.shape)
        dims, vs = P["dims"], tuple(float(v) for v in P["vs"])
        ks, ss, sd = P["bilateral"]
        d = ops.bilateral_filter(depth_u16, ks, ss, sd)                                       # sob_fusion.cpp:78
        ops.truncate_depth(d, P["trunc_depth"])                                               # :85
        dists = ops.compute_dists(d, P["intr"])                                               # :91
        if self.frame == 0:                                                                   # :93-123
            self.phi_global = ops.new_volume(dims)
            ops.integrate_depth(dists, self.phi_global, vs, P["trunc"], P["eta"], P["R"], P["t"], P["intr"])
            self._colour(colour, self.phi_global, None)
            self.phi_global_psi_inv, self.phi_n, self.phi_n_psi = ops.new_volume(dims), ops.new_volume(dims), ops.new_volume(dims)
            self.psi, self.psi_inv = ops.new_field(dims), ops.new_field(dims)
            ops.init_identity(self.psi)
            ops.init_identity(self.psi_inv)
            self.solver = ops.Solver(dims, max_iter=self.max_iter, alpha=P["alpha"], w_reg=P["w_reg"], s=P["s"], lam=P["lam"],
                                     max_update_norm=P["max_update_norm"])
            self.frame += 1
            return None
        ops.clear_volume(self.phi_n)                                                          # :129
        ops.integrate_depth(dists, self.phi_n, vs, P["trunc"], P["eta"], P["R"], P["t"], P["intr"])  # :130
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
        self.ops.integrate_colour(colour, tsdf, psi, self.colour_global, P["vs"], P["R"], P["t"], P["intr"],
                                  self.ops.colour_weight_cap(P["max_weight"]))

    def colour_global_psi_inv(self):
        """the canonical colour warped to live, colour_global o psi_inv (computed on request); None without colour"""
        import torch

        if self.colour_global is None:
            return None
        return self.ops.apply_colour(self.colour_global, torch.empty_like(self.colour_global), self.psi_inv)

    def render(self, which="phi_global", light=(0.0, 0.0, 0.0), colour=True):
        """Raycast + shade one of the volumes ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi") from the sequence's own depth
        camera (the pose and intrinsics its frames are integrated with) -> (rows, cols, 4) uint8 BGRA image; light in the camera frame.
        With colour frames fused and colour=True, the canonical volumes phi_global and phi_global_psi_inv are shaded in colour
        (colour_global, colour_global o psi_inv); the live volumes are always grey."""
        if which not in ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi"):
            raise ValueError(f"unknown volume {which!r}")
        vol = getattr(self, which)
        if vol is None:
            raise RuntimeError(f"{which} does not exist before the first frame")
        P, (rows, cols) = self.P, self.image_shape
        pts, nrm = self.ops.raycast(vol, P["vs"], P["trunc"], P["R"], P["t"], P["intr"], rows=rows, cols=cols)
        if colour and self.colour_global is not None and which in ("phi_global", "phi_global_psi_inv"):
            col = self.colour_global if which == "phi_global" else self.colour_global_psi_inv()
            return self.ops.render_colour(pts, nrm, self.ops.sample_colour(col, P["vs"], P["R"], P["t"], pts, nrm), light)
        return self.ops.render_image(pts, nrm, light)

    def close(self):
        if self.solver is not None:
            self.solver.close()
            self.solver = None
