"""Thin torch-tensor front end over the C ABI (include/sobfu_hip.h).

torch is used for device memory and streams only; every function below is a single C-ABI call on raw device
pointers.  Tensor conventions (float32, contiguous, on a HIP device):
  TSDF volume (Z, Y, X, 2) {tsdf, weight}; vector field (Z, Y, X, 4) (w == 0); Jacobian (Z, Y, X, 4, 4).
Names follow the reference's launcher names (include/sobfu/*.hpp `namespace device`, kfusion/internal.hpp).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib
from ._lib import SolverParams, SolverReport, check

_F3 = C.c_float * 3
_F2 = C.c_float * 2
_F7 = C.c_float * 7
_F9 = C.c_float * 9


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("sobfu_amd needs a HIP device (MI355X); there is no CPU fallback")


def _ptr(t: torch.Tensor, dtype=torch.float32):
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
        raise ValueError(f"expected a contiguous {dtype} tensor on the GPU, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _xyz(t: torch.Tensor):
    Z, Y, X = t.shape[:3]
    return C.c_int(X), C.c_int(Y), C.c_int(Z)


def _f(x):
    return C.c_float(float(x))


def _pose(R, t):
    return (_F9(*[float(v) for v in np.asarray(R, np.float32).reshape(9)]), _F3(*[float(v) for v in np.asarray(t, np.float32).reshape(3)]))


def _vs3(voxel_size):
    return _F3(*[float(v) for v in voxel_size])


def new_volume(dims, device="cuda"):
    X, Y, Z = dims
    return torch.zeros((Z, Y, X, 2), dtype=torch.float32, device=device)


def new_field(dims, device="cuda"):
    X, Y, Z = dims
    return torch.zeros((Z, Y, X, 4), dtype=torch.float32, device=device)


def new_jacobian(dims, device="cuda"):
    X, Y, Z = dims
    return torch.zeros((Z, Y, X, 4, 4), dtype=torch.float32, device=device)


# ---- TSDF --------------------------------------------------------------------------------------
def clear_volume(vol):
    check(_lib.lib().sobfu_hip_clear_volume(_ptr(vol), *_xyz(vol), _stream()), "clear_volume")


def integrate_depth(dists, vol, voxel_size, trunc, eta, R, t, intr):
    Rm, tv = _pose(R, t)
    assert dists.is_cuda and dists.dtype == torch.float32 and dists.stride(1) == 1
    check(_lib.lib().sobfu_hip_integrate_depth(C.c_void_p(dists.data_ptr()), C.c_int(dists.stride(0) * 4),
                                               C.c_int(dists.shape[0]), C.c_int(dists.shape[1]), _ptr(vol), *_xyz(vol),
                                               _vs3(voxel_size), _f(trunc), _f(eta), Rm, tv, _f(intr[0]), _f(intr[1]), _f(intr[2]), _f(intr[3]),
                                               _stream()), "integrate_depth")


def tile3_integrate_depth(dists, vol_local, base, voxel_size, trunc, eta, R, t, intr):
    """integrate(depth) into a tile whose local cell (0, 0, 0) is global cell `base` = (xb, yb, zb) (multi-GPU tiles)"""
    Rm, tv = _pose(R, t)
    assert dists.is_cuda and dists.dtype == torch.float32 and dists.stride(1) == 1
    check(_lib.lib().sobfu_hip_tile3_integrate_depth(C.c_void_p(dists.data_ptr()), C.c_int(dists.stride(0) * 4), C.c_int(dists.shape[0]),
                                                     C.c_int(dists.shape[1]), _ptr(vol_local), *_xyz(vol_local), *[C.c_int(int(b)) for b in base],
                                                     _vs3(voxel_size), _f(trunc), _f(eta), Rm, tv, _f(intr[0]),
                                                     _f(intr[1]), _f(intr[2]), _f(intr[3]), _stream()), "tile3_integrate_depth")


def integrate_fuse(phi_global, phi_n_psi, max_weight):
    check(_lib.lib().sobfu_hip_integrate_fuse(_ptr(phi_global), _ptr(phi_n_psi), *_xyz(phi_global), _f(max_weight),
                                              _stream()), "integrate_fuse")


def init_sphere(vol, voxel_size, trunc, eta, centre, radius):
    check(_lib.lib().sobfu_hip_init_sphere(_ptr(vol), *_xyz(vol), _vs3(voxel_size), _f(trunc),
                                           _f(eta), _F3(*[float(np.float32(v)) for v in centre]), _f(np.float32(radius)),
                                           _stream()), "init_sphere")


def init_box(vol, voxel_size, trunc, b):
    check(_lib.lib().sobfu_hip_init_box(_ptr(vol), *_xyz(vol), _vs3(voxel_size), _f(trunc),
                                        _F3(*[float(v) for v in b]), _stream()), "init_box")


def init_ellipsoid(vol, voxel_size, trunc, r):
    check(_lib.lib().sobfu_hip_init_ellipsoid(_ptr(vol), *_xyz(vol), _vs3(voxel_size), _f(trunc),
                                              _F3(*[float(v) for v in r]), _stream()), "init_ellipsoid")


def init_plane(vol, voxel_size, trunc, z):
    check(_lib.lib().sobfu_hip_init_plane(_ptr(vol), *_xyz(vol), _vs3(voxel_size), _f(trunc), _f(z),
                                          _stream()), "init_plane")


def init_torus(vol, voxel_size, trunc, t):
    check(_lib.lib().sobfu_hip_init_torus(_ptr(vol), *_xyz(vol), _vs3(voxel_size), _f(trunc),
                                          _F2(*[float(v) for v in t]), _stream()), "init_torus")


# ---- depth pre-steps -----------------------------------------------------------------------------
def _u16(t):
    # torch has no uint16 arithmetic on all builds; depth images travel as int16 views of the same bits
    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.int16, torch.uint16)):
        raise ValueError("depth images must be contiguous 16-bit tensors on the GPU")
    return C.c_void_p(t.data_ptr())


def bilateral_filter(src, ksz, sigma_spatial, sigma_depth):
    dst = torch.empty_like(src)
    rows, cols = src.shape
    check(_lib.lib().sobfu_hip_bilateral_filter(_u16(src), C.c_int(cols * 2), _u16(dst), C.c_int(cols * 2), C.c_int(rows),
                                                C.c_int(cols), C.c_int(ksz), _f(sigma_spatial), _f(sigma_depth), _stream()),
          "bilateral_filter")
    return dst


def truncate_depth(depth, max_dist_m):
    rows, cols = depth.shape
    check(_lib.lib().sobfu_hip_truncate_depth(_u16(depth), C.c_int(cols * 2), C.c_int(rows), C.c_int(cols), _f(max_dist_m),
                                              _stream()), "truncate_depth")


def compute_dists(depth, intr):
    rows, cols = depth.shape
    dists = torch.empty((rows, cols), dtype=torch.float32, device=depth.device)
    check(_lib.lib().sobfu_hip_compute_dists(_u16(depth), C.c_int(cols * 2), _ptr(dists), C.c_int(cols * 4), C.c_int(rows),
                                             C.c_int(cols), _f(intr[0]), _f(intr[1]), _f(intr[2]), _f(intr[3]), _stream()),
          "compute_dists")
    return dists


# ---- vector fields -----------------------------------------------------------------------------
def clear_field(f):
    check(_lib.lib().sobfu_hip_clear_field(_ptr(f), *_xyz(f), _stream()), "clear_field")


def init_identity(psi):
    check(_lib.lib().sobfu_hip_init_identity(_ptr(psi), *_xyz(psi), _stream()), "init_identity")


def apply(phi, phi_warped, psi):
    check(_lib.lib().sobfu_hip_apply(_ptr(phi), _ptr(phi_warped), _ptr(psi), *_xyz(phi), _stream()), "apply")


def estimate_inverse(psi, psi_inv, n_sweeps=48):
    check(_lib.lib().sobfu_hip_estimate_inverse(_ptr(psi), _ptr(psi_inv), *_xyz(psi), C.c_int(n_sweeps), _stream()),
          "estimate_inverse")


def tsdf_gradient(vol, grad):
    check(_lib.lib().sobfu_hip_tsdf_gradient(_ptr(vol), _ptr(grad), *_xyz(vol), _stream()), "tsdf_gradient")


def laplacian(psi, L):
    check(_lib.lib().sobfu_hip_laplacian(_ptr(psi), _ptr(L), *_xyz(psi), _stream()), "laplacian")


def jacobian(psi, J, mode):
    check(_lib.lib().sobfu_hip_jacobian(_ptr(psi), _ptr(J), *_xyz(psi), C.c_int(mode), _stream()), "jacobian")


# ---- solver launchers ----------------------------------------------------------------------------
def sobolev_filter(s, lam):
    out = (C.c_float * 16)()
    check(_lib.lib().sobfu_hip_sobolev_filter(C.c_int(s), _f(np.float32(lam)), out), "sobolev_filter")
    return np.array(out[:s], np.float32)


def _taps(S):
    S = np.asarray(S, np.float32)
    assert S.size >= 7
    return _F7(*[float(v) for v in S[:7]])


def potential_gradient(phi_n_psi, phi_global, grad, L, nabla_U, w_reg):
    check(_lib.lib().sobfu_hip_potential_gradient(_ptr(phi_n_psi), _ptr(phi_global), _ptr(grad), _ptr(L), _ptr(nabla_U),
                                                  _f(w_reg), *_xyz(phi_n_psi), _stream()), "potential_gradient")


def convolution_rows(dst, src, S):
    check(_lib.lib().sobfu_hip_convolution_rows(_ptr(dst), _ptr(src), _taps(S), *_xyz(src), _stream()), "convolution_rows")


def convolution_columns(dst, src, S):
    check(_lib.lib().sobfu_hip_convolution_columns(_ptr(dst), _ptr(src), _taps(S), *_xyz(src), _stream()), "convolution_columns")


def convolution_depth(dst, src, S):
    check(_lib.lib().sobfu_hip_convolution_depth(_ptr(dst), _ptr(src), _taps(S), *_xyz(src), _stream()), "convolution_depth")


def update_psi(psi, nabla_U_S, updates, alpha):
    check(_lib.lib().sobfu_hip_update_psi(_ptr(psi), _ptr(nabla_U_S), _ptr(updates), _f(alpha), *_xyz(psi), _stream()),
          "update_psi")


# ---- reductions ----------------------------------------------------------------------------------
def reduce_config(n):
    b, t = C.c_int(), C.c_int()
    check(_lib.lib().sobfu_hip_reduce_config(C.c_int(n), C.byref(b), C.byref(t)), "reduce_config")
    return b.value, t.value


def _scratch(dev):
    return torch.empty(65536 * 2, dtype=torch.float32, device=dev)


def data_energy(phi_global, phi_n):
    out, sc = C.c_float(), _scratch(phi_global.device)
    check(_lib.lib().sobfu_hip_data_energy(_ptr(phi_global), _ptr(phi_n), C.c_int(phi_global.numel() // 2), _ptr(sc),
                                           C.byref(out), _stream()), "data_energy")
    return out.value


def reg_energy_sobolev(J):
    out, sc = C.c_float(), _scratch(J.device)
    check(_lib.lib().sobfu_hip_reg_energy_sobolev(_ptr(J), C.c_int(J.numel() // 16), _ptr(sc), C.byref(out), _stream()),
          "reg_energy_sobolev")
    return out.value


def reg_energy_sobolev_from_psi(psi):
    out, sc = C.c_float(), _scratch(psi.device)
    check(_lib.lib().sobfu_hip_reg_energy_sobolev_from_psi(_ptr(psi), *_xyz(psi), _ptr(sc), C.byref(out), _stream()),
          "reg_energy_sobolev_from_psi")
    return out.value


def max_update_norm(updates):
    out, sc = _F2(), _scratch(updates.device)
    check(_lib.lib().sobfu_hip_max_update_norm(_ptr(updates), C.c_int(updates.numel() // 4), _ptr(sc), out, _stream()),
          "max_update_norm")
    return out[0], out[1]


# ---- fused passes --------------------------------------------------------------------------------
def fused_potential_gradient(phi_n_psi, phi_global, psi, nabla_U, w_reg):
    check(_lib.lib().sobfu_hip_fused_potential_gradient(_ptr(phi_n_psi), _ptr(phi_global), _ptr(psi), _ptr(nabla_U),
                                                        _f(w_reg), *_xyz(psi), _stream()), "fused_potential_gradient")


def fused_smooth_update_apply(nabla_U, psi, phi_n, phi_n_psi, S, alpha, updates=None, slots=None):
    """Returns max ||u|| (sqrt rounded down, as Reductor::max_update_norm().x)."""
    if slots is None:
        slots = torch.zeros(256, dtype=torch.int32, device=psi.device)
    up = _ptr(updates) if updates is not None else None
    check(_lib.lib().sobfu_hip_fused_smooth_update_apply(_ptr(nabla_U), _ptr(psi), _ptr(phi_n), _ptr(phi_n_psi), up,
                                                         _ptr(slots, torch.int32), _taps(S), _f(alpha), *_xyz(psi),
                                                         _stream()), "fused_smooth_update_apply")
    m = np.float32(slots.max().cpu().numpy().view(np.float32))
    r = np.sqrt(m, dtype=np.float32)
    if r > 0 and np.float64(r) * np.float64(r) > np.float64(m):
        r = np.nextafter(r, np.float32(-np.inf), dtype=np.float32)
    return float(r)


# ---- solver handle -------------------------------------------------------------------------------
class Solver:
    """sobfu::cuda::Solver (reference include/sobfu/solver.hpp:52-101) over the opaque C handle."""

    def __init__(self, dims, *, max_iter, alpha, w_reg, s=7, lam=0.1, max_update_norm=-1.0, verbosity=0, quiet=True):
        _require_gpu()
        self.dims = tuple(int(d) for d in dims)
        self.params = SolverParams(verbosity, max_iter, s, max_update_norm, np.float32(lam), alpha, w_reg)
        self._h = C.c_void_p()
        check(_lib.lib().sobfu_hip_solver_create(C.byref(self._h), *[C.c_int(d) for d in self.dims],
                                                 C.byref(self.params)), "solver_create")
        self.log_lines = []
        self._cb = _lib.LOG_FN(self._on_log)
        self._quiet = quiet
        check(_lib.lib().sobfu_hip_solver_set_logger(self._h, self._cb, None), "solver_set_logger")

    def _on_log(self, line, _user):
        self.log_lines.append(line.decode())
        if not self._quiet:
            print(line.decode())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().sobfu_hip_solver_destroy(self._h)
            self._h = None

    __del__ = close

    def workspace_bytes(self):
        return int(_lib.lib().sobfu_hip_solver_workspace_bytes(self._h))

    def set_compact(self, enable=True):
        check(_lib.lib().sobfu_hip_solver_set_compact(self._h, C.c_int(1 if enable else 0)), "set_compact")

    def set_profiling(self, stride=1):
        """HIP events around the two launches of every stride-th iteration (0 / False = off)"""
        check(_lib.lib().sobfu_hip_solver_set_profiling(self._h, C.c_int(int(stride))), "set_profiling")

    def get_profile(self, reset=True):
        """(ms in pass A, ms in pass B, iterations timed) from HIP events on the solver's stream."""
        a, b, n = C.c_float(), C.c_float(), C.c_int()
        check(_lib.lib().sobfu_hip_solver_get_profile(self._h, C.byref(a), C.byref(b), C.byref(n), C.c_int(1 if reset else 0)),
              "get_profile")
        return a.value, b.value, n.value

    def keep_updates(self, keep=True):
        check(_lib.lib().sobfu_hip_solver_keep_updates(self._h, C.c_int(1 if keep else 0)), "keep_updates")

    def updates(self):
        """Tensor view (no copy) of Reductor::updates (reference src/sobfu/reductor.cpp:26)."""
        p = _lib.lib().sobfu_hip_solver_updates(self._h)
        if not p:
            raise _lib.HipError("solver_updates: allocation failed")
        X, Y, Z = self.dims

        class _Raw:
            __cuda_array_interface__ = {"shape": (Z, Y, X, 4), "typestr": "<f4", "data": (int(p), False), "version": 2}

        return torch.as_tensor(_Raw(), device="cuda")

    def estimate_psi(self, phi_global, phi_global_psi_inv, phi_n, phi_n_psi, psi, psi_inv):
        """Solver::estimate_psi (reference src/sobfu/solver.cpp:69-101).  Returns (report, per-iteration max norms)."""
        rep = SolverReport()
        hist = (C.c_float * max(1, self.params.max_iter))()
        check(_lib.lib().sobfu_hip_solver_estimate_psi(self._h, _ptr(phi_global), _ptr(phi_global_psi_inv), _ptr(phi_n),
                                                       _ptr(phi_n_psi), _ptr(psi), _ptr(psi_inv), C.byref(rep), hist,
                                                       _stream()), "solver_estimate_psi")
        return rep, np.array(hist[:rep.iterations], np.float32)

    def begin(self, phi_global, phi_n, phi_n_psi, psi, max_iters):
        """the loop in pieces (sobfu_hip_solver_begin / step / end): begin enters the iteration format, step(n) ENQUEUES n
        iterations without synchronising, end() synchronises and returns what iterate() would"""
        self._session = (phi_global, phi_n, phi_n_psi, psi, int(max_iters))  # keeps the buffers alive
        check(_lib.lib().sobfu_hip_solver_begin(self._h, _ptr(phi_global), _ptr(phi_n), _ptr(phi_n_psi), _ptr(psi), C.c_int(int(max_iters)),
                                                _stream()), "solver_begin")

    def step(self, n_iters):
        check(_lib.lib().sobfu_hip_solver_step(self._h, C.c_int(int(n_iters)), _stream()), "solver_step")

    def end(self):
        rep = SolverReport()
        hist = (C.c_float * max(1, self._session[4] if getattr(self, "_session", None) else 1))()
        check(_lib.lib().sobfu_hip_solver_end(self._h, C.byref(rep), hist, _stream()), "solver_end")
        self._session = None
        return rep, np.array(hist[:rep.iterations], np.float32)

    def iterate(self, phi_global, phi_n, phi_n_psi, psi, n_iters):
        rep = SolverReport()
        hist = (C.c_float * max(1, n_iters))()
        check(_lib.lib().sobfu_hip_solver_iterate(self._h, _ptr(phi_global), _ptr(phi_n), _ptr(phi_n_psi), _ptr(psi),
                                                  C.c_int(n_iters), C.byref(rep), hist, _stream()), "solver_iterate")
        return rep, np.array(hist[:rep.iterations], np.float32)


# ---- marching cubes (include/kfusion/internal.hpp:213-225) ---------------------------------------------------------------
def mc_workspace(vol):
    """scratch for mc_occupied_voxels / mc_offsets on volumes of this shape (keep it between frames: no allocation per call)"""
    _lib.lib().sobfu_hip_mc_workspace_bytes.restype = C.c_size_t
    n = int(_lib.lib().sobfu_hip_mc_workspace_bytes(*_xyz(vol)))
    return torch.empty(n, dtype=torch.uint8, device=vol.device)


def _ws(workspace):
    if workspace is None:
        return None, C.c_size_t(0)
    return _ptr(workspace, torch.uint8), C.c_size_t(workspace.numel())


def mc_occupied_voxels(vol, max_size, workspace=None):
    """getOccupiedVoxels -> (occupied int32 (3, max_size) on the GPU: voxel index / vertex count / vertex offset rows, count)"""
    occ = torch.zeros((3, int(max_size)), dtype=torch.int32, device=vol.device)
    n = C.c_int(0)
    check(_lib.lib().sobfu_hip_mc_occupied_voxels(_stream(), _ptr(vol), *_xyz(vol), _ptr(occ, torch.int32), C.c_int(occ.shape[1]),
                                                  C.c_int(int(max_size)), C.byref(n), *_ws(workspace)), "mc_occupied_voxels")
    return occ, n.value


def mc_offsets(occ, count, workspace=None):
    """computeOffsetsAndTotalVertices: row 2 = exclusive scan of row 1 -> total vertices"""
    total = C.c_int(0)
    check(_lib.lib().sobfu_hip_mc_offsets(_stream(), _ptr(occ, torch.int32), C.c_int(occ.shape[1]), C.c_int(int(count)), C.byref(total),
                                          *_ws(workspace)), "mc_offsets")
    return total.value


def mc_generate_triangles(vol, occ, count, volume_size, R, t, vertices, normals):
    """generateTriangles into float4 buffers (n, 4)"""
    Rm, tv = _pose(R, t)
    assert vertices.shape == normals.shape and vertices.shape[1] == 4
    check(_lib.lib().sobfu_hip_mc_generate_triangles(_stream(), _ptr(vol), *_xyz(vol), _ptr(occ, torch.int32), C.c_int(occ.shape[1]),
                                                     C.c_int(int(count)), _f(volume_size[0]), _f(volume_size[1]), _f(volume_size[2]), Rm, tv,
                                                     _ptr(vertices), _ptr(normals), C.c_int(vertices.shape[0])), "mc_generate_triangles")


def marching_cubes(vol, volume_size, R=np.eye(3), t=(0, 0, 0), max_voxels=2_000_000, max_vertices=None, workspace=None, colour=None):
    """kfusion::cuda::MarchingCubes::run (src/kfusion/marching_cubes.cpp:23-79) -> (vertices (n, 4), normals (n, 4)) GPU tensors; with a
    colour volume of the same dims, (vertices, normals, colours (n, 4) uint8 BGRA) -- the vertices' colours, sample_colour's rule"""
    max_vertices = max_vertices or 3 * max_voxels
    occ, count = mc_occupied_voxels(vol, max_voxels, workspace)
    if count == 0:
        e = torch.zeros((0, 4), dtype=torch.float32, device=vol.device)
        if colour is not None:
            return e, e.clone(), torch.zeros((0, 4), dtype=torch.uint8, device=vol.device)
        return e, e.clone()
    total = min(mc_offsets(occ, count, workspace), max_vertices // 3 * 3)  # whole triangles only
    v = torch.zeros((max_vertices, 4), dtype=torch.float32, device=vol.device)
    n = torch.zeros_like(v)
    mc_generate_triangles(vol, occ, count, volume_size, R, t, v, n)
    if colour is not None:
        Z, Y, X = vol.shape[:3]
        vs = [float(np.float32(volume_size[i]) / np.float32(d)) for i, d in enumerate((X, Y, Z))]  # the cell size of generateTriangles
        return v[:total], n[:total], sample_colour(colour, vs, R, t, v[:total], mc_vertices=True)
    return v[:total], n[:total]


def mc_indexed_workspace(vol):
    """workspace of marching_cubes_indexed on volumes of this shape (6 bytes per voxel; keep it between calls)"""
    _lib.lib().sobfu_hip_mc_indexed_workspace_bytes.restype = C.c_size_t
    n = int(_lib.lib().sobfu_hip_mc_indexed_workspace_bytes(*_xyz(vol)))
    return torch.empty(n, dtype=torch.uint8, device=vol.device)


def marching_cubes_indexed(vol, volume_size, R=np.eye(3), t=(0, 0, 0), workspace=None, colour=None):
    """Indexed (welded) marching cubes: one vertex per cut edge, shared by its triangles -> (vertices (V, 4), normals (V, 4) float32,
    faces (F, 3) int32) GPU tensors; with a colour volume of the same dims, + colours (V, 4) uint8 BGRA (sample_colour's rule).  Face k
    is marching_cubes' triangle k with corners 1 and 2 swapped; vertex normals are the TSDF gradient.  Rules: sobfu_amd/csrc/mc_kernels.hip."""
    L = _lib.lib()
    if workspace is None:
        workspace = mc_indexed_workspace(vol)
    Rm, tv = _pose(R, t)
    active, nv, nt = C.c_int(0), C.c_int(0), C.c_int(0)
    ws = _ws(workspace)
    check(L.sobfu_hip_mc_indexed_count(_stream(), _ptr(vol), *_xyz(vol), *ws, C.byref(active), C.byref(nv), C.byref(nt)), "mc_indexed_count")
    v = torch.zeros((nv.value, 4), dtype=torch.float32, device=vol.device)
    n = torch.zeros_like(v)
    f = torch.zeros((nt.value, 3), dtype=torch.int32, device=vol.device)
    if nt.value > 0:
        check(L.sobfu_hip_mc_indexed_generate(_stream(), _ptr(vol), *_xyz(vol), _f(volume_size[0]), _f(volume_size[1]), _f(volume_size[2]), Rm, tv,
                                              *ws, _ptr(v), _ptr(n), C.c_int(nv.value), _ptr(f, torch.int32), C.c_int(nt.value)),
              "mc_indexed_generate")
    if colour is not None:
        Z, Y, X = vol.shape[:3]
        vs = [float(np.float32(volume_size[i]) / np.float32(d)) for i, d in enumerate((X, Y, Z))]
        return v, n, f, sample_colour(colour, vs, R, t, v, mc_vertices=True)
    return v, n, f


# ---- rendering (kfusion::cuda::renderImage / renderTangentColors; KinectFusion raycaster) ---------------------------------------
def _image_ptr(t, dtype, channels):
    if not (t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.shape[2] == channels and t.stride(2) == 1 and t.stride(1) == channels):
        raise ValueError(f"expected a (rows, cols, {channels}) {dtype} image on the GPU with contiguous rows, got {t.dtype} {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr()), C.c_int(t.stride(0) * t.element_size())


def raycast(vol, voxel_size, trunc, R, t, intr, rows=480, cols=640, step_factor=0.75, points=None, normals=None):
    """Raycasts a TSDF volume (Z, Y, X, 2) from the camera of vol2cam = (R, t) (the pose integrate_depth takes) with intrinsics
    intr = (fx, fy, cx, cy) -> (points, normals), two (rows, cols, 4) float32 tensors in the camera frame; normals[..., 3] is 1 on a
    hit and 0 on a miss (where both are all zero).  `points` / `normals` may be given to render into existing buffers."""
    Rm, tv = _pose(R, t)
    if points is None:
        points = torch.empty((rows, cols, 4), dtype=torch.float32, device=vol.device)
    if normals is None:
        normals = torch.empty((rows, cols, 4), dtype=torch.float32, device=vol.device)
    vs = [float(np.float32(v)) for v in voxel_size]
    check(_lib.lib().sobfu_hip_raycast(_ptr(vol), *_xyz(vol), _f(vs[0]), _f(vs[1]), _f(vs[2]), _f(trunc), Rm, tv, _f(intr[0]), _f(intr[1]),
                                       _f(intr[2]), _f(intr[3]), C.c_int(int(rows)), C.c_int(int(cols)), _f(step_factor),
                                       *_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4), _stream()), "raycast")
    return points, normals


def render_image(points, normals, light=(0.0, 0.0, 0.0), image=None):
    """renderImage: Lambertian grey from a light at `light` (camera frame) -> (rows, cols, 4) uint8 BGRA; misses are all zero."""
    rows, cols = normals.shape[:2]
    if image is None:
        image = torch.empty((rows, cols, 4), dtype=torch.uint8, device=normals.device)
    check(_lib.lib().sobfu_hip_render_image(*_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4), C.c_int(rows),
                                            C.c_int(cols), _f(light[0]), _f(light[1]), _f(light[2]), *_image_ptr(image, torch.uint8, 4),
                                            _stream()), "render_image")
    return image


def render_normals(normals, image=None):
    """renderTangentColors: (r, g, b) = (n * 0.5 + 0.5) * 255 -> (rows, cols, 4) uint8 BGRA; misses are all zero."""
    rows, cols = normals.shape[:2]
    if image is None:
        image = torch.empty((rows, cols, 4), dtype=torch.uint8, device=normals.device)
    check(_lib.lib().sobfu_hip_render_normals(*_image_ptr(normals, torch.float32, 4), C.c_int(rows), C.c_int(cols),
                                              *_image_ptr(image, torch.uint8, 4), _stream()), "render_normals")
    return image


# ---- depth sensor model (sobfu_amd/csrc/depth_sensor_kernels.hip) ----------------------------------------------------
@dataclasses.dataclass
class SensorModel:
    """The fields of sobfu_hip_sensor_params but seed and frame (include/sobfu_hip.h states the rule they enter)."""
    lateral: float = 0.0        # sigma of the pixel jitter, pixels
    z_min: float = 0.0          # depths kept: (z_min, z_max]
    z_max: float = float("inf")
    cos_min: float = 0.0        # pixels seen flatter than this are lost
    edge_radius: int = 0        # 0..3; 0: no edge test
    edge_jump: float = 0.0      # metres
    edge_drop: float = 0.0      # probability that a pixel at an edge is lost
    drop: float = 0.0           # probability that any pixel is lost
    a0: float = 0.0             # sigma_z = (a0 + a1 (z - z0)^2) + a2 ((1 - c^2) / c^2) / sqrt(z)
    a1: float = 0.0
    z0: float = 0.0
    a2: float = 0.0
    disparity: float = 0.0      # focal x baseline x sub-pixel levels, pixel metres; 0: no quantisation

    @classmethod
    def kinect(cls, **changes):
        """a first-generation structured-light camera: Nguyen et al.'s axial noise, 0.8 pixels of jitter, 1/8-pixel disparity levels
        (8 x 0.075 m x 580 px), dropouts beyond 78 degrees and at half of the pixels next to a 5 cm jump"""
        return dataclasses.replace(cls(lateral=0.8, z_min=0.4, z_max=4.0, cos_min=0.2, edge_radius=1, edge_jump=0.05, edge_drop=0.5, drop=0.0,
                                       a0=0.0012, a1=0.0019, z0=0.4, a2=0.0001, disparity=348.0), **changes)

    @classmethod
    def ideal(cls, **changes):
        """the identity: the frame is the renderer's own depth image, rint(1000 z) of every hit"""
        return dataclasses.replace(cls(), **changes)

    def params(self, seed=0, frame=0):
        return _lib.SensorParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame) & 0xFFFFFFFF, self.lateral, self.z_min, self.z_max, self.cos_min,
                                 int(self.edge_radius), self.edge_jump, self.edge_drop, self.drop, self.a0, self.a1, self.z0, self.a2, self.disparity)


def _plane_ptr(t, dtypes, what):
    if not (t.is_cuda and t.dtype in dtypes and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)):
        raise ValueError(f"expected a (rows, cols) {dtypes[0]} {what} image on the GPU with contiguous rows, got {t.dtype} {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr()), C.c_int(t.stride(0) * t.element_size())


def depth_sensor(points, normals, model, seed=0, frame=0, depth=None, flags=False):
    """What a depth sensor described by `model` (a SensorModel) reports of a clean render: points, normals (rows, cols, 4) float32 as
    ops.raycast and TriangleGrid.render give them -> depth (rows, cols) int16, the bits of uint16 millimetres (0: no reading), as the
    depth pre-steps take them.  The random numbers depend on (seed, frame, pixel) alone: the same call gives the same frame.  depth: an
    existing (possibly pitched) image to write into.  flags: True -> (depth, flags), flags (rows, cols) uint8 with what became of every
    pixel (SOBFU_SENSOR_*: 0 valid, 1 miss, 2 range, 3 grazing, 4 edge, 5 dropout); an existing uint8 image may be given instead."""
    rows, cols = int(points.shape[0]), int(points.shape[1])
    if tuple(normals.shape[:2]) != (rows, cols):
        raise ValueError("points and normals differ in size")
    if depth is None:
        depth = torch.empty((rows, cols), dtype=torch.int16, device=points.device)
    if flags is True:
        flags = torch.empty((rows, cols), dtype=torch.uint8, device=points.device)
    want_flags = flags is not None and flags is not False
    for img in (depth,) + ((flags,) if want_flags else ()):
        if tuple(img.shape) != (rows, cols):
            raise ValueError(f"the output images must be {rows} x {cols}")
    p = model.params(seed, frame)
    fl = _plane_ptr(flags, (torch.uint8,), "flag") if want_flags else (None, C.c_int(0))
    check(_lib.lib().sobfu_hip_depth_sensor(*_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4), C.c_int(rows), C.c_int(cols),
                                            C.byref(p), *_plane_ptr(depth, (torch.int16, torch.uint16), "depth"), *fl, _stream()), "depth_sensor")
    return (depth, flags) if want_flags else depth


def philox4x32_10(counters, key):
    """The generator behind depth_sensor on its own: counters (n, 4) int32 (the bits of uint32), key = (k0, k1) -> (n, 4) int32 outputs"""
    if not (counters.dim() == 2 and counters.shape[1] == 4):
        raise ValueError("expected (n, 4) counters")
    out = torch.empty_like(counters)
    if counters.shape[0] == 0:
        return out
    k = (C.c_uint32 * 2)(int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF)
    check(_lib.lib().sobfu_hip_philox4x32_10(_ptr(counters, torch.int32), k, C.c_int(int(counters.shape[0])), _ptr(out, torch.int32), _stream()), "philox4x32_10")
    return out


# ---- colour (sobfu_amd/csrc/colour_kernels.hip): a (Z, Y, X, 4) uint8 volume of (b, g, r, weight); BGRA frames ---------------------
def new_colour_volume(dims, device="cuda"):
    X, Y, Z = dims
    return torch.zeros((Z, Y, X, 4), dtype=torch.uint8, device=device)


def colour_weight_cap(max_weight):
    """cap of the colour weight: min((int) TSDF_MAX_WEIGHT, 255), at least 1 (kfusion::cuda::colour_weight_cap)"""
    w = float(max_weight)
    return 1 if not w >= 1.0 else 255 if w >= 255.0 else int(w)


def _colour_ptr(t):
    if not (t.dim() == 4 and t.shape[3] == 4):
        raise ValueError(f"expected a (Z, Y, X, 4) uint8 colour volume, got {tuple(t.shape)}")
    return _ptr(t, torch.uint8)


def integrate_colour(image, tsdf, psi, colour, voxel_size, R, t, intr, cap):
    """Fuses a (rows, cols, 4) uint8 BGRA frame, registered to the depth camera of vol2cam = (R, t) with intr = (fx, fy, cx, cy), into
    `colour` through `tsdf` (the volume about to be fused) and `psi` (None = identity)."""
    Rm, tv = _pose(R, t)
    if tuple(colour.shape[:3]) != tuple(tsdf.shape[:3]) or (psi is not None and tuple(psi.shape[:3]) != tuple(tsdf.shape[:3])):
        raise ValueError("colour, tsdf and psi must have the same dims")
    check(_lib.lib().sobfu_hip_integrate_colour(*_image_ptr(image, torch.uint8, 4), C.c_int(image.shape[0]), C.c_int(image.shape[1]), _ptr(tsdf),
                                                None if psi is None else _ptr(psi), _colour_ptr(colour), *_xyz(colour),
                                                _vs3(voxel_size), Rm, tv, _f(intr[0]), _f(intr[1]), _f(intr[2]), _f(intr[3]),
                                                C.c_int(int(cap)), _stream()), "integrate_colour")


def apply_colour(colour, colour_warped, psi_inv):
    """colour_warped(y) = colour(psi_inv(y)), the renormalised trilinear colour sampler"""
    if tuple(colour.shape) != tuple(colour_warped.shape) or tuple(psi_inv.shape[:3]) != tuple(colour.shape[:3]):
        raise ValueError("colour, colour_warped and psi_inv must have the same dims")
    check(_lib.lib().sobfu_hip_apply_colour(_colour_ptr(colour), _colour_ptr(colour_warped), _ptr(psi_inv), *_xyz(colour), _stream()),
          "apply_colour")
    return colour_warped


def sample_colour(colour, voxel_size, R, t, points, normals=None, mc_vertices=False, out=None):
    """Samples `colour` at float4 points of a frame whose pose from volume metres is (R, t): a (rows, cols, 4) raycast image (with its
    normals: misses give zeros) or an (n, 4) list (marching-cubes vertices with mc_vertices=True and the marching-cubes pose) -> uint8
    BGRA of the same leading shape; a point with no colour gives (0, 0, 0, 0)."""
    Rm, tv = _pose(R, t)
    flat = points.dim() == 2
    p3 = points.unsqueeze(0) if flat else points
    if out is None:
        out = torch.empty(points.shape[:-1] + (4,), dtype=torch.uint8, device=points.device)
    o3 = out.unsqueeze(0) if out.dim() == 2 else out
    rows, cols = p3.shape[:2]
    if rows * cols == 0:
        return out
    nrm = (None, C.c_int(0)) if normals is None else _image_ptr(normals.unsqueeze(0) if normals.dim() == 2 else normals, torch.float32, 4)
    check(_lib.lib().sobfu_hip_sample_colour(_colour_ptr(colour), *_xyz(colour), _vs3(voxel_size), Rm, tv,
                                             C.c_int(1 if mc_vertices else 0), *_image_ptr(p3, torch.float32, 4), *nrm, C.c_int(rows),
                                             C.c_int(cols), *_image_ptr(o3, torch.uint8, 4), _stream()), "sample_colour")
    return out


def render_colour(points, normals, colours, light=(0.0, 0.0, 0.0), image=None):
    """render_image with colour: a hit with colour (colours[..., 3] != 0) -> colour * (0.2 + 0.8 max(0, n . l)), a hit without colour ->
    render_image's grey, a miss -> zeros; (rows, cols, 4) uint8 BGRA."""
    rows, cols = normals.shape[:2]
    if image is None:
        image = torch.empty((rows, cols, 4), dtype=torch.uint8, device=normals.device)
    check(_lib.lib().sobfu_hip_render_colour(*_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4),
                                             *_image_ptr(colours, torch.uint8, 4), C.c_int(rows), C.c_int(cols), _f(light[0]), _f(light[1]),
                                             _f(light[2]), *_image_ptr(image, torch.uint8, 4), _stream()), "render_colour")
    return image


# ---- points through the deformation (sobfu_amd/csrc/warp_points_kernels.hip): (n, 4) float32 point / normal lists --------------------
def _point_list(t, what):
    if not (t.dim() == 2 and t.shape[1] == 4):
        raise ValueError(f"expected an (n, 4) float32 list of {what}, got {tuple(t.shape)}")
    return _ptr(t)


def warp_points(psi, voxel_size, R, t, points, normals=None, mc_vertices=False, out=None):
    """Carries (n, 4) points of a frame whose pose from volume metres is (R, t) (marching-cubes vertices with mc_vertices=True and the
    marching-cubes pose) through psi, v -> psi(v), and their normals (optional) through the cofactor matrix of psi's Jacobian -> points,
    or (points, normals).  `out`: a tensor (or, with normals, a pair) to write into; it may be the input."""
    Rm, tv = _pose(R, t)
    po, no = (out if normals is not None else (out, None)) if out is not None else (None, None)
    po = torch.empty_like(points) if po is None else po
    if normals is not None:
        no = torch.empty_like(normals) if no is None else no
        if tuple(normals.shape) != tuple(points.shape) or tuple(no.shape) != tuple(points.shape):
            raise ValueError("points and normals must have the same shape")
    if tuple(po.shape) != tuple(points.shape):
        raise ValueError("the output must have the points' shape")
    if points.shape[0] == 0:  # an empty tensor has no address to hand over
        return po if normals is None else (po, no)
    check(_lib.lib().sobfu_hip_warp_points(_ptr(psi), *_xyz(psi), _vs3(voxel_size), Rm, tv, C.c_int(1 if mc_vertices else 0),
                                           _point_list(points, "points"), None if normals is None else _point_list(normals, "normals"),
                                           C.c_int(points.shape[0]), _point_list(po, "points"), None if normals is None else _point_list(no, "normals"),
                                           _stream()), "warp_points")
    return po if normals is None else (po, no)


def sample_tsdf(vol, voxel_size, R, t, points, mc_vertices=False, out=None):
    """The trilinear TSDF of `vol` (Z, Y, X, 2) at (n, 4) points (pose and mc_vertices as in warp_points) -> (n,) float32 in units of the
    truncation distance; NaN where one of the eight corners has no weight (the raycaster's validity rule)."""
    Rm, tv = _pose(R, t)
    if out is None:
        out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    if tuple(out.shape) != (points.shape[0],):
        raise ValueError("the output must hold one float per point")
    if points.shape[0] == 0:
        return out
    check(_lib.lib().sobfu_hip_sample_tsdf(_ptr(vol), *_xyz(vol), _vs3(voxel_size), Rm, tv, C.c_int(1 if mc_vertices else 0),
                                           _point_list(points, "points"), C.c_int(points.shape[0]), _ptr(out), _stream()), "sample_tsdf")
    return out


# ---- exact point-to-mesh distances (sobfu_amd/csrc/mesh_distance_kernels.hip) ------------------------------------------------------------
_MESH_MODES = {"auto": 0, "grid": 1, "brute": 2}


def mesh_grid_plan(bbox, n_triangles, cell=None):
    """The uniform grid over a mesh with this bounding box (min x, y, z, max x, y, z) -> origin (3,) float32, h, dims (3,) (host only)"""
    origin, h, dims = _F3(), C.c_float(0), (C.c_int * 3)()
    check(_lib.lib().sobfu_hip_mesh_grid_plan((C.c_float * 6)(*[float(v) for v in bbox]), C.c_int(int(n_triangles)), _f(cell or 0.0), origin,
                                              C.byref(h), dims), "mesh_grid_plan")
    return np.array(list(origin), np.float32), float(h.value), np.array(list(dims), np.int32)


def align_info(status, iters, trace):
    """the status word of sobfu_hip_mesh_align_estimate -> dict(status, iterations, converged, failed, trace)"""
    failed, converged = bool(status & 0x10000), bool(status & 0x20000)
    done = (status & 0xFFFF) if status else iters
    return dict(status=status, iterations=done, converged=converged, failed=failed, trace=np.array(trace[:min(iters, done + (1 if failed else 0))]))


class TriangleGrid:
    """A uniform grid over an indexed triangle mesh -- vertices (V, 4) float32, faces (F, 3) int32, GPU tensors that must stay unchanged
    while the grid is used -- for exact nearest-triangle queries.  cell: the cell edge (None: the plan's default).  Owns the workspace.
    A face index out of range or a non-finite corner raises HipError (SOBFU_E_BADARG) here: there is no grid to query then."""

    def __init__(self, vertices, faces, cell=None):
        L = _lib.lib()
        L.sobfu_hip_mesh_grid_workspace_bytes.restype = C.c_size_t
        _point_list(vertices, "vertices")
        if not (faces.dim() == 2 and faces.shape[1] == 3):
            raise ValueError(f"expected (F, 3) int32 faces, got {tuple(faces.shape)}")
        self.vertices, self.faces = vertices, faces
        self.n_vertices, self.n_triangles = int(vertices.shape[0]), int(faces.shape[0])
        xyz = vertices[:, :3]
        xyz = xyz[torch.isfinite(xyz).all(1)]  # a non-finite vertex is the build's to refuse when a face uses it
        if xyz.shape[0] and self.n_triangles:
            bbox = torch.cat([xyz.amin(0), xyz.amax(0)]).cpu().numpy()
        else:
            bbox = np.zeros(6, np.float32)
        self.origin, self.h, dims = mesh_grid_plan(bbox, self.n_triangles, cell)
        self.dims = tuple(int(d) for d in dims)
        self._plan = (_F3(*[float(v) for v in self.origin]), _f(self.h), (C.c_int * 3)(*[int(d) for d in self.dims]))
        self.unresolved_buffer = None
        refs, max_refs = C.c_int(0), 8 * self.n_triangles + 1024
        while True:
            nbytes = int(L.sobfu_hip_mesh_grid_workspace_bytes(self._plan[2], C.c_int(max_refs)))
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=vertices.device)
            rc = L.sobfu_hip_mesh_grid_build(*self._mesh(), *self._plan, *_ws(self.workspace), C.c_int(max_refs), C.byref(refs), _stream())
            if rc == -3 and refs.value > max_refs:  # SOBFU_E_UNSUPPORTED: the references need more room
                max_refs = refs.value
                continue
            check(rc, "mesh_grid_build")
            break
        self.references = refs.value
        self._boundary, self.boundary_edges = None, None

    @property
    def boundary(self):
        """The mesh's boundary chain on the device, computed once: (B, 2, 4) float32, per edge u = (x, y, z, k) and v = (x, y, z, 0) with
        k = (#triangles that run u -> v) - (#that run v -> u) != 0, sorted by the vertex indices (u < v).  Empty for a closed,
        consistently oriented mesh.  boundary_edges: the (B, 3) int32 numpy rows (u, v, k)."""
        if self._boundary is None:
            faces = np.ascontiguousarray(self.faces.detach().cpu().numpy(), np.int32)
            L, count = _lib.lib(), C.c_int(0)
            fp = faces.ctypes.data_as(C.POINTER(C.c_int)) if self.n_triangles else None
            check(L.sobfu_hip_mesh_boundary(fp, C.c_int(self.n_triangles), C.c_int(self.n_vertices), None, C.c_int(0), C.byref(count)), "mesh_boundary")
            edges = np.zeros((count.value, 3), np.int32)
            if count.value:
                check(L.sobfu_hip_mesh_boundary(fp, C.c_int(self.n_triangles), C.c_int(self.n_vertices), edges.ctypes.data_as(C.POINTER(C.c_int)),
                                                C.c_int(count.value), C.byref(count)), "mesh_boundary")
            self.boundary_edges = edges
            dev = self.vertices.device
            b = torch.zeros((len(edges), 2, 4), dtype=torch.float32, device=dev)
            if len(edges):
                idx = torch.from_numpy(edges.astype(np.int64)).to(dev)
                b[:, 0, :3], b[:, 1, :3] = self.vertices[idx[:, 0], :3], self.vertices[idx[:, 1], :3]
                b[:, 0, 3] = idx[:, 2].to(torch.float32)
            self._boundary = b.contiguous()
        return self._boundary

    def _boundary_args(self):
        b = self.boundary
        return (_ptr(b) if b.shape[0] else None, C.c_int(int(b.shape[0])))

    def _mesh(self):
        return (_ptr(self.vertices) if self.n_vertices else None, C.c_int(self.n_vertices),
                _ptr(self.faces, torch.int32) if self.n_triangles else None, C.c_int(self.n_triangles))

    def _target(self):  # the nine arguments every mesh entry point of the C ABI starts with: the grid's workspace, the mesh, the plan
        return (*_ws(self.workspace), *self._mesh(), *self._plan)

    @staticmethod
    def _mode(mode):
        if mode not in _MESH_MODES:
            raise ValueError(f"unknown mode {mode!r}")
        return C.c_int(_MESH_MODES[mode])

    def query(self, points, max_dist=None, closest=False, mode="auto", ring_cap=None):
        """(n, 4) float32 points -> dist (n,) float32, tri (n,) int32 [, closest (n, 4) float32]: the distance to the nearest triangle, the
        lowest triangle index at that distance and its closest point (x, y, z, 1).  max_dist: farther points get (+Inf, -1, zeros).
        mode "auto" | "grid" | "brute" and ring_cap (shells walked before a point goes to brute force) never change the answer."""
        mode = self._mode(mode)
        n = int(points.shape[0])
        dist = torch.empty(n, dtype=torch.float32, device=points.device)
        tri = torch.empty(n, dtype=torch.int32, device=points.device)
        cl = torch.empty((n, 4), dtype=torch.float32, device=points.device) if closest else None
        if n:
            self.unresolved_buffer = torch.empty(n, dtype=torch.int32, device=points.device)
            check(_lib.lib().sobfu_hip_mesh_distance(*self._target(), _point_list(points, "points"), C.c_int(n), _f(0.0 if max_dist is None else max_dist),
                                                     mode, C.c_int(int(ring_cap or 0)), _ptr(dist), _ptr(tri, torch.int32), None if cl is None else _ptr(cl),
                                                     _ptr(self.unresolved_buffer, torch.int32), _stream()), "mesh_distance")
        return (dist, tri, cl) if closest else (dist, tri)

    # ---- rigid alignment of a point list to this mesh (sobfu_amd/csrc/mesh_align_kernels.hip) ----
    def _align_workspace(self, n, device):
        return torch.empty(int(_lib.lib().sobfu_hip_mesh_align_workspace_bytes(C.c_int(n))), dtype=torch.uint8, device=device)

    def _align_target(self, points, n, max_dist, mode, ring_cap):
        mode = self._mode(mode)
        return (*self._target(), _point_list(points, "points") if n else None, C.c_int(n), _f(0.0 if max_dist is None else max_dist), mode,
                C.c_int(int(ring_cap or 0)))

    def align_step(self, points, pose, max_dist=None, mode="auto", ring_cap=None):
        """One transform + nearest-triangle query + reduction of the (n, 4) float32 points at the 4 x 4 `pose` (points -> this mesh's
        frame) -> the 29 float64 sums of the point-to-plane normal equations (numpy): the 21 upper-triangular J_i J_j, the 6 J_i r, the
        inlier count, the sum of r r.  No solve."""
        n = int(points.shape[0])
        if n == 0:
            return np.zeros(29)
        pose_d = torch.as_tensor(np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16)), device=points.device)
        ws = self._align_workspace(n, points.device)
        sums = torch.empty(29, dtype=torch.float64, device=points.device)
        check(_lib.lib().sobfu_hip_mesh_align_step(*self._align_target(points, n, max_dist, mode, ring_cap), _ptr(pose_d), *_ws(ws),
                                                   _ptr(sums, torch.float64), _stream()), "mesh_align_step")
        return sums.cpu().numpy()

    def align(self, points, pose=None, iters=30, max_dist=None, dof=6, eps_rot=0.0, eps_trans=0.0, mode="auto", ring_cap=None, trace=None):
        """Point-to-plane ICP of the (n, 4) float32 points against this mesh from `pose` (4 x 4, points -> this mesh's frame; None: the
        identity): `iters` iterations enqueued as one chain, one synchronisation to read the result -> (pose (4, 4) float32 tensor,
        info).  dof 6: rigid; 3: translation only.  The loop stops early once an update is below both eps_rot (radians) and eps_trans
        (metres); 0 never stops.  info: status (the device's word), iterations (updates applied), converged (stopped by the gate),
        failed (the solve of iteration `iterations` had a non-positive pivot: the pose before it is returned), trace ((iterations
        run, 4) float32: inliers, rms residual, |w|, |t_inc|).  Without points there is nothing to solve: failed at iteration 0.
        trace: an (iters, 4) float32 GPU tensor for the device to write into (rows of iterations that did not run are left as they are)."""
        n = int(points.shape[0])
        iters = int(iters)
        start = np.eye(4, dtype=np.float32) if pose is None else np.ascontiguousarray(np.asarray(pose, np.float32).reshape(4, 4))
        pose_d = torch.as_tensor(start.reshape(16).copy(), device=points.device)
        status = torch.zeros(1, dtype=torch.int32, device=points.device)
        if trace is None:
            trace = torch.zeros((max(iters, 1), 4), dtype=torch.float32, device=points.device)
        elif tuple(trace.shape) != (iters, 4) or iters == 0:
            raise ValueError("the trace must hold (iters, 4) floats")
        ws = self._align_workspace(n, points.device)
        if int(dof) not in (3, 6) or iters < 0:
            raise ValueError("dof is 3 or 6 and iters >= 0")
        if n:
            check(_lib.lib().sobfu_hip_mesh_align_estimate(*self._align_target(points, n, max_dist, mode, ring_cap), C.c_int(iters), C.c_int(int(dof)),
                                                           _f(eps_rot), _f(eps_trans), *_ws(ws), _ptr(pose_d), _ptr(status, torch.int32), _ptr(trace),
                                                           _stream()), "mesh_align_estimate")
        st = int(status.item()) if n else (0x10000 if iters else 0)
        return pose_d.reshape(4, 4), align_info(st, iters, trace.cpu().numpy())

    # ---- rays against this mesh (sobfu_amd/csrc/mesh_ray_kernels.hip) ----
    def raycast(self, origins, dirs, t_min=0.0, t_max=None, mode="auto", bary=False, side=False):
        """(n, 4) float32 origins and directions (not normalised, w ignored) -> t (n,) float32, tri (n,) int32 [, bary (n, 2) float32]
        [, side (n,) int8]: the smallest ray parameter in (t_min, t_max] at which the ray meets a triangle, the lowest triangle index at
        that parameter, the weights of its second and third corner, and +1 / -1 for the face whose corners run counter-clockwise /
        clockwise as seen from the origin.  A miss is (+Inf, -1, (0, 0), 0).  t_max None: unlimited.  mode "auto" | "grid" | "brute"
        never changes the answer."""
        mode = self._mode(mode)
        n = int(origins.shape[0])
        if int(dirs.shape[0]) != n:
            raise ValueError("origins and dirs must hold the same number of rays")
        dev = origins.device
        t = torch.empty(n, dtype=torch.float32, device=dev)
        tri = torch.empty(n, dtype=torch.int32, device=dev)
        b = torch.empty((n, 2), dtype=torch.float32, device=dev) if bary else None
        s = torch.empty(n, dtype=torch.int8, device=dev) if side else None
        if n:
            check(_lib.lib().sobfu_hip_mesh_raycast(*self._target(), _point_list(origins, "origins"), _point_list(dirs, "dirs"), C.c_int(n), _f(t_min),
                                                    _f(0.0 if t_max is None else t_max), mode, _ptr(t), _ptr(tri, torch.int32),
                                                    None if b is None else _ptr(b), None if s is None else _ptr(s, torch.int8), _stream()), "mesh_raycast")
        return tuple(x for x in (t, tri, b, s) if x is not None)

    def render(self, intr, rows, cols, pose=None, z_min=0.0, z_max=None, vertex_normals=None, vertex_colours=None, outputs=("depth",)):
        """This mesh seen by the pinhole camera intr = (fx, fy, cx, cy) at `pose` = (R, t), mesh frame -> camera frame (the pose raycast
        and integrate_depth take; None: the identity) -> a dict with the images named in `outputs`: "depth" (rows, cols) int16, the
        bits of uint16 millimetres as the depth pre-steps take them (0: a miss), "points" and "normals" (rows, cols, 4) float32 in ops.raycast's format, "colour" (rows, cols, 4) uint8
        BGRA (needs vertex_colours, (V, 4) uint8 BGRA), "tri" (rows, cols) int32 (-1: a miss).  vertex_normals: (V, 4) float32, mixed
        over the face; None: the face's own normal.  Depths are limited to (z_min, z_max]; z_max None: unlimited.  An entry of
        `outputs` may also be given as a dict name -> tensor to render into existing (possibly pitched) images."""
        given = dict(outputs) if isinstance(outputs, dict) else {name: None for name in outputs}
        kinds = {"depth": (torch.int16, 0), "points": (torch.float32, 4), "normals": (torch.float32, 4), "colour": (torch.uint8, 4), "tri": (torch.int32, 0)}
        unknown = set(given) - set(kinds)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        if "colour" in given and vertex_colours is None:
            raise ValueError("the colour output needs vertex_colours")
        R, t = (np.eye(3), (0.0, 0.0, 0.0)) if pose is None else pose
        Rm, tv = _pose(R, t)
        dev = self.vertices.device
        args = []
        for name in ("depth", "points", "normals", "colour", "tri"):
            dtype, ch = kinds[name]
            if name not in given:
                args += [None, C.c_int(0)]
                continue
            img = given[name]
            if img is None:
                img = given[name] = torch.empty((rows, cols, ch) if ch else (rows, cols), dtype=dtype, device=dev)
            if ch:
                args += list(_image_ptr(img, dtype, ch))
            else:
                sixteen = name == "depth" and img.dtype == torch.uint16  # the same bits
                if not (img.is_cuda and (img.dtype == dtype or sixteen) and img.dim() == 2 and img.stride(1) == 1):
                    raise ValueError(f"expected a (rows, cols) {dtype} image on the GPU with contiguous rows, got {img.dtype} {tuple(img.shape)}")
                args += [C.c_void_p(img.data_ptr()), C.c_int(img.stride(0) * img.element_size())]
            if tuple(img.shape[:2]) != (rows, cols):
                raise ValueError(f"the {name} image must be {rows} x {cols}")
        vn = None if vertex_normals is None else _point_list(vertex_normals, "vertex_normals")
        vc = None
        if vertex_colours is not None:
            if not (vertex_colours.dim() == 2 and vertex_colours.shape[1] == 4):
                raise ValueError("expected (V, 4) uint8 vertex colours")
            vc = _ptr(vertex_colours, torch.uint8)
        for v in (vertex_normals, vertex_colours):
            if v is not None and int(v.shape[0]) != self.n_vertices:
                raise ValueError("one normal / colour per vertex")
        check(_lib.lib().sobfu_hip_mesh_render(*self._target(), vn, vc, Rm, tv, *map(_f, intr[:4]), C.c_int(int(rows)), C.c_int(int(cols)), _f(z_min),
                                               _f(0.0 if z_max is None else z_max), *args, _stream()), "mesh_render")
        return given

    # ---- this mesh, closed, as a signed TSDF volume and an inside / outside test (sobfu_amd/csrc/mesh_voxel_kernels.hip) ----
    def voxelise(self, dims, vs, trunc, eta, out=None, mode="auto", sign="parity", winding_out=None):
        """This mesh, its vertices in the volume's frame, as a TSDF volume of dims = (X, Y, Z) voxels of size vs (3,): voxel (i, j, k) has
        its centre at i vs + vs / 2 per axis; tsdf = clamp(s / trunc, -1, 1) with s the exact distance to the mesh, negative inside;
        weight = s > -eta -> (volume (Z, Y, X, 2) float32, open_rows (1,) int32 GPU tensor: the rows along x that cross the mesh an odd
        number of times -- 0 for a closed mesh).  out: a volume to write into.  mode never changes a bit.  X <= 512.
        sign: "parity" (a closed mesh: inside iff the row crosses it an odd number of times beyond the voxel) or "winding" (any oriented
        mesh, open ones included: inside iff the generalised winding number exceeds 1 / 2; open_rows is then only information).
        winding_out (sign="winding"): a (Z, Y, X) float32 tensor that receives the winding number at every voxel centre."""
        if sign not in ("parity", "winding"):
            raise ValueError(f"unknown sign {sign!r}")
        if winding_out is not None and sign != "winding":
            raise ValueError("winding_out needs sign='winding'")
        mode = self._mode(mode)
        X, Y, Z = (int(d) for d in dims)
        dev = self.vertices.device
        vol = torch.empty((Z, Y, X, 2), dtype=torch.float32, device=dev) if out is None else out
        if tuple(vol.shape) != (Z, Y, X, 2):
            raise ValueError(f"the volume must be {(Z, Y, X, 2)}, got {tuple(vol.shape)}")
        if winding_out is not None and tuple(winding_out.shape) != (Z, Y, X):
            raise ValueError(f"winding_out must be {(Z, Y, X)}, got {tuple(winding_out.shape)}")
        L = _lib.lib()
        # one path; the winding entry point takes the boundary behind the target and winding_out ahead of the stream
        if sign == "winding":
            name, size, fn = "mesh_voxelise_winding", L.sobfu_hip_mesh_voxelise_winding_workspace_bytes, L.sobfu_hip_mesh_voxelise_winding
            boundary, extra = self._boundary_args, (None if winding_out is None else _ptr(winding_out),)
        else:
            name, size, fn = "mesh_voxelise", L.sobfu_hip_mesh_voxelise_workspace_bytes, L.sobfu_hip_mesh_voxelise
            boundary, extra = tuple, ()
        nbytes = int(size(C.c_int(X), C.c_int(Y), C.c_int(Z)))
        if nbytes == 0:
            raise ValueError(f"cannot voxelise into {X} x {Y} x {Z} voxels (X <= 512)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        open_rows = torch.empty(1, dtype=torch.int32, device=dev)
        check(fn(*self._target(), *boundary(), _ptr(vol), C.c_int(X), C.c_int(Y), C.c_int(Z), _vs3(vs), _f(trunc), _f(eta), mode, *_ws(ws),
                 _ptr(open_rows, torch.int32), *extra, _stream()), name)
        return vol, open_rows

    def inside(self, points, mode="auto"):
        """(n, 4) float32 points -> inside (n,) uint8 (1: the row from the point along +x crosses the mesh an odd number of times), open
        (n,) uint8 (1: the point's whole row crosses it an odd number of times: the mesh is not closed there)"""
        mode = self._mode(mode)
        n = int(points.shape[0])
        ins = torch.empty(n, dtype=torch.uint8, device=points.device)
        opn = torch.empty(n, dtype=torch.uint8, device=points.device)
        if n:
            check(_lib.lib().sobfu_hip_mesh_inside(*self._target(), _point_list(points, "points"), C.c_int(n), _ptr(ins, torch.uint8),
                                                   _ptr(opn, torch.uint8), mode, _stream()), "mesh_inside")
        return ins, opn

    def winding(self, points, mode="boundary", walk="auto"):
        """(n, 4) float32 points -> (n,) float32 generalised winding numbers: 1 inside and 0 outside a closed, outward-oriented mesh,
        smooth across the holes of an open one; inside iff > 1 / 2.  mode "boundary": signed row crossings + the solid angles of the
        strips behind the boundary edges (the definition on seam points); "sum": the definition, every triangle's solid angle.
        walk "auto" | "grid" | "brute": the crossing walk, never changes a bit."""
        if mode not in ("boundary", "sum"):
            raise ValueError(f"unknown mode {mode!r}")
        walk = self._mode(walk)
        n = int(points.shape[0])
        w = torch.empty(n, dtype=torch.float32, device=points.device)
        if n:
            check(_lib.lib().sobfu_hip_mesh_winding(*self._target(), *self._boundary_args(), _point_list(points, "points"), C.c_int(n), _ptr(w),
                                                    C.c_int(0 if mode == "boundary" else 1), walk, _stream()), "mesh_winding")
        return w

    def sample(self, density=None, n=None, seed=0, tri=False, bary=False, areas=False):
        """mesh_sample on this grid's own mesh"""
        return mesh_sample(self.vertices, self.faces, density, n, seed, tri, bary, areas)

    def unresolved(self):
        """how many points of the last query hit the ring cap and were finished by brute force (synchronises)"""
        n = C.c_int(0)
        check(_lib.lib().sobfu_hip_mesh_distance_unresolved(_ws(self.workspace)[0], C.byref(n), _stream()), "mesh_distance_unresolved")
        return n.value


def mesh_distance(points, vertices, faces, max_dist=None, closest=False, mode="auto", ring_cap=None, cell=None):
    """TriangleGrid(vertices, faces, cell).query(points, ...) in one call"""
    return TriangleGrid(vertices, faces, cell).query(points, max_dist, closest, mode, ring_cap)


# ---- area-weighted mesh samples and F-score counts (sobfu_amd/csrc/mesh_sample_kernels.hip) -------------------------------
def _mesh_args(vertices, faces):
    _point_list(vertices, "vertices")
    if not (faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError(f"expected (F, 3) int32 faces, got {tuple(faces.shape)}")
    nv, nt = int(vertices.shape[0]), int(faces.shape[0])
    return (_ptr(vertices) if nv else None, C.c_int(nv), _ptr(faces, torch.int32) if nt else None, C.c_int(nt))


def mesh_sample_count(vertices, faces, density, seed=0, areas=False):
    """The count call of mesh_sample on its own -> (rc, total, workspace, areas): sobfu_hip_mesh_sample_count's return code (0, -1 for a
    face index out of range or a non-finite corner, -3 for more than INT32_MAX samples), the 64-bit total, the workspace (a uint8
    tensor, for mesh_sample_generate) and the (F,) float64 areas when asked for.  Synchronises once."""
    L = _lib.lib()
    mesh = _mesh_args(vertices, faces)
    nt = int(faces.shape[0])
    ws = torch.empty(int(L.sobfu_hip_mesh_sample_workspace_bytes(C.c_int(nt))), dtype=torch.uint8, device=vertices.device)
    a = torch.empty(nt, dtype=torch.float64, device=vertices.device) if areas else None
    total = C.c_longlong(0)
    rc = L.sobfu_hip_mesh_sample_count(*mesh, C.c_double(float(density)), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), *_ws(ws),
                                       _ptr(a, torch.float64) if areas and nt else None, C.byref(total), _stream())
    return rc, int(total.value), ws, a


def mesh_sample_generate(vertices, faces, seed, workspace, max_samples, tri=False, bary=False):
    """The generate call of mesh_sample on its own, through the workspace of mesh_sample_count -> (rc, points (max_samples, 4) float32,
    tri (max_samples,) int32 or None, bary (max_samples, 2) float32 or None)"""
    dev, n = vertices.device, int(max_samples)
    p = torch.empty((n, 4), dtype=torch.float32, device=dev)
    t = torch.empty(n, dtype=torch.int32, device=dev) if tri else None
    b = torch.empty((n, 2), dtype=torch.float32, device=dev) if bary else None
    rc = _lib.lib().sobfu_hip_mesh_sample_generate(*_mesh_args(vertices, faces), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), *_ws(workspace),
                                                   _ptr(p) if n else None, _ptr(t, torch.int32) if tri and n else None, _ptr(b) if bary and n else None,
                                                   C.c_int(n), _stream())
    return rc, p, t, b


def mesh_sample(vertices, faces, density=None, n=None, seed=0, tri=False, bary=False, areas=False):
    """Points drawn uniformly per unit area from an indexed mesh (vertices (V, 4) float32, faces (F, 3) int32, GPU tensors) -> points
    (N, 4) float32 (x, y, z, 1) on the GPU [, tri (N,) int32: each sample's triangle] [, bary (N, 2) float32: the weights of that
    triangle's second and third corner] [, areas (F,) float64].  Exactly one of density (samples per unit area) and n is given.
    Triangle t receives floor(area_t density) samples plus one more with probability frac(area_t density), so the total is within the
    number of triangles of density x the mesh's area.  n means density = n / math.fsum(areas): the sample count then lands within that
    spread of n, it is NOT exactly n.  Samples are ordered by triangle; the result depends on the mesh, the density and the seed alone,
    bit for bit (sobfu_amd/csrc/sobfu_mesh_sample.hpp)."""
    import math

    if (density is None) == (n is None):
        raise ValueError("give exactly one of density and n")
    a = None
    if n is not None:
        if int(n) < 0:
            raise ValueError("n >= 0")
        rc, _, _, a = mesh_sample_count(vertices, faces, 0.0, seed, areas=True)
        check(rc, "mesh_sample_count")
        total_area = math.fsum(a.cpu().numpy().tolist())
        density = float(n) / total_area if total_area > 0.0 and int(n) > 0 else 0.0
    if not (math.isfinite(density) and density >= 0.0):
        raise ValueError(f"the density must be finite and >= 0, got {density}")
    rc, total, ws, a2 = mesh_sample_count(vertices, faces, density, seed, areas=areas and a is None)
    check(rc, "mesh_sample_count")
    rc, p, t, b = mesh_sample_generate(vertices, faces, seed, ws, total, tri, bary)
    check(rc, "mesh_sample_generate")
    extras = [x for x, asked in ((t, tri), (b, bary), (a2 if a is None else a, areas)) if asked]
    return (p, *extras) if extras else p


def distance_score(dist, thresholds):
    """(n,) float32 distances on the GPU, up to 16 thresholds (any order) -> (within (K,) int64 numpy: how many distances are finite and
    <= each threshold, finite: how many are finite at all).  NaN and +Inf are never within.  Synchronises to read the counts."""
    th = [float(x) for x in np.asarray(thresholds, np.float64).reshape(-1)]
    if not 1 <= len(th) <= 16:
        raise ValueError("1 to 16 thresholds")
    n = int(dist.numel())
    counts = torch.empty(len(th) + 1, dtype=torch.int64, device=dist.device)
    check(_lib.lib().sobfu_hip_distance_score(_ptr(dist) if n else None, C.c_int(n), (C.c_float * len(th))(*th), C.c_int(len(th)),
                                              _ptr(counts, torch.int64), _stream()), "distance_score")
    c = counts.cpu().numpy()
    return c[:-1].copy(), int(c[-1])


# ---- warp-field diagnostics (sobfu_amd/csrc/warp_stats_kernels.hip) -----------------------------------------------------
# the result block's words (include/sobfu_hip.h, SOBFU_WS_*)
(WS_N_DET, WS_N_FOLD, WS_N_DET_NONFINITE, WS_N_DISP, WS_N_DISP_NONFINITE, WS_N_RES, WS_N_RES_ABOVE, WS_N_RES_OUTSIDE, WS_N_RES_NONFINITE,
 WS_DET_BELOW) = range(10)
(WS_DET_SUM, WS_DISP_SUM, WS_RES_SUM, WS_DET_MIN_KEY, WS_DET_MAX_KEY, WS_DISP_MAX_KEY, WS_RES_MAX_KEY, WS_WORDS) = (25, 27, 29, 31, 32, 33, 34, 64)


def _ws_signed(word):
    word = int(word)
    return word - (1 << 64) if word >> 63 else word


def _ws_mean(words, at, n):
    """(HI 2^24 + LO) 2^-44 / n, in doubles operation by operation (sobfu_amd::WarpStats does the same); NaN for an empty group"""
    if n == 0:
        return float("nan")
    return (float(_ws_signed(words[at])) * 16777216.0 + float(_ws_signed(words[at + 1]))) / 17592186044416.0 / float(n)


def _ws_key(key, maximum, dims):
    """a key of the result block -> (value, (x, y, z)); an empty group: (NaN, (-1, -1, -1))"""
    key = int(key)
    if key == (1 << 64) - 1:
        return float("nan"), (-1, -1, -1)
    o, index = key >> 32, key & 0xFFFFFFFF
    if maximum:
        o = ~o & 0xFFFFFFFF
    b = o ^ 0x80000000 if o & 0x80000000 else ~o & 0xFFFFFFFF
    X, Y, _ = dims
    return float(np.array([b], np.uint32).view(np.float32)[0]), (index % X, (index // X) % Y, index // (X * Y))


@dataclasses.dataclass
class WarpStats:
    """What warp_stats measured, decoded from the 64 words of the result block (`words`, (64,) uint64).  det_* and disp_* cover the voxels
    of `mask`, res_* those of `mask_inv`; lengths are in the units of voxel_size.  An empty group has NaN values and (-1, -1, -1) voxels."""
    dims: tuple
    words: np.ndarray
    edges: tuple
    has_inverse: bool
    n_det: int
    n_fold: int
    n_det_nonfinite: int
    fold_fraction: float
    det_below: tuple  # per edge: the voxels with det < edge
    det_min: float
    det_min_at: tuple
    det_max: float
    det_max_at: tuple
    det_mean: float
    n_disp: int
    n_disp_nonfinite: int
    disp_max: float
    disp_max_at: tuple
    disp_mean: float
    n_res: int
    n_res_above: int
    n_res_outside: int
    n_res_nonfinite: int
    res_max: float
    res_max_at: tuple
    res_mean: float
    det: object = None  # (Z, Y, X) float32 on the GPU with volumes=True
    res: object = None

    @classmethod
    def from_words(cls, words, dims, edges=(), has_inverse=True, det=None, res=None):
        w = np.asarray(words, np.uint64).reshape(WS_WORDS)
        dims = tuple(int(v) for v in dims)
        c = [int(v) for v in w[:WS_DET_BELOW]]
        (det_min, det_min_at), (det_max, det_max_at) = _ws_key(w[WS_DET_MIN_KEY], False, dims), _ws_key(w[WS_DET_MAX_KEY], True, dims)
        (disp_max, disp_max_at), (res_max, res_max_at) = _ws_key(w[WS_DISP_MAX_KEY], True, dims), _ws_key(w[WS_RES_MAX_KEY], True, dims)
        return cls(dims=dims, words=w.copy(), edges=tuple(float(e) for e in edges), has_inverse=bool(has_inverse), n_det=c[WS_N_DET], n_fold=c[WS_N_FOLD],
                   n_det_nonfinite=c[WS_N_DET_NONFINITE], fold_fraction=c[WS_N_FOLD] / c[WS_N_DET] if c[WS_N_DET] else float("nan"),
                   det_below=tuple(int(v) for v in w[WS_DET_BELOW:WS_DET_BELOW + len(edges)]), det_min=det_min, det_min_at=det_min_at, det_max=det_max,
                   det_max_at=det_max_at, det_mean=_ws_mean(w, WS_DET_SUM, c[WS_N_DET]), n_disp=c[WS_N_DISP], n_disp_nonfinite=c[WS_N_DISP_NONFINITE],
                   disp_max=disp_max, disp_max_at=disp_max_at, disp_mean=_ws_mean(w, WS_DISP_SUM, c[WS_N_DISP]), n_res=c[WS_N_RES],
                   n_res_above=c[WS_N_RES_ABOVE], n_res_outside=c[WS_N_RES_OUTSIDE], n_res_nonfinite=c[WS_N_RES_NONFINITE], res_max=res_max,
                   res_max_at=res_max_at, res_mean=_ws_mean(w, WS_RES_SUM, c[WS_N_RES]), det=det, res=res)

    def line(self, frame):
        """the line apps/sobfu_headless prints with --warp-stats (floats as %.9g: they round-trip)"""
        def g(v):
            return "nan" if v != v else "%.9g" % v

        s = "warp %d: voxels=%d det min=%s @%d,%d,%d max=%s mean=%s folds=%d (%s%%) disp max=%s mean=%s" % (
            frame, self.n_det, g(self.det_min), *self.det_min_at, g(self.det_max), g(self.det_mean), self.n_fold, g(100.0 * self.fold_fraction),
            g(self.disp_max), g(self.disp_mean))
        if self.has_inverse:
            s += " inv res max=%s @%d,%d,%d mean=%s above=%d outside=%d" % (g(self.res_max), *self.res_max_at, g(self.res_mean), self.n_res_above,
                                                                          self.n_res_outside)
        return s


def warp_stats(psi, psi_inv=None, mask=None, mask_inv=None, voxel_size=(1.0, 1.0, 1.0), band=1.0, edges=(0, .25, .5, 1, 2, 4), res_tol=None, volumes=False,
               result=None):
    """Diagnostics of the deformation psi in one pass -> WarpStats: det J (min / max with their voxels, mean, folds det <= 0, the counts
    below each of up to 16 ascending `edges`), the displacement |psi - id| (max, mean) and, with psi_inv, the residual |psi(psi_inv(x)) - x|
    (max with its voxel, mean, the counts above res_tol, outside the volume and non-finite); lengths in the units of voxel_size.
    mask / mask_inv: TSDF volumes; only voxels with weight > 0 and |tsdf| < band count in the det and displacement / the residual group
    (meant: phi_global / phi_global o psi_inv).  res_tol: default a tenth of the smallest voxel side.  volumes: also the per-voxel det
    and residual, (Z, Y, X) float32 on the GPU (every voxel, masked or not).  result: a (64,) int64 GPU tensor to reuse, cleared or not.
    Every figure is an exact integer sum or minimum: the same bits from run to run (the rules: sobfu_amd/csrc/sobfu_warp_stats.hpp).
    Swapping psi and psi_inv measures psi_inv o psi.  Synchronises to read the result."""
    vs = [float(np.float32(v)) for v in voxel_size]  # as the kernel takes them: the default res_tol is the C++ twin's, bit for bit
    ed = [float(e) for e in edges]
    if len(ed) > 16:
        raise ValueError("at most 16 edges")
    if psi_inv is None and mask_inv is not None:
        raise ValueError("mask_inv needs psi_inv")
    for t, last in ((psi_inv, 4), (mask, 2), (mask_inv, 2)):
        if t is not None and tuple(t.shape) != tuple(psi.shape[:3]) + (last,):
            raise ValueError(f"expected a {tuple(psi.shape[:3]) + (last,)} tensor, got {tuple(t.shape)}")
    Z, Y, X = psi.shape[:3]
    tol = 0.1 * min(vs) if res_tol is None else float(res_tol)
    words = torch.empty(WS_WORDS, dtype=torch.int64, device=psi.device) if result is None else result
    det = torch.empty((Z, Y, X), dtype=torch.float32, device=psi.device) if volumes else None
    res = torch.empty((Z, Y, X), dtype=torch.float32, device=psi.device) if volumes and psi_inv is not None else None

    def opt(t):
        return None if t is None else _ptr(t)

    check(_lib.lib().sobfu_hip_warp_stats(_ptr(psi), opt(psi_inv), opt(mask), opt(mask_inv), *_xyz(psi), _F3(*vs), _f(band),
                                          (C.c_float * len(ed))(*ed) if ed else None, C.c_int(len(ed)), _f(tol), _ptr(words, torch.int64), opt(det), opt(res),
                                          _stream()), "warp_stats")
    return WarpStats.from_words(words.cpu().numpy().view(np.uint64), (X, Y, Z), ed, psi_inv is not None, det, res)


# ---- camera tracking (sobfu_amd/csrc/icp_kernels.hip): projective ICP and its image pyramids -------------------------------------
class IcpLevel(C.Structure):
    """sobfu_hip_icp_level"""
    _fields_ = [("curr", C.c_void_p), ("curr_step", C.c_int), ("ncurr", C.c_void_p), ("ncurr_step", C.c_int), ("prev", C.c_void_p),
                ("prev_step", C.c_int), ("nprev", C.c_void_p), ("nprev_step", C.c_int), ("rows", C.c_int), ("cols", C.c_int)]


def _depth_image(t):
    if not (t.is_cuda and t.dim() == 2 and t.dtype in (torch.int16, torch.uint16) and t.stride(1) == 1):
        raise ValueError("depth images must be (rows, cols) 16-bit tensors on the GPU with contiguous rows")
    return C.c_void_p(t.data_ptr()), C.c_int(t.stride(0) * 2)


def depth_pyramid(depth, sigma_depth, out=None):
    """depthBuildPyramid: (rows, cols) -> (rows // 2, cols // 2) uint16 (as int16) depth; sigma_depth in metres"""
    rows, cols = depth.shape
    if out is None:
        out = torch.empty((rows // 2, cols // 2), dtype=depth.dtype, device=depth.device)
    check(_lib.lib().sobfu_hip_depth_pyramid(*_depth_image(depth), C.c_int(rows), C.c_int(cols), *_depth_image(out), _f(sigma_depth), _stream()),
          "depth_pyramid")
    return out


def point_normals(depth, intr, points=None, normals=None):
    """computePointNormals -> (points, normals), (rows, cols, 4) float32 in the camera frame; invalid pixels are NaN"""
    rows, cols = depth.shape
    points = torch.empty((rows, cols, 4), dtype=torch.float32, device=depth.device) if points is None else points
    normals = torch.empty((rows, cols, 4), dtype=torch.float32, device=depth.device) if normals is None else normals
    check(_lib.lib().sobfu_hip_compute_point_normals(*_depth_image(depth), C.c_int(rows), C.c_int(cols), _f(intr[0]), _f(intr[1]), _f(intr[2]),
                                                     _f(intr[3]), *_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4),
                                                     _stream()), "point_normals")
    return points, normals


def normals_mask_depth(depth, intr, normals=None):
    """computeNormalsAndMaskDepth: normals of `depth`; `depth` is zeroed in place where the normal is NaN"""
    rows, cols = depth.shape
    normals = torch.empty((rows, cols, 4), dtype=torch.float32, device=depth.device) if normals is None else normals
    check(_lib.lib().sobfu_hip_compute_normals_mask_depth(*_depth_image(depth), C.c_int(rows), C.c_int(cols), _f(intr[0]), _f(intr[1]), _f(intr[2]),
                                                          _f(intr[3]), *_image_ptr(normals, torch.float32, 4), _stream()), "normals_mask_depth")
    return normals


def resize_depth_normals(depth, normals, depth_out=None, normals_out=None):
    """resizeDepthNormals: half resolution of (depth, normals); `depth_out` / `normals_out` may be given to write into existing buffers"""
    rows, cols = depth.shape
    d = torch.empty((rows // 2, cols // 2), dtype=depth.dtype, device=depth.device) if depth_out is None else depth_out
    n = torch.empty((rows // 2, cols // 2, 4), dtype=torch.float32, device=depth.device) if normals_out is None else normals_out
    if tuple(d.shape) != (rows // 2, cols // 2) or tuple(n.shape) != (rows // 2, cols // 2, 4):
        raise ValueError(f"the outputs of a ({rows}, {cols}) image must be ({rows // 2}, {cols // 2}) and ({rows // 2}, {cols // 2}, 4)")
    check(_lib.lib().sobfu_hip_resize_depth_normals(*_depth_image(depth), *_image_ptr(normals, torch.float32, 4), C.c_int(rows), C.c_int(cols),
                                                    *_depth_image(d), *_image_ptr(n, torch.float32, 4), _stream()), "resize_depth_normals")
    return d, n


def resize_points_normals(points, normals, points_out=None, normals_out=None):
    """resizePointsNormals: half resolution of (points, normals); an output pixel is valid iff its four source pixels are.
    `points_out` / `normals_out` may be given to write into existing buffers"""
    rows, cols = points.shape[:2]
    p = torch.empty((rows // 2, cols // 2, 4), dtype=torch.float32, device=points.device) if points_out is None else points_out
    n = torch.empty((rows // 2, cols // 2, 4), dtype=torch.float32, device=points.device) if normals_out is None else normals_out
    if tuple(p.shape) != (rows // 2, cols // 2, 4) or tuple(n.shape) != (rows // 2, cols // 2, 4):
        raise ValueError(f"the outputs of a ({rows}, {cols}) image must be ({rows // 2}, {cols // 2}, 4)")
    check(_lib.lib().sobfu_hip_resize_points_normals(*_image_ptr(points, torch.float32, 4), *_image_ptr(normals, torch.float32, 4), C.c_int(rows),
                                                     C.c_int(cols), *_image_ptr(p, torch.float32, 4), *_image_ptr(n, torch.float32, 4), _stream()),
          "resize_points_normals")
    return p, n


def _icp_level(curr, ncurr, prev, nprev):
    depth = curr.dim() == 2
    if depth:
        c, p = _depth_image(curr), _depth_image(prev)
    else:
        c, p = _image_ptr(curr, torch.float32, 4), _image_ptr(prev, torch.float32, 4)
    if tuple(curr.shape[:2]) != tuple(prev.shape[:2]) or tuple(ncurr.shape[:2]) != tuple(curr.shape[:2]) or tuple(nprev.shape[:2]) != tuple(curr.shape[:2]):
        raise ValueError("the current and previous images of a level must have the same size")
    return IcpLevel(c[0], c[1], *_image_ptr(ncurr, torch.float32, 4), p[0], p[1], *_image_ptr(nprev, torch.float32, 4), curr.shape[0], curr.shape[1]), depth


class ICP:
    """kfusion::cuda::ProjectiveICP on the device: owns the workspace, the pose and the status word.  Angles in radians.
    estimate() enqueues the whole coarse-to-fine loop and synchronises once (to read the result); enqueue() does not synchronise."""

    def __init__(self, dist_thres=0.1, angle_thres=np.deg2rad(20.0), iters=(10, 5, 4, 0), device="cuda"):
        _require_gpu()
        self.dist_thres, self.angle_thres = float(dist_thres), float(angle_thres)
        self.iters = (list(iters) + [0, 0, 0, 0])[:4]
        self.workspace = torch.empty(int(_lib.lib().sobfu_hip_icp_workspace_bytes()), dtype=torch.uint8, device=device)
        self.pose = torch.empty(16, dtype=torch.float32, device=device)
        self.status = torch.empty(1, dtype=torch.int32, device=device)
        self.trace = torch.zeros(2 * sum(self.iters), dtype=torch.float32, device=device)

    def used_levels(self):
        """getUsedLevelsNum: the finest-to-coarsest count up to the last level with iterations"""
        n = 4
        while n > 0 and self.iters[n - 1] == 0:
            n -= 1
        return n

    def enqueue(self, intr, curr, ncurr, prev, nprev):
        """curr / prev: lists (finest first) of (rows, cols, 4) points or (rows, cols) depth; ncurr / nprev: the normals"""
        n = self.used_levels()
        if n < 1 or min(len(curr), len(ncurr), len(prev), len(nprev)) < n:
            raise ValueError(f"{n} pyramid levels needed")
        lv = [_icp_level(curr[i], ncurr[i], prev[i], nprev[i]) for i in range(n)]
        if len({d for _, d in lv}) != 1:
            raise ValueError("all levels must be points or all depth")
        arr = (IcpLevel * n)(*[l for l, _ in lv])
        check(_lib.lib().sobfu_hip_icp_estimate(arr, C.c_int(n), (C.c_int * 4)(*self.iters), C.c_int(1 if lv[0][1] else 0), _f(intr[0]), _f(intr[1]),
                                                _f(intr[2]), _f(intr[3]), _f(self.dist_thres), _f(self.angle_thres), _ptr(self.workspace, torch.uint8),
                                                C.c_size_t(self.workspace.numel()), _ptr(self.pose), _ptr(self.status, torch.int32), _ptr(self.trace),
                                                _stream()), "icp_estimate")

    def estimate(self, intr, curr, ncurr, prev, nprev):
        """-> (ok, 4 x 4 float32 numpy pose mapping the current frame into the previous one)"""
        self.enqueue(intr, curr, ncurr, prev, nprev)
        return int(self.status.item()) == 0, self.pose.cpu().numpy().reshape(4, 4)

    def failure(self):
        """(level, iteration) of the failed solve, or None"""
        s = int(self.status.item())
        return None if s == 0 else ((s >> 8) & 0xFF, s & 0xFF)


def icp_estimate(intr, curr, ncurr, prev, nprev, dist_thres=0.1, angle_thres=np.deg2rad(20.0), iters=(10, 5, 4, 0)):
    """ProjectiveICP::estimateTransform on pyramids (lists, finest first) -> (ok, 4 x 4 pose: current frame -> previous frame)"""
    return ICP(dist_thres, angle_thres, iters).estimate(intr, curr, ncurr, prev, nprev)


def icp_step(level_index, intr, curr, ncurr, prev, nprev, aff, dist_thres=0.1, angle_thres=np.deg2rad(20.0), codes=False, workspace=None):
    """One correspondence + reduction pass of pyramid level `level_index` (base intrinsics intr) at the 4 x 4 pose `aff` ->
    (A 6 x 6, b (6,), inlier count, rms residual, code map (rows, cols) uint8 or None), float64 numpy.  `codes` may also be a
    (rows, cols) uint8 tensor on the GPU with contiguous rows (any row stride) to write the code map into."""
    lvl, depth = _icp_level(curr, ncurr, prev, nprev)
    dev = curr.device
    aff_d = torch.as_tensor(np.asarray(aff, np.float32).reshape(16), device=dev)
    ws = torch.empty(int(_lib.lib().sobfu_hip_icp_workspace_bytes()), dtype=torch.uint8, device=dev) if workspace is None else workspace
    sums = torch.empty(29, dtype=torch.float64, device=dev)
    if isinstance(codes, torch.Tensor):
        cm = codes
        if not (cm.is_cuda and cm.dtype == torch.uint8 and tuple(cm.shape) == tuple(curr.shape[:2]) and cm.stride(1) == 1):
            raise ValueError("the code map must be a (rows, cols) uint8 tensor on the GPU with contiguous rows")
    else:
        cm = torch.empty(tuple(curr.shape[:2]), dtype=torch.uint8, device=dev) if codes else None
    check(_lib.lib().sobfu_hip_icp_step(C.byref(lvl), C.c_int(int(level_index)), C.c_int(1 if depth else 0), _f(intr[0]), _f(intr[1]), _f(intr[2]),
                                        _f(intr[3]), _f(dist_thres), _f(angle_thres), _ptr(aff_d), _ptr(ws, torch.uint8), C.c_size_t(ws.numel()),
                                        _ptr(sums, torch.float64), None if cm is None else C.c_void_p(cm.data_ptr()),
                                        C.c_int(0 if cm is None else cm.stride(0)), _stream()), "icp_step")
    s = sums.cpu().numpy()
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    count = s[27]
    rms = float(np.sqrt(s[28] / count)) if count > 0 else 0.0
    return A, s[21:27].copy(), int(count), rms, None if cm is None else cm.cpu().numpy()
