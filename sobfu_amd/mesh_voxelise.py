"""A closed triangle mesh as a full 3-D signed TSDF volume, on the GPU by ops.TriangleGrid.voxelise (sobfu_amd/csrc/mesh_voxel_kernels.hip):
the sensor-free twin of rendering the mesh to a depth frame (mesh_render.render_mesh_depth) and integrating that.  What it returns is a
phi_n as integrate_depth makes one, but two-sided: exact distances and signs on both sides of the surface.

pose = (R, t) takes the mesh's frame to the camera frame, as in mesh_render (MESH_FRAME: the meshes the project writes and evaluates
against); params["R"], params["t"] place the volume in the camera frame (a voxel centre v is seen at R v + t)."""
from __future__ import annotations

import numpy as np
import torch

from .mesh_render import MESH_FRAME, _mesh

# The grid's cell edge in voxels: half a brick.  Measured on config 3's volume against 1.3, 8 and 16 voxels (profiles/mesh_voxelise.md); a
# cell as large as the truncation distance, 48 voxels there, makes every brick gather most of the mesh.
CELL_IN_VOXELS = 4.0


def mesh_to_volume_frame(vertices, params, pose=MESH_FRAME):
    """(V, 3 | 4) vertices in the mesh frame -> (V, 4) float32 numpy vertices in the volume's frame: mesh -> camera by `pose`, camera ->
    volume by the inverse of (params["R"], params["t"]), composed in float64 and applied once per vertex in float64"""
    v = vertices.detach().cpu().numpy() if hasattr(vertices, "detach") else np.asarray(vertices)
    Rp, tp = (np.eye(3), np.zeros(3)) if pose is None else (np.asarray(pose[0], np.float64).reshape(3, 3), np.asarray(pose[1], np.float64).reshape(3))
    Rv, tv = np.asarray(params["R"], np.float64).reshape(3, 3), np.asarray(params["t"], np.float64).reshape(3)
    M, m = Rv.T @ Rp, Rv.T @ (tp - tv)
    out = np.ones((len(v), 4), np.float32)
    out[:, :3] = v[:, :3].astype(np.float64) @ M.T + m
    return out


def mesh_to_tsdf(vertices, faces, params, pose=MESH_FRAME, out=None, cell=None, mode="auto", return_grid=False, sign="parity"):
    """vertices (V, 3 | 4) and faces (F, 3), numpy arrays or tensors, in the mesh frame -> (phi (Z, Y, X, 2) float32 GPU tensor of the
    volume of `params` (dims, vs, trunc, eta), open_rows (1,) int32 GPU tensor: 0 for a closed mesh).  The vertices are transformed once
    and the triangle grid is built with a cell edge of `cell` (None: CELL_IN_VOXELS voxels).  out: a volume to
    write into.  return_grid: -> (phi, open_rows, grid), the ops.TriangleGrid of the transformed mesh (in the VOLUME's frame).
    sign: "parity" (closed meshes) or "winding" (any oriented mesh: inside iff its generalised winding number exceeds 1 / 2)."""
    from . import ops

    trunc = float(params["trunc"])
    v, f = _mesh(mesh_to_volume_frame(vertices, params, pose), faces)
    grid = ops.TriangleGrid(v, f, cell=CELL_IN_VOXELS * float(max(params["vs"])) if cell is None else float(cell))
    phi, open_rows = grid.voxelise(params["dims"], tuple(float(x) for x in params["vs"]), trunc, float(params["eta"]), out=out, mode=mode, sign=sign)
    return (phi, open_rows, grid) if return_grid else (phi, open_rows)
