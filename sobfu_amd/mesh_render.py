"""Depth and colour frames of a triangle mesh, rendered on the GPU by ops.TriangleGrid.render (sobfu_amd/csrc/mesh_ray_kernels.hip): the
mesh-driven twins of synthetic.render_sphere_depth / render_textured_sphere_colour.  What they return feeds SobFusion as those do.

pose = (R, t) takes the mesh's frame to the camera frame (the pose argument of ops.raycast); None: the mesh is in the camera frame.
The meshes the project writes and evaluates against -- marching cubes, --evaluate, SobFusion.evaluate -- are in the camera frame with y
and z negated, (x, -y, -z): MESH_FRAME is the pose that renders those."""
from __future__ import annotations

import numpy as np
import torch

MESH_FRAME = (np.diag([1.0, -1.0, -1.0]).astype(np.float32), np.zeros(3, np.float32))


def _mesh(vertices, faces):
    v = torch.as_tensor(np.ascontiguousarray(vertices, np.float32) if isinstance(vertices, np.ndarray) else vertices)
    f = torch.as_tensor(np.ascontiguousarray(faces, np.int32) if isinstance(faces, np.ndarray) else faces)
    if v.dim() != 2 or v.shape[1] not in (3, 4):
        raise ValueError(f"expected (V, 3) or (V, 4) vertices, got {tuple(v.shape)}")
    if v.shape[1] == 3:
        v = torch.cat([v, torch.ones((v.shape[0], 1), dtype=v.dtype, device=v.device)], 1)
    return v.to(device="cuda", dtype=torch.float32).contiguous(), f.to(device="cuda", dtype=torch.int32).contiguous()


def mesh_grid(vertices, faces):
    """vertices (V, 3 | 4) and faces (F, 3), numpy arrays or tensors -> an ops.TriangleGrid on the GPU: build it once per mesh and use it
    for rendering (grid=...) and for distance queries alike"""
    from . import ops

    return ops.TriangleGrid(*_mesh(vertices, faces))


def render_mesh_depth(vertices, faces, intr, rows=480, cols=640, pose=None, grid=None, sensor=None, seed=0, frame=0):
    """uint16 millimetre depth image (numpy) of the mesh seen by the pinhole camera intr = (fx, fy, cx, cy): pixel (u, v) casts
    ((u - cx) / fx, (v - cy) / fy, 1); depth = z of the nearest triangle the ray meets, rounded (half to even) to millimetres; 0 where
    the ray misses.  grid: a TriangleGrid of this mesh (mesh_grid) to reuse.  sensor: an ops.SensorModel -- the frame that depth
    sensor would report of the rendered points and normals (ops.depth_sensor with this seed and frame number) instead of the clean one."""
    g = mesh_grid(vertices, faces) if grid is None else grid
    if sensor is not None:
        from . import ops

        r = g.render(intr, rows, cols, pose=pose, outputs=("points", "normals"))
        d = ops.depth_sensor(r["points"], r["normals"], sensor, seed, frame)
    else:
        d = g.render(intr, rows, cols, pose=pose, outputs=("depth",))["depth"]
    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.uint16)


def render_mesh_colour(vertices, faces, colours, intr, rows=480, cols=640, pose=None, grid=None):
    """(rows, cols, 4) uint8 BGRA colour frame (numpy) of the mesh of render_mesh_depth with per-vertex BGRA `colours` (V, 4) uint8: a
    pixel that hits takes the barycentric mix of its triangle's corner colours, alpha 255; a miss is (0, 0, 0, 0)."""
    g = mesh_grid(vertices, faces) if grid is None else grid
    c = torch.as_tensor(np.ascontiguousarray(colours, np.uint8) if isinstance(colours, np.ndarray) else colours).to(device="cuda", dtype=torch.uint8)
    img = g.render(intr, rows, cols, pose=pose, vertex_colours=c.contiguous(), outputs=("colour",))["colour"]
    torch.cuda.synchronize()
    return img.cpu().numpy()
