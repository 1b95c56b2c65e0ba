"""Mesh files of the indexed marching-cubes path (ops.marching_cubes_indexed): binary little-endian PLY 1.0, byte for byte what
sobfu_amd::write_ply (include/sobfu_amd/sobfu.hpp) writes."""
from __future__ import annotations

import numpy as np


def _host(a, dtype):
    if a is None:
        return None
    if hasattr(a, "detach"):  # a torch tensor, on the GPU or not
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype)


def write_ply(path, vertices, normals, faces, colours=None):
    """vertices / normals (V, 4) float32 (x, y, z, w), faces (F, 3) int32, colours (V, 4) uint8 BGRA or None -> PLY with vertex
    (float x y z nx ny nz [uchar red green blue]) and face (list uchar int vertex_indices)"""
    v, n, f, c = _host(vertices, np.float32), _host(normals, np.float32), _host(faces, np.int32), _host(colours, np.uint8)
    V, Fn = len(v), len(f)
    if n.shape != (V, 4) or v.shape != (V, 4) or f.shape != (Fn, 3):
        raise ValueError(f"expected vertices / normals (V, 4) and faces (F, 3), got {v.shape} {n.shape} {f.shape}")
    coloured = c is not None and len(c) > 0
    if coloured and c.shape != (V, 4):
        raise ValueError(f"expected colours (V, 4), got {c.shape}")
    props = "".join(f"property float {p}\n" for p in ("x", "y", "z", "nx", "ny", "nz"))
    if coloured:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {V}\n{props}"
              f"element face {Fn}\nproperty list uchar int vertex_indices\nend_header\n")
    vt = [(p, "<f4") for p in ("x", "y", "z", "nx", "ny", "nz")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if coloured else [])
    rec = np.zeros(V, np.dtype(vt))
    for k, p in enumerate(("x", "y", "z")):
        rec[p] = v[:, k]
        rec["n" + p] = n[:, k]
    if coloured:
        rec["red"], rec["green"], rec["blue"] = c[:, 2], c[:, 1], c[:, 0]
    fr = np.zeros(Fn, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    fr["n"] = 3
    fr["i"] = f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(fr.tobytes())
