"""Reconstruction error against a ground-truth mesh: exact vertex-to-surface distances in both directions (ops.TriangleGrid, the
kernels of sobfu_amd/csrc/mesh_distance_kernels.hip) and their statistics, as in the SobolevFusion / KillingFusion evaluations.  The
Python twin of sobfu_amd::compare_meshes (include/sobfu_amd/evaluate.hpp)."""
from __future__ import annotations

import numpy as np


def distance_stats(dist):
    """float32 distances (+Inf = no match within max_dist) -> dict(n, within, mean, rms, median, max): float64 statistics over the finite
    ones; all 0 when there is none.  The median of an even count is the mean of the two middle values."""
    d = np.asarray(dist.detach().cpu().numpy() if hasattr(dist, "detach") else dist).astype(np.float64).ravel()
    f = d[np.isfinite(d)]
    if f.size == 0:
        return dict(n=int(d.size), within=0, mean=0.0, rms=0.0, median=0.0, max=0.0)
    return dict(n=int(d.size), within=int(f.size), mean=float(f.mean()), rms=float(np.sqrt((f * f).mean())), median=float(np.median(f)),
                max=float(f.max()))


def device_tensor(a, dtype):
    """a tensor or array -> a contiguous tensor of `dtype` on the GPU"""
    import torch

    if not hasattr(a, "detach"):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device="cuda", dtype=dtype).contiguous()


def compare_meshes(a_vertices, a_faces, b_vertices, b_faces, max_dist=None, return_distances=False):
    """Two indexed meshes (vertices (V, 4) float32, faces (F, 3) int32; tensors or arrays) -> dict(a_to_b, b_to_a: the statistics of
    distance_stats over the distances from each vertex of one mesh to the surface of the other; chamfer: the mean of the two means;
    hausdorff: the larger of the two maxima).  Vertices farther than max_dist have no match and count in n only.
    return_distances: -> (dict, a_to_b distances, b_to_a distances) (float32 GPU tensors)."""
    import torch

    from . import ops

    av, bv = device_tensor(a_vertices, torch.float32), device_tensor(b_vertices, torch.float32)
    af, bf = device_tensor(a_faces, torch.int32), device_tensor(b_faces, torch.int32)
    d_ab = ops.TriangleGrid(bv, bf).query(av, max_dist)[0]
    d_ba = ops.TriangleGrid(av, af).query(bv, max_dist)[0]
    ab, ba = distance_stats(d_ab), distance_stats(d_ba)
    out = dict(a_to_b=ab, b_to_a=ba, chamfer=0.5 * (ab["mean"] + ba["mean"]), hausdorff=max(ab["max"], ba["max"]))
    return (out, d_ab, d_ba) if return_distances else out


STAT_FIELDS = ("n", "within", "mean", "rms", "median", "max")


def format_result(r):
    """the app's printed form: every field at %.9g, a_to_b and b_to_a prefixed"""
    parts = [f"{side}.{k}={r[side][k]:.9g}" for side in ("a_to_b", "b_to_a") for k in STAT_FIELDS]
    return " ".join(parts + [f"chamfer={r['chamfer']:.9g}", f"hausdorff={r['hausdorff']:.9g}"])
