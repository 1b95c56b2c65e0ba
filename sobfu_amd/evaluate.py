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


def signed_stats(dist, inside, open_):
    """the signed fields of one direction: signed_mean (float64 mean over the finite distances, each negative where its vertex is inside
    the other mesh), inside (how many of those vertices are inside), open (how many of ALL the vertices lie on a row that crosses the
    other mesh an odd number of times: it is not closed there and their sign means nothing)"""
    d = dist.detach().cpu().numpy().astype(np.float64).ravel()
    i, o = inside.detach().cpu().numpy().astype(bool).ravel(), open_.detach().cpu().numpy().astype(bool).ravel()
    f = np.isfinite(d)
    if not f.any():
        return dict(signed_mean=0.0, inside=0, open=int(o.sum()))
    return dict(signed_mean=float(np.where(i[f], -d[f], d[f]).mean()), inside=int(i[f].sum()), open=int(o.sum()))


def compare_meshes(a_vertices, a_faces, b_vertices, b_faces, max_dist=None, return_distances=False, signed=False):
    """Two indexed meshes (vertices (V, 4) float32, faces (F, 3) int32; tensors or arrays) -> dict(a_to_b, b_to_a: the statistics of
    distance_stats over the distances from each vertex of one mesh to the surface of the other; chamfer: the mean of the two means;
    hausdorff: the larger of the two maxima).  Vertices farther than max_dist have no match and count in n only.
    return_distances: -> (dict, a_to_b distances, b_to_a distances) (float32 GPU tensors).
    signed: each direction gains the fields of signed_stats -- the sign is that of the query vertex against the OTHER mesh
    (ops.TriangleGrid.inside), which should be closed: a_to_b.signed_mean > 0 says mesh a lies outside b on average (inflated).  The
    unsigned fields are the same with and without.
    signed="winding": the sign is that of the other mesh's generalised winding number (ops.TriangleGrid.winding: inside iff > 1 / 2),
    which is defined for open meshes too; `open` still counts the vertices on rows the other mesh crosses an odd number of times."""
    import torch

    from . import ops

    av, bv = device_tensor(a_vertices, torch.float32), device_tensor(b_vertices, torch.float32)
    af, bf = device_tensor(a_faces, torch.int32), device_tensor(b_faces, torch.int32)
    gb, ga = ops.TriangleGrid(bv, bf), ops.TriangleGrid(av, af)
    d_ab = gb.query(av, max_dist)[0]
    d_ba = ga.query(bv, max_dist)[0]
    ab, ba = distance_stats(d_ab), distance_stats(d_ba)
    if signed == "winding":
        ab.update(signed_stats(d_ab, gb.winding(av) > 0.5, gb.inside(av)[1]))
        ba.update(signed_stats(d_ba, ga.winding(bv) > 0.5, ga.inside(bv)[1]))
    elif signed:
        ab.update(signed_stats(d_ab, *gb.inside(av)))
        ba.update(signed_stats(d_ba, *ga.inside(bv)))
    out = dict(a_to_b=ab, b_to_a=ba, chamfer=0.5 * (ab["mean"] + ba["mean"]), hausdorff=max(ab["max"], ba["max"]))
    return (out, d_ab, d_ba) if return_distances else out


STAT_FIELDS = ("n", "within", "mean", "rms", "median", "max")


SIGNED_FIELDS = ("signed_mean", "inside", "open")


def format_result(r):
    """the app's printed form: every field at %.9g, a_to_b and b_to_a prefixed; the signed fields follow each side's where present"""
    parts = [f"{side}.{k}={r[side][k]:.9g}" for side in ("a_to_b", "b_to_a") for k in STAT_FIELDS + SIGNED_FIELDS if k in r[side]]
    return " ".join(parts + [f"chamfer={r['chamfer']:.9g}", f"hausdorff={r['hausdorff']:.9g}"])


# ---- automatic rigid alignment of the ground truth (ops.TriangleGrid.align, sobfu_amd/csrc/mesh_align_kernels.hip) ----------------------
def rigid_inverse(pose):
    """the inverse of a rigid 4 x 4 float32 pose, in the operation order of sobfu_amd/csrc/sobfu_rigid.hpp: R^T, and
    t' = (float32) -((P_0r P_03 + P_1r P_13) + P_2r P_23) in float64"""
    P = np.asarray(pose, np.float32).reshape(4, 4)
    D = P.astype(np.float64)
    out = np.zeros((4, 4), np.float32)
    out[:3, :3] = P[:3, :3].T
    for r in range(3):
        out[r, 3] = np.float32(-((D[0, r] * D[0, 3] + D[1, r] * D[1, 3]) + D[2, r] * D[2, 3]))
    out[3, 3] = 1
    return out


def align_meshes(model_vertices, gt_vertices, gt_faces, pose=None, iters=30, max_dist=None, dof=6, eps_rot=0.0, eps_trans=0.0):
    """Refines the pose that carries a ground-truth mesh into the model's frame: point-to-plane ICP of the model's vertices (the source: a
    partial surface, every point of which has a counterpart) against the ground-truth mesh (the target: complete; its grid is built
    once).  pose: the caller's ground-truth-to-model guess (None: the identity); its rigid inverse starts the loop, and the rigid
    inverse of the result is returned -> (pose (4, 4) float32 numpy, to apply to the ground truth, info of ops.TriangleGrid.align).
    ICP needs a start within its basin: this is a refinement, not a global registration."""
    import torch

    from . import ops

    mv, gv = device_tensor(model_vertices, torch.float32), device_tensor(gt_vertices, torch.float32)
    gf = device_tensor(gt_faces, torch.int32)
    start = None if pose is None else rigid_inverse(pose)
    found, info = ops.TriangleGrid(gv, gf).align(mv, start, iters, max_dist, dof, eps_rot, eps_trans)
    return rigid_inverse(found.cpu().numpy()), info


def format_alignment(info, pose):
    """the app's printed form: status, iterations, the inliers and rms residual of the last iteration that ran, the 16 pose numbers at %.9g"""
    last = info["trace"][-1] if len(info["trace"]) else (0.0, 0.0)
    return "status=0x%x iterations=%d inliers=%d rms=%.9g pose=%s" % (info["status"], info["iterations"], int(last[0]), float(last[1]),
                                                                   ",".join("%.9g" % float(v) for v in np.asarray(pose, np.float32).reshape(16)))


# ---- precision, recall and F-score over area-weighted samples (ops.mesh_sample, ops.distance_score) -----------------------
def f_score(a_vertices, a_faces, b_vertices, b_faces, thresholds, density=None, n=None, seed=0, max_dist=None):
    """Two indexed meshes, a = the model and b = the ground truth, each sampled uniformly per unit area at the same density (exactly one
    of density, in samples per square metre, and n is given; n: the density is n over the larger of the two areas), a with the draws of
    `seed` and b with those of seed + 1.  Each sample set is sent to the other mesh's surface (ops.TriangleGrid.query) and scored against
    the thresholds (metres, up to 16, any order) -> dict(thresholds; precision, recall, f: lists, one entry per threshold -- the share of
    a's samples within tau of b, of b's samples within tau of a, and 2 P R / (P + R), 0 when P + R = 0; a_samples, b_samples: the two
    counts; a_to_b, b_to_a: distance_stats of the sampled distances; chamfer, hausdorff: as in compare_meshes, now weighted by area).
    The denominators are all the samples: one farther than max_dist has no match and is a miss.  A side without samples scores 0."""
    import math

    import torch

    from . import ops

    if (density is None) == (n is None):
        raise ValueError("give exactly one of density and n")
    th = [float(np.float32(t)) for t in np.asarray(thresholds, np.float64).reshape(-1)]  # as the kernel compares them
    av, bv = device_tensor(a_vertices, torch.float32), device_tensor(b_vertices, torch.float32)
    af, bf = device_tensor(a_faces, torch.int32), device_tensor(b_faces, torch.int32)
    ga, gb = ops.TriangleGrid(av, af), ops.TriangleGrid(bv, bf)
    if n is not None:
        areas = []
        for v, f in ((av, af), (bv, bf)):
            rc, _, _, a = ops.mesh_sample_count(v, f, 0.0, 0, areas=True)
            ops.check(rc, "mesh_sample_count")
            areas.append(math.fsum(a.cpu().numpy().tolist()))
        density = float(n) / max(areas) if max(areas) > 0.0 else 0.0
    pa, pb = ga.sample(density=density, seed=seed), gb.sample(density=density, seed=int(seed) + 1)
    d_ab, d_ba = gb.query(pa, max_dist)[0], ga.query(pb, max_dist)[0]
    (wa, _), (wb, _) = ops.distance_score(d_ab, th), ops.distance_score(d_ba, th)
    na, nb = int(pa.shape[0]), int(pb.shape[0])
    precision = [int(w) / na if na else 0.0 for w in wa]
    recall = [int(w) / nb if nb else 0.0 for w in wb]
    f = [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(precision, recall)]
    ab, ba = distance_stats(d_ab), distance_stats(d_ba)
    return dict(thresholds=th, precision=precision, recall=recall, f=f, a_samples=na, b_samples=nb, a_to_b=ab, b_to_a=ba,
                chamfer=0.5 * (ab["mean"] + ba["mean"]), hausdorff=max(ab["max"], ba["max"]))


def format_f_score(r):
    """the app's printed form: the two sample counts, then tau, precision, recall and f per threshold, then the fields of format_result;
    every float at %.9g"""
    parts = [f"a_samples={r['a_samples']}", f"b_samples={r['b_samples']}"]
    for t, p, q, f in zip(r["thresholds"], r["precision"], r["recall"], r["f"]):
        parts.append(f"tau={t:.9g} precision={p:.9g} recall={q:.9g} f={f:.9g}")
    return " ".join(parts) + " " + format_result(r)
