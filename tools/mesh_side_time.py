"""Call times of the mesh-side and ICP entry points on the workloads of profiles/mesh_distance.md, mesh_render.md, mesh_voxelise.md,
mesh_align.md and icp_256_kernel_stats.md, one JSON line per run: `python tools/mesh_side_time.py [name ...]`.  Device events around each
call, the median of CALLS calls after one warm-up call.  SOBFU_HIP_LIB picks the library, so two builds can be timed side by side, each
run in a process of its own (profiles/mesh_side_home.md).

The mesh: marching_cubes_indexed of init_sphere (r = 0.2 m at (0.375, 0.37, 0.38)) in a 256^3 volume of 0.75 m -- 175 632 triangles,
87 818 vertices.
  distance_brute   its own vertices moved 2 mm along their normals, mode brute (brute_force_kernel<false>)
  distance_grid    the same points, mode grid with closest points (grid_query_kernel, then brute_force_kernel<true> on an empty list)
  raycast_brute    the 160 x 120 rays of a camera 0.6 m in front of the sphere, mode brute (ray_brute_kernel)
  voxelise         back into the 256^3 volume, trunc 48 voxels, eta 3 voxels, cell 4 voxels (row_parity_kernel, brick_kernel)
  inside           the voxel centres of every fourth voxel per axis, 64^3 points (mesh_inside_kernel)
  voxelise_winding the open mesh of profiles/mesh_winding.md -- the same mesh without the faces whose centroid lies within 4 mm of the
                   planes x = centre and y = centre + 0.1 m -- into the 256^3 volume with sign="winding" (row_winding_kernel,
                   winding_sum_kernel over the seam list, brick_kernel); the JSON line carries its triangle and boundary-edge counts
  winding          the 64^3 points of `inside` against the open mesh, mode "boundary" (mesh_winding_kernel, winding_sum_kernel)
  align            10 iterations, dof 6, from the vertices turned by 1 degree and moved 2 mm (align_*_kernel and the grid query)
  sample_sphere / sample_box   about 1 M area-weighted samples (profiles/mesh_sample.md) of the mesh and of a 1 x 0.5 x 0.25 m box of 12
                   triangles: ops.mesh_sample at a given density -- count, scan, the read-back, generate (sample_count_kernel, the scan,
                   sample_generate_kernel); sample_sphere_generate / sample_box_generate: the generate call alone through a counted workspace
  sample_score     ops.distance_score of the sphere samples' distances against four thresholds (distance_score_kernel)
  sample_query     TriangleGrid.query of the sphere's samples against the mesh moved by 2 mm: what f_score spends per direction
  icp_points / icp_depth   {10, 5, 4} iterations on 640 x 480 frames rendered from the mesh at two poses (icp_*_kernel)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sobfu_amd import ops  # noqa: E402

CALLS = {"distance_brute": 5, "distance_grid": 30, "raycast_brute": 5, "voxelise": 3, "inside": 5, "voxelise_winding": 3, "winding": 5, "align": 20, "icp_points": 20, "icp_depth": 20,
         "sample_sphere": 20, "sample_box": 20, "sample_sphere_generate": 30, "sample_box_generate": 30, "sample_score": 30, "sample_query": 10}
N, SIZE = 256, 0.75
VS = SIZE / N
INTR = (525.0, 525.0, 319.5, 239.5)


def timed(name, fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS[name]):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main(names):
    vol = ops.new_volume((N, N, N))
    ops.init_sphere(vol, (VS,) * 3, 48 * VS, 3 * VS, (0.375, 0.37, 0.38), 0.2)
    v, nrm, f = ops.marching_cubes_indexed(vol, (SIZE,) * 3)
    del vol
    moved = v.clone()
    moved[:, :3] += 0.002 * nrm[:, :3]
    grid = ops.TriangleGrid(v, f)
    centre = v[:, :3].mean(0)
    out = dict(lib=os.environ.get("SOBFU_HIP_LIB", "in-tree"), triangles=int(f.shape[0]), vertices=int(v.shape[0]))
    if "distance_brute" in names:
        out["distance_brute"] = timed("distance_brute", lambda: grid.query(moved, mode="brute"))
    if "distance_grid" in names:
        out["distance_grid"] = timed("distance_grid", lambda: grid.query(moved, closest=True, mode="grid"))
    if "raycast_brute" in names:
        u, w = torch.meshgrid(torch.arange(160.0, device="cuda"), torch.arange(120.0, device="cuda"), indexing="xy")
        d = torch.stack([(u - 79.5) / 131.0, (w - 59.5) / 131.0, torch.ones_like(u), torch.zeros_like(u)], -1).reshape(-1, 4).contiguous()
        o = torch.cat([centre - torch.tensor([0.0, 0.0, 0.6], device="cuda"), torch.ones(1, device="cuda")]).repeat(d.shape[0], 1).contiguous()
        out["raycast_brute"] = timed("raycast_brute", lambda: grid.raycast(o, d, mode="brute"))
    if {"voxelise", "inside", "voxelise_winding", "winding"} & set(names):
        vv = v.clone()  # the mesh in the volume's frame: marching cubes writes (x, -y, -z)
        vv[:, 1:3] *= -1.0
        vgrid = ops.TriangleGrid(vv, f, cell=4 * VS)
        if "voxelise" in names:
            dst = ops.new_volume((N, N, N))
            out["voxelise"] = timed("voxelise", lambda: vgrid.voxelise((N, N, N), (VS,) * 3, 48 * VS, 3 * VS, out=dst))
            del dst
        if "inside" in names or "winding" in names:
            g = (torch.arange(0, N, 4, dtype=torch.float32, device="cuda") + 0.5) * VS
            zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
            pts = torch.stack([xx, yy, zz, torch.ones_like(xx)], -1).reshape(-1, 4).contiguous()
        if "inside" in names:
            out["inside"] = timed("inside", lambda: vgrid.inside(pts))
        if "voxelise_winding" in names or "winding" in names:
            mid = vv[f.long(), :3].mean(1)
            keep = ((mid[:, 0] - 0.375).abs() > 0.004) & ((mid[:, 1] - 0.47).abs() > 0.004)
            ogrid = ops.TriangleGrid(vv, f[keep].contiguous(), cell=4 * VS)
            out.update(open_triangles=ogrid.n_triangles, boundary_edges=int(ogrid.boundary.shape[0]))
            if "voxelise_winding" in names:
                dst = ops.new_volume((N, N, N))
                out["voxelise_winding"] = timed("voxelise_winding", lambda: ogrid.voxelise((N, N, N), (VS,) * 3, 48 * VS, 3 * VS, out=dst, sign="winding"))
                del dst
            if "winding" in names:
                out["winding"] = timed("winding", lambda: ogrid.winding(pts, mode="boundary"))
    if "align" in names:
        a = np.deg2rad(1.0)
        R = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device="cuda")
        src = v.clone()
        src[:, :3] = (v[:, :3] - centre) @ R.T + centre + torch.tensor([0.002, 0.0, 0.0], device="cuda")
        out["align"] = timed("align", lambda: grid.align(src, iters=10, dof=6))
    if any(n.startswith("sample") for n in names):
        import math

        bv = torch.tensor([(x, y, z, 1.0) for z in (0.0, 0.25) for y in (0.0, 0.5) for x in (0.0, 1.0)], dtype=torch.float32, device="cuda")
        bf = torch.tensor([(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)],
                          dtype=torch.int32, device="cuda")
        for name, (mv, mf) in (("sample_sphere", (v, f)), ("sample_box", (bv, bf))):
            area = math.fsum(ops.mesh_sample_count(mv, mf, 0.0, areas=True)[3].cpu().numpy().tolist())
            density = 1.0e6 / area
            rc, total, ws, _ = ops.mesh_sample_count(mv, mf, density)
            assert rc == 0
            out[name + "_samples"] = total
            if name in names:
                out[name] = timed(name, lambda: ops.mesh_sample(mv, mf, density=density))
            if name + "_generate" in names:
                out[name + "_generate"] = timed(name + "_generate", lambda: ops.mesh_sample_generate(mv, mf, 0, ws, total))
        if "sample_score" in names or "sample_query" in names:
            pts = grid.sample(density=1.0e6 / math.fsum(ops.mesh_sample_count(v, f, 0.0, areas=True)[3].cpu().numpy().tolist()))
            mgrid = ops.TriangleGrid(moved, f)
            dist = mgrid.query(pts)[0]
            if "sample_score" in names:
                out["sample_score"] = timed("sample_score", lambda: ops.distance_score(dist, (0.001, 0.002, 0.005, 0.01)))
            if "sample_query" in names:
                out["sample_query"] = timed("sample_query", lambda: mgrid.query(pts))
    if "icp_points" in names or "icp_depth" in names:
        t0 = (-centre + torch.tensor([0.0, 0.0, 0.6], device="cuda")).cpu().numpy()
        frames = [grid.render(INTR, 480, 640, pose=(np.eye(3), t0 + dt), outputs=("depth",))["depth"] for dt in ((0, 0, 0), (0.003, -0.002, 0.001))]

        def li(level):
            return tuple(float(np.float32(np.float32(x) / np.float32(1 << level))) for x in INTR)

        def pyramids(d, depth_mode):
            dd = [d]
            for _ in range(2):
                dd.append(ops.depth_pyramid(dd[-1], 0.04))
            if depth_mode:
                return dd, [ops.normals_mask_depth(x, li(i)) for i, x in enumerate(dd)]
            pn = [ops.point_normals(x, li(i)) for i, x in enumerate(dd)]
            return [p for p, _ in pn], [n for _, n in pn]

        for name, depth_mode in (("icp_points", False), ("icp_depth", True)):
            if name in names:
                c, nc = pyramids(frames[1].clone(), depth_mode)
                p, np_ = pyramids(frames[0].clone(), depth_mode)
                icp = ops.ICP(0.1, np.deg2rad(20), (10, 5, 4, 0))
                out[name] = timed(name, lambda: icp.enqueue(INTR, c, nc, p, np_))
                out[name + "_status"] = int(icp.status.item())
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:] or list(CALLS))
