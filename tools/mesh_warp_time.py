"""Timing probe of the canonical mesh carried to live: the 256^3 sphere of tests/test_marching_cubes.py::test_hip_256_cubed_mesh_is_closed,
its indexed mesh, the vertices and normals pushed through a smooth psi (up to 2 voxels) and phi sampled at them.  Under
`rocprofv3 --kernel-trace --stats` this gives the kernel times of profiles/mesh_warp_256_kernel_stats.md; on its own, host-side times
(synchronised perf_counter around REPS enqueued calls)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sobfu_amd import ops  # noqa: E402

REPS = int(os.environ.get("MESH_WARP_REPS", "20"))
n, vs = 256, 0.75 / 256
vol = ops.new_volume((n, n, n))
ops.init_sphere(vol, (vs,) * 3, 48 * vs, 3 * vs, (0.375, 0.37, 0.38), 0.2)
g = torch.arange(n, dtype=torch.float32, device="cuda")
zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
psi = torch.stack([xx + 2.0 * torch.sin(yy * 0.05), yy + 1.5 * torch.cos(zz * 0.04), zz + 1.0 * torch.sin(xx * 0.03), torch.zeros_like(xx)], -1).contiguous()
del xx, yy, zz
R, t = np.eye(3), (0, 0, 0)
ws = ops.mc_indexed_workspace(vol)


def timed(what, fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        out = fn()
    torch.cuda.synchronize()
    print("%s: %.1f us per call (%d calls)" % (what, 1e6 * (time.perf_counter() - t0) / REPS, REPS))
    return out


v, nr, f = timed("marching_cubes_indexed 256^3", lambda: ops.marching_cubes_indexed(vol, (0.75,) * 3, workspace=ws))
print("%d vertices, %d faces" % (v.shape[0], f.shape[0]))
wv, wn = torch.empty_like(v), torch.empty_like(nr)
timed("warp_points with normals", lambda: ops.warp_points(psi, (vs,) * 3, R, t, v, nr, mc_vertices=True, out=(wv, wn)))
timed("warp_points without normals", lambda: ops.warp_points(psi, (vs,) * 3, R, t, v, mc_vertices=True, out=wv))
d = torch.empty(v.shape[0], dtype=torch.float32, device="cuda")
timed("sample_tsdf", lambda: ops.sample_tsdf(vol, (vs,) * 3, R, t, wv, mc_vertices=True, out=d))
moved = (wv - v)[:, :3].norm(dim=1)
print("displacement: mean %.3f max %.3f voxel; valid samples %d of %d" % (float(moved.mean()) / vs, float(moved.max()) / vs, int((~torch.isnan(d)).sum()), d.numel()))
