"""bench.py's --steps and --dump-outputs on the host: the timed regions add up to exactly --steps iterations, and the dump is
float32, within 64 MB and the same sample of cells from run to run."""
import os

import numpy as np
import torch

import bench


def test_regions_add_up_to_the_steps():
    for K in (1, 2, 6, 7, 24, 50, 101):
        for R in (1, 2, 3, 5, 7, 200):
            sizes = bench.region_steps(K, R)
            assert sum(sizes) == K and len(sizes) == min(K, R) and max(sizes) - min(sizes) <= 1 and min(sizes) >= 1


def test_median_step_is_per_step():
    assert bench.median_step_s([1.0, 3.0, 2.0], [1, 3, 1]) == 1.0
    assert bench.median_step_s([4.0, 6.0], [2, 2]) == 2.5


def _dump(tmp_path, dim, tag):
    dims = (dim, dim, dim)
    g = torch.Generator().manual_seed(1)
    psi = torch.rand((dim, dim, dim, 4), generator=g)
    pnp = torch.rand((dim, dim, dim, 2), generator=g)
    d = tmp_path / tag
    bench.dump_outputs(str(d), dims, psi, pnp, np.arange(5, dtype=np.float32))
    return {f[:-4]: np.load(d / f) for f in os.listdir(d)}, psi, pnp


def test_dump_small_grid_is_whole(tmp_path):
    out, psi, pnp = _dump(tmp_path, 16, "a")
    assert set(out) == {"psi", "phi_n_psi", "max_update_norms"}
    assert np.array_equal(out["psi"], psi.numpy()) and np.array_equal(out["phi_n_psi"], pnp.numpy())
    assert all(a.dtype == np.float32 for a in out.values())


def test_dump_large_grid_is_a_fixed_sample_within_64_mb(tmp_path):
    out, psi, pnp = _dump(tmp_path, 104, "a")  # 104^3 > bench.DUMP_MAX_VOXELS
    again, _, _ = _dump(tmp_path, 104, "b")
    assert set(out) == {"psi", "phi_n_psi", "max_update_norms", "sample_voxels"}
    idx = out["sample_voxels"]
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_MAX_VOXELS and np.array_equal(idx, again["sample_voxels"])
    i = idx.astype(np.int64)
    assert np.array_equal(out["psi"], psi.numpy().reshape(-1, 4)[i]) and np.array_equal(out["phi_n_psi"], pnp.numpy().reshape(-1, 2)[i])
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
