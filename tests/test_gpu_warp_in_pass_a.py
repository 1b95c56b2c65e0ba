"""The compact single-GPU loop of grids beyond the Infinity Cache runs without the phi_n o psi stream: pass A samples phi_n at psi
itself and pass B stores no F (solver_kernels.hip, loop_warps_in_pass_a).  Its solves must be bit for bit those of the F-stream
loop (SOBFU_WARP_A=0) and of the API format.  Small grids take the same launch path with SOBFU_CACHE_CELLS=0, which makes every
grid count as beyond the cache: odd extents then reach the clamp and mirror edges of both passes."""
import numpy as np
import pytest

from fixture_inputs import sphere_volume, warped_identity

pytestmark = pytest.mark.gpu

ALPHA, W_REG = 0.001, 0.6


@pytest.fixture(scope="module")
def ops():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sobfu_amd import ops as o

    return o


def _inputs(dims, seed):
    X, Y, Z = dims
    c = (0.5 * X, 0.5 * Y, 0.5 * Z)
    r = 0.3 * min(dims)
    pg = sphere_volume(dims, c, r, 4.0)
    pn = sphere_volume(dims, (c[0] + 1.3, c[1] - 0.7, c[2] + 0.4), r, 4.0)
    psi = warped_identity(dims, seed, 1.5)  # displacements past the faces: the samplers clamp
    return pg, pn, psi


def _solve(ops, dims, ins, *, mode="iterate", compact=True, max_iter=6, thr=-1.0, split=(2, 3, 1)):
    import torch

    pg, pn, psi = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins)
    pnp = ops.new_volume(dims)
    sv = ops.Solver(dims, max_iter=max_iter, alpha=ALPHA, w_reg=W_REG, max_update_norm=thr)
    sv.set_compact(compact)
    if mode == "split":  # begin / step / end
        sv.begin(pg, pn, pnp, psi, max_iter)
        for n in split:
            sv.step(n)
        rep, hist = sv.end()
    else:
        rep, hist = sv.iterate(pg, pn, pnp, psi, max_iter)
    torch.cuda.synchronize()
    out = (psi.cpu().numpy(), pnp.cpu().numpy(), hist, rep.iterations, rep.converged)
    sv.close()
    return out


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert a[3:] == b[3:]


def _check(ops, monkeypatch, dims, seed, **kw):
    ins = _inputs(dims, seed)
    warp = _solve(ops, dims, ins, **kw)
    monkeypatch.setenv("SOBFU_WARP_A", "0")
    fstream = _solve(ops, dims, ins, **kw)
    monkeypatch.delenv("SOBFU_WARP_A")
    api = _solve(ops, dims, ins, compact=False, **kw)
    _same(warp, fstream)
    _same(warp, api)
    return warp


def test_256_cubed(ops, monkeypatch):
    out = _check(ops, monkeypatch, (256, 256, 256), 11, max_iter=4)
    assert out[3] == 4 and np.isfinite(out[2]).all()


def test_odd_grid_beyond_cache(ops, monkeypatch):
    monkeypatch.setenv("SOBFU_CACHE_CELLS", "0")
    _check(ops, monkeypatch, (67, 45, 37), 12, max_iter=6)
    _check(ops, monkeypatch, (130, 9, 29), 13, max_iter=5)


def test_threshold_fires_mid_run(ops, monkeypatch):
    monkeypatch.setenv("SOBFU_CACHE_CELLS", "0")
    dims = (67, 45, 37)
    free = _solve(ops, dims, _inputs(dims, 14), max_iter=8)
    thr = float(free[2][3])  # the norm of iteration 4: the solver stops there at the latest
    stop = 1 + int(np.flatnonzero(free[2] <= np.float32(thr))[0])
    out = _check(ops, monkeypatch, dims, 14, max_iter=8, thr=thr)
    assert out[3] == stop <= 4 and out[4] == 1


def test_begin_step_end(ops, monkeypatch):
    monkeypatch.setenv("SOBFU_CACHE_CELLS", "0")
    dims = (67, 45, 37)
    out = _check(ops, monkeypatch, dims, 15, mode="split", max_iter=6, split=(2, 3, 1))
    whole = _solve(ops, dims, _inputs(dims, 15), max_iter=6)
    _same(out, whole)
