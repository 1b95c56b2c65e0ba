"""The warping march of pass A at the edges of its own tile shape (64 x kWarpWY = 16 cells, sobfu_geometry.hpp).  With SOBFU_CACHE_CELLS=0 every grid counts as beyond the Infinity Cache and takes the
warping loop; its solves must be bit for bit those of the F-stream loop (SOBFU_WARP_A=0) and of the API format: psi, phi_n o psi, the
norm history and the iteration count.

Grids: (67, 45, 37) odd everywhere, a partial third tile row; (130, 9, 29) Y below the tile height; (64, 17, 5) one row into a second
tile and a short z; (65, 16, 3) one lane into a second tile column and a march shorter than the pipeline (psi is requested two planes
ahead); (70, 33, 40) more than one z-chunk per tile.  psi is the identity displaced by up to 1.5 cells, which carries samples past
every face (the clamp), or the identity itself: every face cell then sits exactly on 0 and on top = dim - 1, where the upper-index
rule collapses the corner pair."""
import numpy as np
import pytest

from fixture_inputs import identity, sphere_volume, warped_identity

pytestmark = pytest.mark.gpu

ALPHA, W_REG = 0.001, 0.6
GRIDS = [((67, 45, 37), 6), ((130, 9, 29), 5), ((64, 17, 5), 5), ((65, 16, 3), 4), ((70, 33, 40), 4)]


@pytest.fixture(scope="module")
def ops():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sobfu_amd import ops as o

    return o


def _inputs(dims, seed):
    c = tuple(0.5 * e for e in dims)
    r = 0.3 * min(dims)
    pg = sphere_volume(dims, c, r, 4.0)
    pn = sphere_volume(dims, (c[0] + 1.3, c[1] - 0.7, c[2] + 0.4), r, 4.0)
    psi = identity(dims) if seed is None else warped_identity(dims, seed, 1.5)
    return pg, pn, psi


def _solve(ops, dims, ins, compact, max_iter):
    import torch

    pg, pn, psi = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ins)
    pnp = ops.new_volume(dims)
    sv = ops.Solver(dims, max_iter=max_iter, alpha=ALPHA, w_reg=W_REG, max_update_norm=-1.0)
    sv.set_compact(compact)
    rep, hist = sv.iterate(pg, pn, pnp, psi, max_iter)
    torch.cuda.synchronize()
    out = (psi.cpu().numpy(), pnp.cpu().numpy(), hist, rep.iterations, rep.converged)
    sv.close()
    return out


def _check(ops, monkeypatch, dims, seed, max_iter):
    monkeypatch.setenv("SOBFU_CACHE_CELLS", "0")
    ins = _inputs(dims, seed)
    warp = _solve(ops, dims, ins, True, max_iter)
    monkeypatch.setenv("SOBFU_WARP_A", "0")
    fstream = _solve(ops, dims, ins, True, max_iter)
    monkeypatch.delenv("SOBFU_WARP_A")
    api = _solve(ops, dims, ins, False, max_iter)
    for other in (fstream, api):
        for x, y in zip(warp[:3], other[:3]):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        assert warp[3:] == other[3:]
    assert warp[3] == max_iter and np.isfinite(warp[2]).all()
    assert not np.array_equal(warp[0], ins[2])  # the solve moved psi


@pytest.mark.parametrize("dims,max_iter", GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_displaced_past_the_faces(ops, monkeypatch, dims, max_iter):
    _check(ops, monkeypatch, dims, 21 + sum(dims), max_iter)


@pytest.mark.parametrize("dims", [(67, 45, 37), (65, 16, 3)], ids=lambda v: "x".join(map(str, v)))
def test_identity_psi_on_the_faces(ops, monkeypatch, dims):
    _check(ops, monkeypatch, dims, None, 4)
