"""The solver's REPORTING outputs at their edges, against the oracle: the reduction launchers on sentinel inputs at the block / wave /
trip boundaries of the reference's launch shape (tests/reporting_cases.py, pinned to numpy in test_reporting_reference.py), the
convergence break on a threshold exactly equal to a norm, solves whose state turns NaN / inf, and the `updates` buffer, the log and
the report fields at every verbosity.

Arrays are compared bitwise; where NaN may appear the NaN masks must be equal and everything else bitwise (NaN sign and payload
legitimately differ: x86 produces a negative default NaN, the GPU a positive one)."""
import functools

import numpy as np
import pytest

import reporting_cases as RC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device; the product path has no CPU fallback")
    from sobfu_amd import ops as _ops

    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """bitwise, except that NaN matches NaN of any sign / payload"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def f32(x):
    return np.float32(x)


def free_hbm():
    return torch.cuda.mem_get_info()[0]


# ---------------------------------------------------------------------------------------------------
# the reduction launchers on the sentinels of tests/reporting_cases.py
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.SIZES + [512 ** 3])
def test_reduction_launchers_on_sentinels(ops, oracle, n):
    if n * 16 * 3 > free_hbm():
        pytest.skip("not enough free HBM")
    sent = RC.sum_sentinels(n)
    idx = torch.tensor(list(sent), dtype=torch.int64, device="cuda")
    g, f = RC.data_inputs(n, sent)
    want = oracle.data_energy(g, f)
    assert want == RC.exact_energy(sent)
    g_d, f_d = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 2), device="cuda")
    g_d[idx], f_d[idx] = dev(g[list(sent)]), dev(f[list(sent)])
    assert f32(ops.data_energy(g_d, f_d)) == f32(want)
    del g, f, g_d, f_d
    if n <= 2 ** 26 + 1:  # the Jacobian launcher at 512^3 would need 8 GiB for nothing new
        J = RC.jacobian_inputs(n, sent)
        want = oracle.reg_energy_sobolev(J)
        J_d = torch.zeros((n, 4, 4), device="cuda")
        J_d[idx] = dev(J[list(sent)])
        assert f32(ops.reg_energy_sobolev(J_d)) == f32(want) == f32(RC.exact_energy(sent))
        del J, J_d
    u = np.zeros((n, 4), np.float32)
    u_d = torch.zeros((n, 4), device="cuda")
    for name, cells in RC.max_cases(n):
        at = list(cells)
        vals = np.array([cells[i] for i in at], np.float32).reshape(-1, 4)
        u[at] = vals
        want = oracle.max_update_norm(u)
        assert np.array_equal(np.float32(want), np.float32(RC.expected_max(cells, n))), name
        if at:
            u_d[torch.tensor(at, dtype=torch.int64, device="cuda")] = dev(vals)
        got = ops.max_update_norm(u_d)
        assert np.array_equal(np.float32(got).view(np.uint32), np.float32(want).view(np.uint32)), (name, got, want)
        u[at] = 0
        u_d.zero_()
    if n <= RC.BIG:
        u_d.fill_(float("nan"))
        assert ops.max_update_norm(u_d) == (0.0, 0.0)


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 3, 7), (16, 8, 8), (33, 17, 9), (64, 64, 65)])
def test_reg_energy_from_psi_on_sentinels(ops, oracle, dims):
    X, Y, Z = dims
    n = X * Y * Z
    psi = oracle.new_field(dims)
    oracle.init_identity(psi)
    flat = psi.reshape(-1, 4)
    for k, c in enumerate(RC.sentinel_cells(n)):
        flat[c, k % 3] += np.float32(2.0 ** (k % 6))
    flat[:, 3] = 1e30  # w: not part of the displacement
    J = np.zeros((Z, Y, X, 4, 4), np.float32)
    oracle.jacobian(psi, J, 1)
    want = oracle.reg_energy_sobolev(J)
    assert want > 0 or min(dims) == 2  # two cells along an axis: the one-sided differences of both cells vanish (vector_fields.cu)
    assert f32(ops.reg_energy_sobolev_from_psi(dev(psi))) == f32(want)


def test_thin_box_max_norm_ignores_nan(ops, oracle):
    """A thin (lane-per-cell) pass-B box over OWNED cells must leave a NaN update out of the max norm, as the marching paths and the
    reference's reduce_max (strict '>' from 0) do: as an unsigned bit pattern NaN would beat every finite norm in the slots."""
    import tiled_reference
    from sobfu_amd import tiled

    dims = (40, 24, 20)
    X, Y, Z = dims
    rng = np.random.default_rng(3)
    pg = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.integers(0, 3, (Z, Y, X))], -1).astype(np.float32)
    pn = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.integers(0, 3, (Z, Y, X))], -1).astype(np.float32)
    psi0 = oracle.new_field(dims)
    oracle.init_identity(psi0)
    psi0[..., :3] += rng.uniform(-0.5, 0.5, psi0[..., :3].shape).astype(np.float32)
    S = oracle.sobolev_filter(7, 0.1)
    L = tiled.TileLayout(dims, (1, 1, 1), 0)
    ob = L.own_box()
    maxima = []
    for compact in (False, True):
        for thin in (False, True):
            be = tiled_reference.HipBackend(compact=compact)
            psi_l, pnp_l = dev(psi0), torch.zeros(L.local_shape(2), device="cuda")
            st = be.begin(L, dev(pg), dev(pn), pnp_l, psi_l)
            be.pass_a(st, ob, 0.4, None, 0.0)
            nU = host(st.nabla_U)[..., :3].copy()
            st.nabla_U[11, 9, 7, 1] = float("nan")  # one NaN: NaN updates on the seven-cell cross around it
            slots = torch.zeros(256, dtype=torch.int32, device="cuda")
            be.pass_b(st, ob, slots, S, 0.1, None, 0.0, thin=thin)
            torch.cuda.synchronize()
            maxima.append(tiled._sqrt_rd(int(host(slots).view(np.uint32).max())))
    # the oracle on the same nabla_U: smoothing + update, then Reductor::max_update_norm
    nU4 = np.zeros((Z, Y, X, 4), np.float32)
    nU4[..., :3] = nU
    nU4[11, 9, 7, 1] = np.nan
    nUS, upd, psi = oracle.new_field(dims), oracle.new_field(dims), psi0.copy()
    oracle.convolution_rows(nUS, nU4, S)
    oracle.convolution_columns(nUS, nU4, S)
    oracle.convolution_depth(nUS, nU4, S)
    oracle.update_psi(psi, nUS, upd, 0.1)
    assert np.isnan(upd).any(-1).sum() >= 7
    want = oracle.max_update_norm(upd)[0]
    assert np.isfinite(want) and want > 0
    assert all(m == want for m in maxima), (maxima, want)


# ---------------------------------------------------------------------------------------------------
# solves: thresholds exactly on a norm, updates / log / report at every verbosity
# ---------------------------------------------------------------------------------------------------
def _run1_inputs(oracle):
    dims = (64, 64, 64)
    size = np.float32(0.25)
    vs = np.array([size / np.float32(64)] * 3, np.float32)
    trunc, eta = np.float32(10) * vs[0], np.float32(2) * vs[0]
    pg, pn = oracle.new_volume(dims), oracle.new_volume(dims)
    oracle.init_sphere(pg, vs, trunc, eta, (0.13, 0.13, 0.13), 0.012)
    oracle.init_sphere(pn, vs, trunc, eta, (0.125, 0.13, 0.13), 0.012)
    return dims, pg, pn


MAX_ITER, ALPHA, W_REG = 120, 0.01, 0.4
BREAKS = {"none": None, "iteration 1": 1, "reporting iteration": 50, "quiet run": 62}


@functools.lru_cache(maxsize=None)
def _contract_case(brk):
    import oracle

    dims, pg, pn = _run1_inputs(oracle)
    ident = oracle.new_field(dims)
    oracle.init_identity(ident)
    full = oracle.estimate_psi(pg, pn, ident.copy(), max_iter=MAX_ITER, alpha=ALPHA, w_reg=W_REG, verbosity=2, inverse_iters=0)["trace"]
    assert np.all(np.diff(full[:, 2]) < 0)
    k = BREAKS[brk]
    thr = -1.0 if k is None else float(full[k - 1, 2])  # exactly the norm of iteration k: the rule is `<=`
    psi = ident.copy()
    r = oracle.estimate_psi(pg, pn, psi, max_iter=MAX_ITER, alpha=ALPHA, w_reg=W_REG, verbosity=2, max_update_norm=thr)
    assert r["iters"] == (k or MAX_ITER)
    r["psi"] = psi
    return dims, pg, pn, ident, thr, r


def _reports(verbosity, it):
    return verbosity == 2 or (verbosity == 1 and (it == 1 or it % 50 == 0 or it == MAX_ITER))


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "api"])
@pytest.mark.parametrize("brk", list(BREAKS))
@pytest.mark.parametrize("verbosity", [-1, "0+keep", 1, 2, 3])
def test_updates_log_and_report_at_every_verbosity(ops, oracle, verbosity, brk, compact):
    from test_reference_fixtures import expected_log

    dims, pg, pn, ident, thr, r = _contract_case(brk)
    keep = verbosity == "0+keep"
    v = 0 if keep else verbosity
    sv = ops.Solver(dims, max_iter=MAX_ITER, alpha=ALPHA, w_reg=W_REG, verbosity=v, max_update_norm=thr)
    sv.set_compact(compact)
    if keep:
        sv.keep_updates()
    psi_d, psi_inv_d, pnp_d, pgi_d = dev(ident), ops.new_field(dims), ops.new_volume(dims), ops.new_volume(dims)
    rep, hist = sv.estimate_psi(dev(pg), pgi_d, dev(pn), pnp_d, psi_d, psi_inv_d)
    it = r["iters"]
    assert rep.iterations == it and rep.converged == (1 if thr >= 0 else 0)
    assert same(hist, r["trace"][:, 2])
    assert same(host(psi_d), r["psi"]) and same(host(pnp_d), r["phi_n_psi"])
    assert same(host(psi_inv_d), r["psi_inv"]) and same(host(pgi_d), r["phi_global_psi_inv"])
    if v > 0 or keep:
        assert same(host(sv.updates()), r["updates"]), "updates of the last executed iteration"
    assert "\n".join(sv.log_lines) + "\n" == expected_log(r["trace"], dims, MAX_ITER, W_REG, thr, v)
    rep_its = [k for k in range(1, it + 1) if _reports(v, k)]
    if rep_its:
        k = rep_its[-1] - 1
        assert rep.last_e_data == r["trace"][k, 0] and rep.last_e_reg == r["trace"][k, 1]
    else:
        assert np.isnan(rep.last_e_data) and np.isnan(rep.last_e_reg)
    if _reports(v, it):
        assert rep.last_max_update_index == r["trace"][it - 1, 3]
    else:
        assert np.isnan(rep.last_max_update_index)
    sv.close()


@pytest.mark.parametrize("brk", ["iteration 1", "quiet run"])
@pytest.mark.parametrize("keep", [False, True])
def test_session_and_iterate_break_exactly_on_the_threshold(ops, oracle, brk, keep):
    """begin / step / end with the break inside a step, and iterate(): the same stopping iteration and arrays, and with
    keep_updates the last executed iteration's updates"""
    dims, pg, pn, ident, thr, r = _contract_case(brk)
    psi_want = r["psi"]
    sv = ops.Solver(dims, max_iter=MAX_ITER, alpha=ALPHA, w_reg=W_REG, max_update_norm=thr)
    if keep:
        sv.keep_updates()
    psi_d, pnp_d = dev(ident), ops.new_volume(dims)
    sv.begin(dev(pg), dev(pn), pnp_d, psi_d, MAX_ITER)
    for n in (40, 40, 40):  # the break (1 or 62) falls inside a step
        sv.step(n)
    rep, hist = sv.end()
    assert rep.iterations == r["iters"] and rep.converged == 1 and same(hist, r["trace"][:, 2])
    assert same(host(psi_d), psi_want) and same(host(pnp_d), r["phi_n_psi"])
    if keep:
        assert same(host(sv.updates()), r["updates"])
    assert sv.log_lines[-1] == f"SOLVER CONVERGED AFTER {r['iters']} ITERATIONS"
    psi_d, pnp_d = dev(ident), ops.new_volume(dims)
    rep, hist = sv.iterate(dev(pg), dev(pn), pnp_d, psi_d, MAX_ITER)
    assert rep.iterations == r["iters"] and rep.converged == 1 and same(hist, r["trace"][:, 2])
    assert same(host(psi_d), psi_want) and same(host(pnp_d), r["phi_n_psi"])
    if keep:
        assert same(host(sv.updates()), r["updates"])
    sv.close()


# ---------------------------------------------------------------------------------------------------
# non-finite states on every path of the loop
# ---------------------------------------------------------------------------------------------------
NF_DIMS = (40, 24, 36)  # 2 x 2 x 2 tiles of 20 x 12 x 18
NF_ITERS = 6


def _nf_inputs(case):
    import oracle

    if case == "diverging":  # psi overflows to inf, then NaN spreads through the grid until every norm is NaN
        dims = (24, 24, 24)
        size = np.float32(0.25)
        vs = np.array([size / np.float32(24)] * 3, np.float32)
        trunc, eta = np.float32(5) * vs[0], np.float32(2) * vs[0]
        pg, pn = oracle.new_volume(dims), oracle.new_volume(dims)
        oracle.init_sphere(pg, vs, trunc, eta, (0.13, 0.13, 0.13), 0.06)
        oracle.init_sphere(pn, vs, trunc, eta, (0.12, 0.13, 0.13), 0.06)
        psi0 = oracle.new_field(dims)
        oracle.init_identity(psi0)
        return dims, pg, pn, psi0, dict(alpha=1.0, w_reg=1.0), 40
    dims = NF_DIMS
    X, Y, Z = dims
    rng = np.random.default_rng(11)
    pg = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.integers(0, 3, (Z, Y, X))], -1).astype(np.float32)
    pn = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.integers(0, 3, (Z, Y, X))], -1).astype(np.float32)
    psi0 = oracle.new_field(dims)
    oracle.init_identity(psi0)
    psi0[..., :3] += rng.uniform(-0.7, 0.7, psi0[..., :3].shape).astype(np.float32)
    if case == "NaN in phi_n, interior":
        pn[25, 7, 13, 0] = np.nan
    elif case == "NaN in phi_n, corner":
        pn[0, 0, 0, 0] = np.nan
    elif case == "NaN in phi_n, tile shell":  # next to the x, y and z cuts of 2 x 2 x 2 tiles
        pn[18, 12, 20, 0] = np.nan
    elif case == "NaN in psi.y":
        psi0[17, 11, 19, 1] = np.nan
    return dims, pg, pn, psi0, dict(alpha=0.05, w_reg=0.4), NF_ITERS


@functools.lru_cache(maxsize=None)
def _nf_case(case):
    """inputs, a threshold that fires on a partially non-finite iteration (taken from the oracle's trace), the oracle's result"""
    import oracle

    dims, pg, pn, psi0, kw, iters = _nf_inputs(case)
    dead = oracle.estimate_psi(pg, pn, psi0.copy(), max_iter=iters, **kw, verbosity=2, inverse_iters=0)["trace"][:, 2]
    thr = 0.0 if case == "diverging" else float(np.nanmin(dead[:iters - 1]))
    psi = psi0.copy()
    r = oracle.estimate_psi(pg, pn, psi, max_iter=iters, **kw, verbosity=2, max_update_norm=thr)
    k = r["iters"]
    assert k < iters and r["trace"][k - 1, 2] <= thr  # the break fires ...
    part = oracle.estimate_psi(pg, pn, psi0.copy(), max_iter=k - 1 if case == "diverging" else k, **kw, inverse_iters=0)["updates"]
    nan_cells = np.isnan(part[..., :3]).any(-1)
    assert 0 < nan_cells.sum() < nan_cells.size  # ... on (diverging: right after) an iteration whose updates are partly NaN
    if case == "diverging":
        assert np.isnan(r["updates"][..., :3]).all() and r["trace"][k - 1, 2] == 0 and np.isinf(dead).any()
    r["psi"] = psi
    return dims, pg, pn, psi0, kw, iters, thr, r


NF_CASES = ["NaN in phi_n, interior", "NaN in phi_n, corner", "NaN in phi_n, tile shell", "NaN in psi.y", "diverging"]


@pytest.mark.parametrize("path", ["compact", "api", "verbosity 1", "verbosity 2", "session", "native 1 rank"])
@pytest.mark.parametrize("case", NF_CASES)
def test_non_finite_solves(ops, oracle, case, path):
    from sobfu_amd import tiled

    dims, pg, pn, psi0, kw, iters, thr, r = _nf_case(case)
    k = r["iters"]
    if path == "native 1 rank":
        nt = tiled.NativeTiledSolver(dims, max_update_norm=thr, **kw)
        psi_d, pnp_d = dev(psi0), ops.new_volume(dims)
        done, hist = nt.iterate(dev(pg), dev(pn), pnp_d, psi_d, iters)
        nt.close()
        assert done == k and same(hist, r["trace"][:, 2])
        assert same(host(psi_d), r["psi"]) and same(host(pnp_d), r["phi_n_psi"])
        return
    v = {"verbosity 1": 1, "verbosity 2": 2}.get(path, 0)
    sv = ops.Solver(dims, max_iter=iters, max_update_norm=thr, verbosity=v, **kw)
    sv.set_compact(path != "api")
    sv.keep_updates()
    psi_d, pnp_d = dev(psi0), ops.new_volume(dims)
    if path == "session":
        sv.begin(dev(pg), dev(pn), pnp_d, psi_d, iters)
        sv.step(k - 1)
        sv.step(iters - k + 1)
        rep, hist = sv.end()
    else:
        psi_inv_d, pgi_d = ops.new_field(dims), ops.new_volume(dims)
        rep, hist = sv.estimate_psi(dev(pg), pgi_d, dev(pn), pnp_d, psi_d, psi_inv_d)
        assert same(host(psi_inv_d), r["psi_inv"]) and same(host(pgi_d), r["phi_global_psi_inv"])
    assert rep.iterations == k and rep.converged == 1 and same(hist, r["trace"][:, 2])
    assert same(host(psi_d), r["psi"]) and same(host(pnp_d), r["phi_n_psi"])
    assert same(host(sv.updates()), r["updates"])
    sv.close()


@pytest.mark.parametrize("grid", [(2, 2, 2), (1, 2, 2)])
@pytest.mark.parametrize("case", NF_CASES + ["finite, threshold on a norm"])
def test_non_finite_solves_on_tiles(ops, oracle, case, grid):
    """the native tiled loop on the direct transport (every rank in this process): the oracle's stopping iteration, history and
    arrays, and the single-GPU handle's"""
    from test_gpu_tiled_loopback import run_world_direct

    if case == "finite, threshold on a norm":
        dims, pg, pn, psi0, kw, iters = _nf_inputs(case)
        dead = oracle.estimate_psi(pg, pn, psi0.copy(), max_iter=iters, **kw, verbosity=2, inverse_iters=0)["trace"][:, 2]
        thr = float(dead[iters // 2])
        psi = psi0.copy()
        r = oracle.estimate_psi(pg, pn, psi, max_iter=iters, **kw, max_update_norm=thr)
        r["psi"] = psi
    else:
        dims, pg, pn, psi0, kw, iters, thr, r = _nf_case(case)
    k = r["iters"]
    sv = ops.Solver(dims, max_iter=iters, max_update_norm=thr, **kw)
    psi_s, pnp_s = dev(psi0), ops.new_volume(dims)
    rep, hist_s = sv.iterate(dev(pg), dev(pn), pnp_s, psi_s, iters)
    sv.close()
    assert rep.iterations == k and same(hist_s, r["trace"][:, 2])
    out, (psi_t, pnp_t) = run_world_direct(dims, grid, psi0, pg, pn, iters, thr, True, 1, kw)
    for done, hist, _, _ in out:
        assert done == k and same(hist, r["trace"][:, 2]) and same(hist, hist_s)
    assert same(psi_t[..., :3], r["psi"][..., :3]) and same(psi_t[..., :3], host(psi_s)[..., :3])
    assert same(pnp_t, r["phi_n_psi"]) and same(pnp_t, host(pnp_s))
