"""The oracle's reductions -- the two energies and the max update norm with its arg-max, the numbers a solve reports and stops on --
against plain numpy restatements, on sentinel inputs placed at the block, wave and grid-stride trip boundaries of the reference's
launch shape (tests/reporting_cases.py), from 1 cell to 2**26 + 1.  The GPU tests compare the HIP reductions with the oracle bit
for bit; this pins the oracle itself, independently of its C code."""
import numpy as np
import pytest

import reporting_cases as RC


def test_reduce_config_restatement(oracle):
    for n in RC.SIZES + [4, 5, 7, 1000, 2 ** 26 - 1, 2 ** 26 + 1024, 2 ** 30]:
        assert oracle.reduce_config(n) == RC.reduce_config(n), n
    assert RC.reduce_config(2 ** 26) == (65536, 512) and RC.reduce_config(2 ** 26 + 1) == (65536, 512)  # a second trip from here


@pytest.mark.parametrize("n", RC.SIZES)
def test_energies_on_sentinels_are_exact(oracle, n):
    sent = RC.sum_sentinels(n)
    want = RC.exact_energy(sent)
    g, f = RC.data_inputs(n, sent)
    assert oracle.data_energy(g, f) == want
    del g, f
    J = RC.jacobian_inputs(n, sent)
    assert oracle.reg_energy_sobolev(J) == want
    # one sentinel less / one more: the sum must move (a dropped or doubled cell cannot hide)
    c0 = next(iter(sent))
    J[c0] = 0
    assert oracle.reg_energy_sobolev(J) == want - 0.5 * float(np.float64(sent[c0]) ** 2)


@pytest.mark.parametrize("n", [1, 3, 64, 513, 1025, 70000, 2 ** 21 + 3])
def test_energies_on_random_inputs_within_the_summation_bound(oracle, n):
    rng = np.random.default_rng(n)
    g = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 9, n)], -1).astype(np.float32)
    f = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 9, n)], -1).astype(np.float32)
    d = g[:, 0] - f[:, 0]
    t = (d * d).astype(np.float64)  # the fp32 terms, summed exactly
    got = oracle.data_energy(g, f)
    assert abs(got - 0.5 * t.sum()) <= 0.5 * RC.sum_bound(t) + abs(got) * 2.0 ** -24
    J = rng.uniform(-2, 2, (n, 4, 4)).astype(np.float32)
    r = J[:, :3, :3]
    t = ((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]).astype(np.float32)
    t = ((t[:, 0] + t[:, 1]) + t[:, 2]).astype(np.float32).astype(np.float64)
    got = oracle.reg_energy_sobolev(J)
    assert abs(got - 0.5 * t.sum()) <= 0.5 * RC.sum_bound(t) + abs(got) * 2.0 ** -24


def test_norm_restatement_rounds_down():
    u = np.array([[1, 1, 0, 0], [1, 1, 1, 0], [3, 4, 12, 0], [0, 0, 0, 0], [-0.0, -0.0, -0.0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0],
                  [3e19, 0, 0, 0], [1e-30, 0, 0, 0]], np.float32)
    r = RC.norm_rd(u)
    assert r[0] == np.float32(np.sqrt(2)) and r[1] == np.float32(np.sqrt(3))  # fp32(sqrt) of both already lies below
    assert r[2] == 13 and r[3] == 0 and r[4] == 0 and np.isnan(r[5]) and r[6] == np.inf and r[7] == np.inf and r[8] == 0
    s = np.random.default_rng(0).uniform(0, 4, 20000).astype(np.float32)
    r = RC.norm_rd(np.stack([np.sqrt(s.astype(np.float64)), 0 * s, 0 * s], -1).astype(np.float32))
    x = np.stack([np.sqrt(s.astype(np.float64)), 0 * s], -1).astype(np.float32)[:, 0]
    s = x * x  # the fp32 sum the norm rounds
    up = np.nextafter(r, np.float32(np.inf))
    assert np.all(r.astype(np.float64) ** 2 <= s) and np.all(up.astype(np.float64) ** 2 > s)  # the largest float whose square is <= s
    assert np.any(r != np.sqrt(s))  # ... which is not always the rounded-to-nearest root


@pytest.mark.parametrize("n", RC.SIZES)
def test_max_update_norm_on_sentinels(oracle, n):
    u = np.zeros((n, 4), np.float32)
    for name, cells in RC.max_cases(n):
        for i, v in cells.items():
            u[i] = v
        want = RC.expected_max(cells, n)
        got = oracle.max_update_norm(u)
        assert np.array_equal(np.float32(got), np.float32(want)), (name, got, want)
        for i in cells:
            u[i] = 0
    if n <= RC.BIG:  # every cell NaN: nothing beats the 0 the maxima start from
        assert oracle.max_update_norm(np.full((n, 4), np.nan, np.float32)) == (0.0, 0.0)


def test_max_cases_really_test_the_scan_order():
    """the tie cases must put the winner where the lowest index would not (else they could not tell the orders apart), and the
    tree's bit-reversed thread order must differ from the plain one on them"""
    n = 2 ** 26 + 1
    b, t = RC.reduce_config(n)
    cases = dict(RC.max_cases(n))
    for name in ("tie across lanes", "tie across waves, even", "tie across trips"):
        _, idx = RC.expected_max(cases[name], n)
        tied = [i for i, v in cases[name].items() if RC.norm_rd(np.asarray(v, np.float32)) == 13]
        assert idx != float(min(tied)), name
    assert RC.scan_key(69, n)[1] < RC.scan_key(t + 3, n)[1] and RC.scan_key(64, n)[1] < RC.scan_key(3, n)[1]
    # above 2**24 the float-encoded index rounds (reductor.cu:371)
    assert RC.index_value(2 ** 24 + 1, n) == 2 ** 24 and RC.index_value(2 ** 26 + 1, n) == 2 ** 26
