"""The cases of tests/test_gpu_icp_edges.py, checked on the CPU with the numpy restatement alone (tests/icp_cases.py, tests/icp_reference.py):
every case has inliers, every code, a solvable system and few marginal pixels; the estimates' reference chains solve; the failure frames
fail for the reason the GPU tests name; and the sums check rejects a lost inlier and a cols-for-step mix-up."""
import numpy as np
import pytest

import icp_cases as K
import icp_reference as IR

INT_MAX = 2 ** 31 - 1


def _solve(s):
    with np.errstate(all="ignore"):
        return IR.solve(*IR.unpack(s))


@pytest.mark.parametrize("name,parts,m", [("24x40", 1, 4), ("33x67", 3, 3), ("120x160", 19, 4), ("131x259", 34, 4)])
def test_launch_shapes(name, parts, m):
    rows, cols, _ = K.CASES[name]
    assert K.parts_of(rows, cols) == parts and K.pixels_per_lane(rows, cols) == m
    assert K.parts_of(480, 640) == 256 and K.pixels_per_lane(480, 640) == 5  # the capped launch of tests/test_gpu_icp.py


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", list(K.CASES))
def test_cases_are_meaningful(name, mode):
    rows, cols, _ = K.CASES[name]
    codes, row, margin, every = K.reference_pass(name, mode, 0)
    s, _ = IR.sums(row, codes)
    assert s[27] >= 0.25 * rows * cols, s[27]
    assert set(np.unique(codes)) == {0, 40, 80, 120, 160, 200}
    ok, _ = _solve(s)
    assert ok and np.linalg.cond(IR.unpack(s)[0]) <= 1e7
    assert K.cap_of(margin) <= 1e-3 * rows * cols, K.cap_of(margin)
    assert np.array_equal(every[codes == 0], row[codes == 0]) and np.isfinite(every[codes == 0]).all()
    other = K.reference_pass(name, "depth" if mode == "points" else "points", 0)[0]
    assert abs(int((other == 0).sum()) - int(s[27])) <= 1  # points and depth mode see the same frame


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("name", ["24x40", "33x67"])
def test_small_cases_have_no_marginal_pixel(name, mode, level):
    codes, row, margin, _ = K.reference_pass(name, mode, level)
    assert K.cap_of(margin) == 0  # the GPU's codes must be identical
    s, _ = IR.sums(row, codes)
    assert s[27] >= 100 and _solve(s)[0]
    rows, cols = codes.shape
    assert K.parts_of(rows, cols) == (1 if level else K.parts_of(*K.CASES[name][:2]))


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", ["24x40", "120x160"])
def test_two_level_chain_solves(name, mode):
    chain = K.reference_chain(name, mode, (2, 2))
    assert [c[0] for c in chain] == [1, 1, 0, 0]
    for level, inliers, cond, ok, _ in chain:
        assert ok and cond <= 2.5e5 and inliers >= 100, (level, inliers, cond)


@pytest.mark.parametrize("iters,levels", [((3, 0, 2), [2, 2, 0, 0, 0]), ((0, 2, 2), [2, 2, 1, 1])])
def test_three_level_chains_solve(iters, levels):
    chain = K.reference_chain("120x160", "points", iters)
    assert [c[0] for c in chain] == levels and all(c[3] and c[2] <= 2.5e5 for c in chain)


@pytest.mark.parametrize("mode", K.MODES)
def test_the_plane_is_rank_deficient_with_thousands_of_inliers(mode):
    for level, d in enumerate(K.plane_levels(3)):
        a, n = K.maps_of(d, K.PLANE_INTR, level, mode)
        assert np.array_equal(n[:-1, :-1, :3], np.broadcast_to(np.array([0, 0, -1], np.float32), n[:-1, :-1, :3].shape))
        codes, row, _ = IR.correspond(level, K.PLANE_INTR, a, n, a, n, np.eye(4), K.DIST, K.ANGLE)
        s, _ = IR.sums(row, codes)
        A, b = IR.unpack(s)
        assert s[27] == (d.shape[0] - 1) * (d.shape[1] - 1) and A[2, 2] == 0 and s[28] == 0
        assert not _solve(s)[0]
    assert K.plane_levels(1)[0].shape == (48, 64) and (47 * 63) == 2961


def test_the_sparse_frame_has_fewer_than_six_inliers():
    p, n = K.sparse_frame()
    assert IR.valid(p, n).sum() == 4
    _, _, pp, pn = K.level_inputs("24x40", "points", 0, "small")
    codes, row, _ = IR.correspond(0, K.CASES["24x40"][2], p, n, pp, pn, np.eye(4), K.DIST, K.ANGLE)
    s, _ = IR.sums(row, codes)
    assert 0 < s[27] < 6 and not _solve(s)[0]


def test_validity_patches_take_their_codes():
    c, nc, p, np_, cm, pm = K.validity_inputs()
    codes, row, margin, every = K.validity_reference()
    base = K.reference_pass("120x160", "points", 0)[0]
    assert cm.sum() == pm.sum() == 4 * K.PATCH ** 2 and not (cm & pm).any()
    assert (base[cm] == 0).sum() > cm.sum() // 2  # the patches lie on the surface: they spoil inliers
    assert (codes[cm] == 40).all()
    assert not IR.valid(p, np_)[pm].any()
    assert (codes == 120).sum() >= (base == 120).sum() + pm.sum() // 2  # pixels that land in a spoilt patch of the previous frame
    changed = (codes != base) & ~cm
    assert (codes[changed] == 120).all() and np.isin(base[changed], (0, 160, 200)).all()  # only through their targets
    s, sabs = K.sums_over(every, codes == 0)
    assert np.isfinite(s).all() and _solve(s)[0]


def test_edge_depth_sees_every_edge():
    d = K.edge_depth().astype(np.int64)
    for v in (0, 1, 46341, 65535):
        assert (d == v).any()
    assert 46341 ** 2 > INT_MAX >= 46340 ** 2
    q = lambda oy, ox: d[oy::2, ox::2]
    prod = q(0, 0) * q(0, 1)
    nz = (q(0, 0) != 0) & (q(0, 1) != 0) & (q(1, 0) != 0) & (q(1, 1) != 0)
    assert ((prod > INT_MAX) & nz).any() and ((prod > INT_MAX) & ~nz).any() and (~nz & (prod != 0)).any()
    diffs = set()
    for y in range(d.shape[0] // 2):
        for x in range(d.shape[1] // 2):
            win = d[max(0, 2 * y - 2):min(2 * y + 3, d.shape[0] - 1), max(0, 2 * x - 2):min(2 * x + 3, d.shape[1] - 1)]
            diffs |= set(np.abs(win - d[2 * y, 2 * x]).ravel().tolist())
    assert {119, 120, 121} <= diffs
    dd, _ = IR.resize_depth_normals(K.edge_depth(), np.ones(d.shape + (4,), np.float32))
    assert dd[0, 0] == 46341 and dd[1, 0] == 65535 and dd[2, 0] == 0 and dd[3, 0] == 1


# ---- the sums check bites -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", list(K.CASES))
def test_the_sums_check_accepts_the_reference_and_rejects_a_lost_inlier(name, mode):
    rows, cols, _ = K.CASES[name]
    ref = K.reference_pass(name, mode, 0)
    codes, row = ref[0], ref[1]
    s, sabs = IR.sums(row, codes)
    assert K.check_pass(codes, s, ref, rows, cols, cap=0) == (0, 0.0)
    lost = codes.copy()
    y, x = np.argwhere(codes == 0)[-1]  # the last inlier: a tail pixel
    lost[y, x] = 160
    s1, _ = IR.sums(row, lost)
    with pytest.raises(AssertionError):
        K.check_pass(codes, s1, ref, rows, cols)
    s1[27] = s[27]  # even with the count restored, the other sums give the loss away
    with pytest.raises(AssertionError):
        K.check_pass(codes, s1, ref, rows, cols)


@pytest.mark.parametrize("name", ["24x40", "131x259"])
def test_the_sums_check_rejects_cols_in_place_of_step(name):
    rows, cols, intr = K.CASES[name]
    ref = K.reference_pass(name, "points", 0)
    c, nc, p, np_ = K.level_inputs(name, "points", 0)
    pitched = np.full((rows, cols + 1, 4), 7.0, np.float32)  # the previous normals with one pixel of padding per row
    pitched[:, :cols] = np_
    wrong = pitched.reshape(-1, 4)[:rows * cols].reshape(rows, cols, 4)  # row y read at y * cols, not y * step
    codes, row, _ = IR.correspond(0, intr, c, nc, p, wrong, K.NEAR, K.DIST, K.ANGLE)
    s, _ = IR.sums(row, codes)
    with pytest.raises(AssertionError):
        K.check_pass(codes, s, ref, rows, cols)
    with pytest.raises(AssertionError):  # and with the right codes, the sums alone
        K.check_pass(ref[0], s, ref, rows, cols)
