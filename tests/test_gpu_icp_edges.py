"""Camera tracking on the MI355X at the shapes tests/test_gpu_icp.py never reaches (tests/icp_cases.py: one workgroup, a handful, odd
extents, widths off the 64 x 4 tile) and with a row pitch on every operand: the image kernels bit for bit, one correspondence pass with
its codes, count and sums always checked against the derived bound, single solves against the fp64 restatement on the GPU's own sums,
the trace's launch order, and every documented way an estimate fails.  tests/test_icp_cases_cpu.py shows on the CPU that the cases are
meaningful and that the sums check rejects a lost pixel and a cols-for-step mix-up.

Measured on an MI355X (recorded so that a reader sees the slack; nothing is tuned to these):
  correspondence passes   sums error at most 0.162 of the bound (m + 10) 2^-24 sabs (24x40 level 1; 0.014 .. 0.126 at level 0);
                          validity patches 0.038; no case needed its cap: the codes were identical everywhere
  solves                  every pose of every launch 0 ulp from the restatement (1 allowed); every trace row exact"""
import numpy as np
import pytest
import torch

import icp_cases as K
import icp_reference as IR

pytestmark = pytest.mark.gpu
D_SENTINEL, F_SENTINEL = 0x7B7B, 7.0
EYE = np.eye(4, dtype=np.float32)


# ---- device images, dense or pitched ---------------------------------------------------------------------------------------------------
class Images:
    """Makes device images, dense or -- pitched -- as [:, :cols] views of sentinel-filled tensors with 3 more columns (uint16) or one
    more pixel (float4, which keeps the 16-byte alignment), and remembers the pitched ones so that their padding can be checked."""

    def __init__(self, pitched):
        self.pitched, self.bases = pitched, []

    def _new(self, shape, dtype):
        if not self.pitched:
            return torch.empty(shape, dtype=dtype, device="cuda")
        rows, cols = shape[:2]
        pad, fill = {torch.int16: (3, D_SENTINEL), torch.float32: (1, F_SENTINEL), torch.uint8: (3, 0x7B)}[dtype]
        base = torch.full((rows, cols + pad) + tuple(shape[2:]), fill, dtype=dtype, device="cuda")
        self.bases.append((base, cols, fill))
        return base[:, :cols]

    def depth(self, rows, cols):
        return self._new((rows, cols), torch.int16)

    def float4(self, rows, cols):
        return self._new((rows, cols, 4), torch.float32)

    def codes(self, rows, cols):
        return self._new((rows, cols), torch.uint8)

    def put(self, a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        out = self._new(tuple(a.shape), t.dtype)
        out.copy_(t)
        return out

    def check_padding(self):
        torch.cuda.synchronize()
        for base, cols, fill in self.bases:
            assert bool((base[:, cols:] == fill).all()), (tuple(base.shape), cols)
        return len(self.bases)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _f32(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    """NaN at the same places, everything else bit-equal"""
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.dtype.kind != "f":
        assert np.array_equal(got, want)
        return
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(got)
    assert np.array_equal(_bits(got)[m], _bits(want)[m])


# ---- 1. image kernels -------------------------------------------------------------------------------------------------------------------
def _image_chain(d, intr, pitched):
    """every image kernel on depth `d`, through out= tensors -> ({name: numpy}, the Images that made the operands)"""
    from sobfu_amd import ops

    im = Images(pitched)
    rows, cols = d.shape
    out = {}
    src = im.put(d)
    pyr = ops.depth_pyramid(src, K.SIGMA, out=im.depth(rows // 2, cols // 2))
    out["pyr1"] = _u16(pyr)
    if rows // 2 >= 2 and cols // 2 >= 2:
        out["pyr2"] = _u16(ops.depth_pyramid(pyr, K.SIGMA, out=im.depth(rows // 4, cols // 4)))
    p, n = ops.point_normals(src, intr, points=im.float4(rows, cols), normals=im.float4(rows, cols))
    out["points"], out["normals"] = _f32(p), _f32(n)
    dm = im.put(d)
    nm = ops.normals_mask_depth(dm, intr, normals=im.float4(rows, cols))
    out["masked_depth"], out["masked_normals"] = _u16(dm), _f32(nm)
    if rows >= 2 and cols >= 2:
        d2, n2 = ops.resize_depth_normals(dm, nm, depth_out=im.depth(rows // 2, cols // 2), normals_out=im.float4(rows // 2, cols // 2))
        out["rdn_depth"], out["rdn_normals"] = _u16(d2), _f32(n2)
        p2, n2 = ops.resize_points_normals(p, n, points_out=im.float4(rows // 2, cols // 2), normals_out=im.float4(rows // 2, cols // 2))
        out["rpn_points"], out["rpn_normals"] = _f32(p2), _f32(n2)
    assert np.array_equal(_u16(src), d)  # the source is read only
    return out, im


def _image_reference(d, intr):
    rows, cols = d.shape
    ref = {"pyr1": IR.depth_pyramid(d, K.SIGMA)}
    if rows // 2 >= 2 and cols // 2 >= 2:
        ref["pyr2"] = IR.depth_pyramid(ref["pyr1"], K.SIGMA)
    ref["points"], ref["normals"] = IR.point_normals(d, intr)
    ref["masked_depth"], ref["masked_normals"] = IR.normals_mask_depth(d, intr)
    ref["rdn_depth"], ref["rdn_normals"] = IR.resize_depth_normals(ref["masked_depth"], ref["masked_normals"])
    ref["rpn_points"], ref["rpn_normals"] = IR.resize_points_normals(ref["points"], ref["normals"])
    return ref


def _check_images(d, intr):
    ref = _image_reference(d, intr)
    dense, _ = _image_chain(d, intr, False)
    assert set(dense) == set(ref)
    for k in ref:
        _same(dense[k], ref[k])
    pitched, im = _image_chain(d, intr, True)
    assert im.check_padding() >= 10
    for k in ref:
        _same(pitched[k], ref[k])
        assert np.array_equal(_bits(pitched[k]), _bits(dense[k])), k  # bit for bit, NaN payloads included


@pytest.mark.parametrize("name", list(K.CASES))
def test_image_kernels_at_small_odd_and_pitched_shapes(name):
    _, _, intr = K.CASES[name]
    _check_images(K.frames(name)[1], intr)


def test_image_kernels_at_the_depth_edges():
    # 0, 1, 46341 (d * d > INT_MAX), 65535 and values 119 / 120 / 121 mm apart side by side: the restatement computes in int64
    _check_images(K.edge_depth(), (64.0, 64.0, 12.5, 10.5))


@pytest.mark.parametrize("pitched", [False, True])
def test_image_kernels_at_their_minimal_extents(pitched):
    from sobfu_amd import ops

    intr = (64.0, 64.0, 0.5, 0.5)
    im = Images(pitched)
    d = np.array([[900, 1000], [0, 905]], np.uint16)
    assert _u16(ops.depth_pyramid(im.put(d), K.SIGMA, out=im.depth(1, 1)))[0, 0] == 900  # the clipped window is the centre alone
    full = np.array([[46341, 65535], [1, 3]], np.uint16)
    nrm = np.arange(16, dtype=np.float32).reshape(2, 2, 4)
    for src in (d, full):
        d2, n2 = ops.resize_depth_normals(im.put(src), im.put(nrm), depth_out=im.depth(1, 1), normals_out=im.float4(1, 1))
        rd2, rn2 = IR.resize_depth_normals(src, nrm)
        _same(_u16(d2), rd2)
        _same(_f32(n2), rn2)
    assert rd2[0, 0] == (46341 + 65535 + 1 + 3) // 4
    pts = nrm + 1
    p2, n2 = ops.resize_points_normals(im.put(pts), im.put(nrm + 2), points_out=im.float4(1, 1), normals_out=im.float4(1, 1))
    rp2, rn2 = IR.resize_points_normals(pts, nrm + 2)
    assert not np.isnan(rp2).any()
    _same(_f32(p2), rp2)
    _same(_f32(n2), rn2)
    one = np.array([[1000]], np.uint16)
    p, n = ops.point_normals(im.put(one), intr, points=im.float4(1, 1), normals=im.float4(1, 1))
    assert np.isnan(_f32(p)).all() and np.isnan(_f32(n)).all()
    dm = im.put(one)
    nm = _f32(ops.normals_mask_depth(dm, intr, normals=im.float4(1, 1)))
    assert np.isnan(nm[0, 0, :3]).all() and nm[0, 0, 3] == 0 and _u16(dm)[0, 0] == 0
    if pitched:
        assert im.check_padding() >= 10


# ---- 2. one correspondence pass -----------------------------------------------------------------------------------------------------------
def _step(level, intr, inputs, aff, pitched=False):
    """ops.icp_step on numpy inputs (curr, ncurr, prev, nprev) -> (codes, the 29 sums, the Images)"""
    from sobfu_amd import ops

    im = Images(pitched)
    dev = [im.put(a) for a in inputs]
    rows, cols = inputs[1].shape[:2]
    A, b, count, rms, codes = ops.icp_step(level, intr, *dev, aff, K.DIST, K.ANGLE, codes=im.codes(rows, cols))
    return codes, K.pack(A, b, count, rms), im, (A, b, count, rms)


PASSES = [(n, m, 0) for n in K.CASES for m in K.MODES] + [(n, m, 1) for n in ("24x40", "33x67") for m in K.MODES]


@pytest.mark.parametrize("name,mode,level", PASSES)
def test_one_pass_codes_count_and_sums(name, mode, level):
    intr = K.CASES[name][2]
    inputs = K.level_inputs(name, mode, level)
    ref = K.reference_pass(name, mode, level)
    rows, cols = ref[0].shape
    codes, got, _, _ = _step(level, intr, inputs, K.NEAR)
    cap = 0 if name in ("24x40", "33x67") else K.cap_of(ref[2])
    differ, frac = K.check_pass(codes, got, ref, rows, cols, cap=cap)
    print(f"\n{name} {mode} level {level}: parts {K.parts_of(rows, cols)} m {K.pixels_per_lane(rows, cols)} inliers {int(got[27])} "
          f"differing pixels {differ} (cap {cap}) largest sums error / bound {frac:.3f}")
    # every operand pitched: bitwise the same codes and sums, the padding untouched
    pcodes, pgot, im, _ = _step(level, intr, inputs, K.NEAR, pitched=True)
    assert im.check_padding() == 5
    assert np.array_equal(pcodes, codes) and np.array_equal(_bits(pgot), _bits(got))


def test_one_pass_validity_conventions():
    rows, cols, intr = K.CASES["120x160"]
    c, nc, p, np_, cm, pm = K.validity_inputs()
    ref = K.validity_reference()
    codes, got, _, _ = _step(0, intr, (c, nc, p, np_), K.NEAR)
    assert (codes[cm] == 40).all()  # misses, +Inf, a zero normal and a NaN normal in the current frame
    assert (codes == 120).sum() > (K.reference_pass("120x160", "points", 0)[0] == 120).sum() + pm.sum() // 2
    differ, frac = K.check_pass(codes, got, ref, rows, cols)  # ... and 120 wherever the reference sees an invalid target
    assert np.isfinite(got).all()
    print(f"\nvalidity: differing pixels {differ} (cap {K.cap_of(ref[2])}) largest sums error / bound {frac:.3f}")


# ---- 3. the solve ---------------------------------------------------------------------------------------------------------------------------
def _device_levels(inputs_per_level):
    """[(curr, ncurr, prev, nprev) per level] numpy -> four lists of device tensors, finest first"""
    im = Images(False)
    cols = list(zip(*[[im.put(a) for a in lv] for lv in inputs_per_level]))
    return [list(c) for c in cols]


def _estimate(intr, lists, iters, trace_rows=None, icp=None):
    """-> (ok, pose, trace (rows, 2), the ICP object); the trace is prefilled with -7 so that unwritten rows show"""
    from sobfu_amd import ops

    icp = ops.ICP(K.DIST, K.ANGLE, iters) if icp is None else icp
    icp.trace = torch.full((2 * max(sum(iters) + 2, trace_rows or 0),), -7.0, dtype=torch.float32, device="cuda")
    ok, pose = icp.estimate(intr, *lists)
    return ok, pose.copy(), icp.trace.cpu().numpy().reshape(-1, 2), icp


def _solve_chain(name, mode, iters):
    """The poses after every launch of an estimate with budgets `iters`, by truncated budgets; each launch's sums again through
    icp_step at its input pose (the same kernel on the same grid: the doubles the solve saw); the restatement's solve of them.
    -> the largest difference in float32 ulps"""
    intr = K.CASES[name][2]
    n = len(iters)
    per_level = [K.level_inputs(name, mode, l, "small") for l in range(n)]
    lists = _device_levels(per_level)
    order = K.launch_levels(iters)
    poses, traces = [EYE], []
    for k in range(1, len(order) + 1):  # the budgets of the first k launches
        budget = [0] * n
        for l in order[:k]:
            budget[l] += 1
        ok, pose, trace, _ = _estimate(intr, lists, tuple(budget))
        assert ok
        assert (trace[k:] == -7.0).all() and (trace[:k] != -7.0).all()  # exactly k written rows
        poses.append(pose)
        traces.append(trace)
    for k, t in enumerate(traces, 1):  # a shorter budget is a prefix of the longer one
        assert np.array_equal(_bits(t[:k]), _bits(trace[:k]))
    worst = 0
    for k, level in enumerate(order):
        _, _, _, (A, b, count, rms) = _step(level, intr, per_level[level], poses[k])
        with np.errstate(all="ignore"):
            ok, x = IR.solve(A, b)
        assert ok
        want = IR.compose(x, poses[k])
        got = poses[k + 1]
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], np.float32)) and np.isfinite(got).all()
        u = K.ulps(got[:3], want[:3])
        worst = max(worst, int(u.max()))
        assert u.max() <= 1, (k, level, u)
        assert _bits(trace[k, 0]) == _bits(np.float32(count)) and _bits(trace[k, 1]) == _bits(np.float32(rms)), (k, trace[k], count, rms)
    return worst, poses, trace, lists


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", ["24x40", "120x160"])
def test_each_solve_matches_the_fp64_restatement(name, mode):
    worst, poses, _, _ = _solve_chain(name, mode, (2, 2))
    assert not np.array_equal(poses[-1], EYE)
    print(f"\n{name} {mode}: largest pose difference {worst} ulp")


def test_trace_order_skips_a_level_without_iterations():
    # (3, 0, 2, 0): level 2 twice, then level 0 three times; the inlier counts and poses of every launch pin the order
    worst, poses, trace, lists = _solve_chain("120x160", "points", (3, 0, 2))
    print(f"\n(3, 0, 2): largest pose difference {worst} ulp; inliers {trace[:5, 0]}")
    intr = K.CASES["120x160"][2]
    ok, pose, trace4, icp = _estimate(intr, lists, (3, 0, 2, 0), trace_rows=9)
    assert ok and np.array_equal(_bits(pose), _bits(poses[-1]))
    assert np.array_equal(_bits(trace4[:5]), _bits(trace[:5])) and (trace4[5:] == -7.0).all() and len(trace4) == 9
    # bitwise reproducible: the same object again, and a fresh one
    ok2, pose2, trace2, _ = _estimate(intr, lists, (3, 0, 2, 0), trace_rows=9, icp=icp)
    ok3, pose3, trace3, _ = _estimate(intr, lists, (3, 0, 2, 0), trace_rows=9)
    for o, p, t in ((ok2, pose2, trace2), (ok3, pose3, trace3)):
        assert o and np.array_equal(_bits(p), _bits(pose)) and np.array_equal(_bits(t), _bits(trace4))


# ---- 4. failures ------------------------------------------------------------------------------------------------------------------------------
def _plane_lists(mode, levels=3, shape=K.PLANE_SHAPE, intr=K.PLANE_INTR):
    per_level = []
    for l, d in enumerate(K.plane_levels(levels, shape)):
        a, n = K.maps_of(d, intr, l, mode)
        per_level.append((a, n, a, n))
    return per_level


@pytest.mark.parametrize("mode", K.MODES)
def test_rank_deficient_plane_fails_at_the_first_solve(mode):
    per_level = _plane_lists(mode)
    lists = _device_levels(per_level)
    ok, pose, trace, icp = _estimate(K.PLANE_INTR, lists, (3, 2, 2, 0))
    assert not ok and icp.failure() == (2, 0)
    assert np.array_equal(_bits(pose), _bits(EYE))  # the pose of the iteration before: the identity
    _, _, _, (A, b, count, rms) = _step(2, K.PLANE_INTR, per_level[2], EYE)
    assert count == 11 * 15 and A[2, 2] == 0 and rms == 0
    assert trace[0, 0] == count and _bits(trace[0, 1]) == _bits(np.float32(0.0))
    assert (trace[1:] == -7.0).all()  # every later launch exited at once
    _, _, _, (A0, _, count0, _) = _step(0, K.PLANE_INTR, per_level[0], EYE)
    assert count0 == 2961 and A0[2, 2] == 0  # thousands of inliers, and no rotation about z


def test_failure_at_a_later_level_keeps_the_pose_of_the_iteration_before():
    name = "120x160"
    rows, cols, intr = K.CASES[name]
    per_level = [K.level_inputs(name, "points", l, "small") for l in range(3)]
    per_level[0] = _plane_lists("points", 1, (rows, cols), intr)[0]  # the finest level sees the plane
    lists = _device_levels(per_level)
    ok, pose, trace, icp = _estimate(intr, lists, (3, 2, 2, 0))
    assert not ok and icp.failure() == (0, 0)
    ok_before, before, trace_before, _ = _estimate(intr, lists, (0, 2, 2, 0))
    assert ok_before and not np.array_equal(before, EYE)
    assert np.array_equal(_bits(pose), _bits(before))
    assert (trace[:5] != -7.0).all() and (trace[5:] == -7.0).all() and len(trace) >= 7  # four solves and the failed one
    assert np.array_equal(_bits(trace[:4]), _bits(trace_before[:4]))
    _, _, _, (A, _, count, rms) = _step(0, intr, per_level[0], before)
    assert A[2, 2] == 0 and trace[4, 0] == count and _bits(trace[4, 1]) == _bits(np.float32(rms))


def test_fewer_than_six_inliers_fail_and_the_object_recovers():
    name = "24x40"
    intr = K.CASES[name][2]
    good = K.level_inputs(name, "points", 0, "small")
    p, n = K.sparse_frame()
    sparse = _device_levels([(p, n, good[2], good[3])])
    ok, pose, trace, icp = _estimate(intr, sparse, (3, 0, 0, 0))
    assert not ok and icp.failure() == (0, 0)
    assert np.isfinite(pose).all() and np.array_equal(_bits(pose), _bits(EYE))
    assert 0 < trace[0, 0] < 6 and (trace[1:] == -7.0).all()
    # reuse: the object that just failed estimates the good pair, bitwise like a fresh object
    lists = _device_levels([good])
    ok1, pose1, trace1, _ = _estimate(intr, lists, (3, 0, 0, 0), icp=icp)
    ok2, pose2, trace2, _ = _estimate(intr, lists, (3, 0, 0, 0))
    assert ok1 and ok2 and icp.failure() is None
    assert np.array_equal(_bits(pose1), _bits(pose2)) and np.array_equal(_bits(trace1), _bits(trace2))
    assert not np.array_equal(pose1, EYE) and (trace1[:3] != -7.0).all()
