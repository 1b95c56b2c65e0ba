"""Camera tracking on the MI355X: the image kernels and one ICP pass against the numpy restatement tests/icp_reference.py, the whole
on-device estimate on analytic frames (points and depth), bitwise reproducibility, failure on an empty frame, and graph capture."""
import numpy as np
import pytest
import torch

import icp_cases as K
import icp_reference as IR

pytestmark = pytest.mark.gpu
INTR = (570.342, 570.342, 320.0, 240.0)
TRUTH = IR.pose(IR.rot((0.3, 1.0, 0.2), 2.0), (0.012, -0.012, 0.0106))  # 2 degrees, 2 cm


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda()
    return torch.from_numpy(a).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def frames():
    return IR.render_depth(np.eye(4), INTR), IR.render_depth(TRUTH, INTR)


def _same_nan(a, b, ulps=0):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    if ulps == 0:
        assert np.array_equal(a[m], b[m])
    else:
        assert (np.abs(a[m].view(np.int32).astype(np.int64) - b[m].view(np.int32).astype(np.int64)) <= ulps).all()


def test_image_kernels_match_the_restatement(frames):
    from sobfu_amd import ops

    d = frames[1]
    pyr = ops.depth_pyramid(_dev(d), 0.04)
    assert np.array_equal(_u16(pyr), IR.depth_pyramid(d, 0.04))
    pyr2 = ops.depth_pyramid(pyr, 0.04)
    assert np.array_equal(_u16(pyr2), IR.depth_pyramid(IR.depth_pyramid(d, 0.04), 0.04))
    p, n = ops.point_normals(_dev(d), INTR)
    rp, rn = IR.point_normals(d, INTR)
    _same_nan(p.cpu().numpy(), rp)
    _same_nan(n.cpu().numpy(), rn)
    dm = _dev(d)
    nm = ops.normals_mask_depth(dm, INTR)
    rdm, rnm = IR.normals_mask_depth(d, INTR)
    assert np.array_equal(_u16(dm), rdm)
    _same_nan(nm.cpu().numpy(), rnm)
    d2, n2 = ops.resize_depth_normals(dm, nm)
    rd2, rn2 = IR.resize_depth_normals(rdm, rnm)
    assert np.array_equal(_u16(d2), rd2)
    _same_nan(n2.cpu().numpy(), rn2)
    p2, n2 = ops.resize_points_normals(p, n)
    rp2, rn2 = IR.resize_points_normals(rp, rn)
    _same_nan(p2.cpu().numpy(), rp2)
    _same_nan(n2.cpu().numpy(), rn2)


@pytest.mark.parametrize("depth_mode", [False, True])
@pytest.mark.parametrize("level", [0, 1])
def test_icp_step_matches_the_restatement(frames, depth_mode, level):
    from sobfu_amd import ops

    d0, d1 = frames
    for _ in range(level):
        d0, d1 = IR.depth_pyramid(d0, 0.04), IR.depth_pyramid(d1, 0.04)
    li = tuple(float(np.float32(np.float32(v) / np.float32(1 << level))) for v in INTR)
    if depth_mode:
        c, nc = IR.normals_mask_depth(d1, li)
        p, np_ = IR.normals_mask_depth(d0, li)
    else:
        c, nc = IR.point_normals(d1, li)
        p, np_ = IR.point_normals(d0, li)
    aff = IR.pose(IR.rot((0.2, 1.0, 0.1), 1.5), (0.008, -0.01, 0.007)).astype(np.float32)  # near, not at, the truth
    A, b, count, rms, codes = ops.icp_step(level, INTR, _dev(c), _dev(nc), _dev(p), _dev(np_), aff, 0.1, np.deg2rad(20), codes=True)
    rcodes, rrow, margin, every = IR.correspond(level, INTR, c, nc, p, np_, aff, 0.1, np.deg2rad(20), unmasked=True)
    differ = codes != rcodes
    assert (margin[differ] < 1e-6).all(), (int(differ.sum()), np.unique(codes[differ]), np.unique(rcodes[differ]))
    assert differ.sum() <= 5
    assert count > 1000
    # the sums, always: the reference's rows over the GPU's inlier mask (the differing pixels, shown marginal above, follow the GPU's
    # decision); the count exactly, the rest within the derived (m + 10) 2^-24 sabs of icp_cases.sums_error -- 15 2^-24 ~ 9e-7 here
    s, sabs = K.sums_over(every, codes == 0)
    frac = K.sums_error(K.pack(A, b, count, rms), s, sabs, *rcodes.shape)
    print(f"\nlevel {level} depth {depth_mode}: differing pixels {int(differ.sum())}, largest sums error / bound {frac:.3f}")


def _li(level):
    return tuple(float(np.float32(np.float32(v) / np.float32(1 << level))) for v in INTR)


def _pyramids(d, levels, depth_mode):
    from sobfu_amd import ops

    dd = [_dev(d)]
    for _ in range(1, levels):
        dd.append(ops.depth_pyramid(dd[-1], 0.04))
    if depth_mode:
        nn = [ops.normals_mask_depth(x, _li(i)) for i, x in enumerate(dd)]
        return dd, nn
    pn = [ops.point_normals(x, _li(i)) for i, x in enumerate(dd)]
    return [a for a, _ in pn], [b for _, b in pn]


def _errors(aff, truth):
    return np.abs(aff[:3, 3] - truth[:3, 3]).max(), IR.rot_angle_deg(aff[:3, :3].astype(np.float64).T @ truth[:3, :3])


@pytest.mark.parametrize("depth_mode", [False, True])
def test_icp_estimate_recovers_the_motion(frames, depth_mode):
    from sobfu_amd import ops

    c, nc = _pyramids(frames[1], 3, depth_mode)
    p, np_ = _pyramids(frames[0], 3, depth_mode)
    icp = ops.ICP(0.1, np.deg2rad(20), (10, 5, 4, 0))
    ok, aff = icp.estimate(INTR, c, nc, p, np_)
    assert ok
    terr, rerr = _errors(aff, TRUTH)
    assert terr < 1e-3, terr
    # depth mode reprojects the millimetre depth of both frames: its normals carry the quantisation, and the estimate a bias of ~0.15 deg
    assert rerr < (0.1 if not depth_mode else 0.2), rerr
    ok2, aff2 = icp.estimate(INTR, c, nc, p, np_)
    assert ok2 and np.array_equal(aff.view(np.int32), aff2.view(np.int32))  # bitwise reproducible
    trace = icp.trace.cpu().numpy().reshape(-1, 2)
    assert (trace[:, 0] > 100).all() and np.isfinite(trace).all()


def test_identical_frames_give_exactly_identity(frames):
    from sobfu_amd import ops

    c, nc = _pyramids(frames[0], 3, False)
    ok, aff = ops.icp_estimate(INTR, c, nc, c, nc)
    assert ok and np.array_equal(aff, np.eye(4, dtype=np.float32))


def test_empty_frame_fails_with_a_finite_pose(frames):
    from sobfu_amd import ops

    c, nc = _pyramids(np.zeros_like(frames[0]), 3, False)
    p, np_ = _pyramids(frames[0], 3, False)
    icp = ops.ICP()
    ok, aff = icp.estimate(INTR, c, nc, p, np_)
    assert not ok and np.isfinite(aff).all()
    assert icp.failure() == (2, 0)  # the first solve, at the coarsest level


def test_estimate_replays_from_a_graph(frames):
    from sobfu_amd import ops

    c, nc = _pyramids(frames[1], 3, False)
    p, np_ = _pyramids(frames[0], 3, False)
    icp = ops.ICP()
    ok, eager = icp.estimate(INTR, c, nc, p, np_)
    assert ok
    icp.pose.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            icp.enqueue(INTR, c, nc, p, np_)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert int(icp.status.item()) == 0
    assert np.array_equal(icp.pose.cpu().numpy().reshape(4, 4).view(np.int32), eager.view(np.int32))
