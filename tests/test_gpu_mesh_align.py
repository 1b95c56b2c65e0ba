"""Rigid alignment of a point list to a mesh on the GPU (sobfu_amd/csrc/mesh_align_kernels.hip) against its float64 twin
tests/mesh_align_reference.py.  The twin takes (tri, closest) from TriangleGrid.query on the same transformed points -- that answer is
pinned bit for bit in tests/test_gpu_mesh_distance.py -- so only the arithmetic of the alignment is under test here.

Bounds: a sum against the twin's correctly rounded one: n 2^-52 sum |terms| (float64 sums of the same terms in another order); a pose after
one solve: 1 float32 ulp per entry (float64 error times the system's condition number, about 7e3, is far below it); a point after a
converged alignment on exact data: 1e-4 L, the bound kMeshMargin on one fp32 point-triangle answer (L = the largest coordinate); a point
on inexact data: the rms residual at the true pose.  Measured slack: profiles/mesh_align.md."""
import numpy as np
import pytest

import mesh_align_reference as MA

pytestmark = pytest.mark.gpu
MD = MA.MD
COUNTS = [1, 63, 64, 65, 256, 257, 642, 2562, 70001]


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


class Scene:
    def __init__(self):
        from sobfu_amd import ops

        self.gv, self.gf = MA.ellipsoid(3)
        self.grid = ops.TriangleGrid(_gpu(self.gv), _gpu(self.gf))
        self.L = float(np.abs(self.gv[:, :3]).max())
        self.T = {k: MA.motion(*k) for k in ((3.0, 5.0), (15.0, 30.0))}
        self.start = self.T[(3.0, 5.0)].astype(np.float32)  # the 3 degree / 5 mm pose
        self.fine = MA.ellipsoid(4)[0]
        assert self.gv.shape == (642, 4) and self.fine.shape == (2562, 4)

    def points(self, n):
        if n <= 642:
            return self.gv[:n].copy()
        return np.tile(self.fine, (n // 2562 + 1, 1))[:n].copy()

    def twin_sums(self, grid, vertices, faces, points, pose, max_dist=None):
        s = MA.transform(points, pose)
        _, tri, closest = grid.query(_gpu(s), max_dist, closest=True)
        return MA.sums(*MA.rows(points, s, tri.cpu().numpy(), closest.cpu().numpy(), vertices, faces))


@pytest.fixture(scope="module")
def scene():
    return Scene()


def _check_sums(got, want, bounds, what):
    err = np.abs(got - want)
    slack = np.where(bounds > 0, err / np.where(bounds > 0, bounds, 1), 0).max()
    print("%s: inliers %d, largest |sum - twin| / bound = %.3g" % (what, int(got[27]), slack))
    assert got[27] == want[27], what
    assert np.all(err <= bounds), (what, err, bounds)


@pytest.mark.parametrize("n", COUNTS)
def test_step_parity(scene, n):
    pts = scene.points(n)
    want, bounds = scene.twin_sums(scene.grid, scene.gv, scene.gf, pts, scene.start)
    got = scene.grid.align_step(_gpu(pts), scene.start)
    assert want[27] == n
    _check_sums(got, want, bounds, "n = %d" % n)
    if n in (65, 2562, 70001):
        for mode in ("grid", "brute"):
            assert np.array_equal(_bits(scene.grid.align_step(_gpu(pts), scene.start, mode=mode)), _bits(got)), mode


def test_outliers_are_left_out(scene):
    from sobfu_amd import ops

    # the target plus a zero-area triangle (three collinear corners) away from the ellipsoid
    gv = np.concatenate([scene.gv, np.array([[0.3, 0.2, -0.75, 1], [0.32, 0.2, -0.75, 1], [0.34, 0.2, -0.75, 1]], np.float32)])
    gf = np.concatenate([scene.gf, np.array([[642, 643, 644]], np.int32)])
    grid = ops.TriangleGrid(_gpu(gv), _gpu(gf))
    base, max_dist = scene.fine.copy(), 0.02
    inv = MA.rigid_inverse(scene.start).astype(np.float64)  # so that the extra points land where they are meant to after the pose
    far = MA.moved(np.array([[0.02, -0.01, -0.5, 1], [0.6, 0.0, -0.75, 1], [0.02, 0.4, -0.75, 1], [-0.3, -0.3, -1.0, 1], [0.02, -0.01, -0.75, 1]], np.float32), inv)
    bad = np.array([[np.nan, 0, -0.75, 1], [0.02, np.inf, -0.75, 1], [0.02, -0.01, -np.inf, 1], [np.nan, np.nan, np.nan, 1]], np.float32)
    flat = MA.moved(np.array([[0.31, 0.201, -0.75, 1], [0.33, 0.2, -0.749, 1], [0.345, 0.2, -0.75, 1]], np.float32), inv)
    extra = np.concatenate([far, bad, flat])
    at = [0, 1, 63, 64, 255, 256, 257, 1000, 1500, 2000, 2561, 2562]  # positions in the base list: other lanes, waves and workgroups
    pts = np.insert(base, at, extra, axis=0)
    assert len(pts) == len(base) + 12
    want, bounds = scene.twin_sums(grid, gv, gf, base, scene.start, max_dist)
    assert want[27] == len(base)  # every point of the list without them is an inlier
    s = MA.transform(flat, scene.start)
    _, tri = grid.query(_gpu(s), max_dist)
    assert list(tri.cpu().numpy()) == [1280] * 3  # their nearest triangle is the zero-area one
    got = grid.align_step(_gpu(pts), scene.start, max_dist=max_dist)
    assert got[27] == len(pts) - 12
    _check_sums(got, want, bounds, "with 12 outliers")
    twin_all, _ = scene.twin_sums(grid, gv, gf, pts, scene.start, max_dist)
    assert twin_all[27] == want[27]  # the twin leaves the same points out


@pytest.mark.parametrize("dof", [6, 3])
def test_one_solve(scene, dof):
    pts = scene.fine
    want_sums, _ = scene.twin_sums(scene.grid, scene.gv, scene.gf, pts, scene.start)
    want, ok, th, tn = MA.update(scene.start, want_sums, dof)
    A, _ = MA.unpack(want_sums)
    print("dof %d: condition number %.3g" % (dof, np.linalg.cond(A if dof == 6 else A[3:, 3:])))
    pose, info = scene.grid.align(_gpu(pts), scene.start, iters=1, dof=dof)
    got = pose.cpu().numpy()
    assert ok and info["status"] == 0 and info["iterations"] == 1 and not info["failed"] and not info["converged"]
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(got), np.abs(want)))
    print("largest difference: %.3g ulp; differing entries: %d" % (ulps.max(), int((ulps > 0).sum())))
    assert np.all(ulps <= 1.0)
    assert np.array_equal(_bits(got[3]), _bits(scene.start[3]))
    tr = info["trace"]
    assert tr.shape == (1, 4) and tr[0, 0] == len(pts) and abs(tr[0, 2] - th) <= 1e-6 * th + 1e-12 and abs(tr[0, 3] - tn) <= 1e-6 * tn
    assert abs(tr[0, 1] - np.sqrt(want_sums[28] / want_sums[27])) <= 1e-6 * tr[0, 1]
    if dof == 3:
        assert np.array_equal(_bits(got[:3, :3]), _bits(scene.start[:3, :3])) and tr[0, 2] == 0


@pytest.mark.parametrize("start", [(3.0, 5.0), (15.0, 30.0)])
def test_known_answer(scene, start):
    import torch

    T = scene.T[start]
    src = MA.moved(scene.gv, np.linalg.inv(T))  # the pose T carries them back onto the target's own vertices
    trace = torch.full((20, 4), -7.0, dtype=torch.float32, device="cuda")
    pose, info = scene.grid.align(_gpu(src), None, iters=20, eps_rot=1e-6, eps_trans=1e-6, trace=trace)
    done = info["iterations"]
    print("start %s: status %#x, trace\n%s" % (start, info["status"], info["trace"]))
    assert info["converged"] and not info["failed"] and info["status"] == (0x20000 | done) and 0 < done < 20
    tr = trace.cpu().numpy()
    assert np.all(tr[done:] == -7.0) and np.all(tr[:done] != -7.0) and np.array_equal(tr[:done], info["trace"])
    assert tr[done - 1, 2] < 1e-6 and tr[done - 1, 3] < 1e-6 and (done == 1 or not (tr[done - 2, 2] < 1e-6 and tr[done - 2, 3] < 1e-6))
    err = np.linalg.norm(MA.transform(src, pose.cpu().numpy())[:, :3].astype(np.float64) - scene.gv[:, :3], axis=1).max()
    print("largest distance to the known position: %.3g m (bound %.3g)" % (err, 1e-4 * scene.L))
    assert err <= 1e-4 * scene.L


def test_inexact_data(scene):
    T = scene.T[(3.0, 5.0)]
    src = MA.moved(scene.fine, np.linalg.inv(T))
    s = scene.grid.align_step(_gpu(src), T.astype(np.float32))
    rms_true = float(np.sqrt(s[28] / s[27]))
    assert s[27] == len(src) and 1e-4 < rms_true < 3e-4
    pose, info = scene.grid.align(_gpu(src), None, iters=20)
    assert info["status"] == 0 and info["iterations"] == 20 and info["trace"].shape == (20, 4)
    err = np.linalg.norm(MA.transform(src, pose.cpu().numpy())[:, :3].astype(np.float64) - scene.fine[:, :3], axis=1).max()
    print("rms residual at the true pose %.6g m, last rms %.6g m, largest distance to the true position %.3g m" % (rms_true, info["trace"][-1, 1], err))
    assert err <= rms_true


def test_translation_only(scene):
    from sobfu_amd import ops

    sv, sf = MD.icosphere(0.1, 3, (0.0, 0.0, -0.75))
    src = sv.copy()
    src[:, 0] -= np.float32(0.004)
    pose, info = ops.TriangleGrid(_gpu(sv), _gpu(sf)).align(_gpu(src), None, iters=5, dof=3)
    got = pose.cpu().numpy()
    L = float(np.abs(sv[:, :3]).max())
    print("recovered shift %s (one step: |t_inc| = %.9g)" % (got[:3, 3], info["trace"][0, 3]))
    assert info["status"] == 0 and np.array_equal(_bits(got[:3, :3]), _bits(np.eye(3, dtype=np.float32)))
    assert np.abs(got[:3, 3].astype(np.float64) - np.array([0.004, 0.0, 0.0])).max() <= 1e-4 * L
    assert np.all(info["trace"][:, 2] == 0)


@pytest.mark.parametrize("dof", [6, 3])
def test_failure_keeps_the_pose(scene, dof):
    import torch

    from sobfu_amd import ops

    qv = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [1, 1, 0, 1], [0, 1, 0, 1]], np.float32)
    qf = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rng = np.random.default_rng(4)
    pts = np.ones((300, 4), np.float32)
    pts[:, :3] = rng.uniform((0.1, 0.1, 0.05), (0.8, 0.9, 0.5), (300, 3))
    start = np.eye(4, dtype=np.float32)
    start[0, 3] = 0.0625
    square = ops.TriangleGrid(_gpu(qv), _gpu(qf))
    for grid, p, max_dist, inliers in ((square, pts, None, 300), (square, pts, 1e-3, 0), (scene.grid, scene.fine, 1e-7, None),
                                      (square, pts[:0], None, None)):
        trace = torch.full((4, 4), -7.0, dtype=torch.float32, device="cuda")
        pose, info = grid.align(_gpu(p), start, iters=4, dof=dof, max_dist=max_dist, trace=trace)
        assert info["status"] == 0x10000 and info["failed"] and not info["converged"] and info["iterations"] == 0
        assert np.array_equal(_bits(pose.cpu().numpy()), _bits(start))
        tr = trace.cpu().numpy()
        assert np.all(tr[1:] == -7.0)
        if inliers is not None:
            assert tr[0, 0] == inliers and info["trace"].shape == (1, 4)


def test_determinism(scene):
    src = MA.moved(scene.fine, np.linalg.inv(scene.T[(3.0, 5.0)]))
    runs = []
    for _ in range(2):
        pose, info = scene.grid.align(_gpu(src), None, iters=10)
        runs.append((pose.cpu().numpy(), info["status"], info["trace"]))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and runs[0][1] == runs[1][1] == 0
    assert np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))
    sums = [scene.grid.align_step(_gpu(src), scene.start) for _ in range(2)]
    assert np.array_equal(_bits(sums[0]), _bits(sums[1]))
