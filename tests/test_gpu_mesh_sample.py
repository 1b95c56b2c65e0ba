"""Area-weighted mesh sampling, the F-score counts and evaluate.f_score on the GPU: the kernels of
sobfu_amd/csrc/mesh_sample_kernels.hip against the numpy restatement tests/mesh_sample_reference.py bit for bit (tests/test_mesh_sample_cpu.py
holds the restatement to the header and checks its statistics), every sample on its triangle, the edges of the C ABI, distance_score against
numpy's counts, f_score against closed forms, SobFusion.evaluate(f_score=...) and the headless app's --evaluate-fscore."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_sample_reference as MS

SEEDS, cases, same_bits = MS.SEEDS, MS.cases, MS.same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
MARGIN = 1e-4  # kMeshMargin (sobfu_amd/csrc/sobfu_mesh.hpp): x L bounds the fp32 error of one point-triangle distance


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sample(v, f, density, seed):
    from sobfu_amd import ops

    vd, fd = _gpu(v), _gpu(f)
    p, tri, bary, areas = ops.mesh_sample(vd, fd, density=density, seed=seed, tri=True, bary=True, areas=True)
    rc, total, ws, _ = ops.mesh_sample_count(vd, fd, density, seed)
    assert rc == 0
    T = len(f)
    counts = _cpu(ws)[64:64 + 4 * T].view(np.int32).astype(np.int64)  # behind the header of 16 ints
    return dict(points=_cpu(p), tri=_cpu(tri), bary=_cpu(bary), areas=_cpu(areas), counts=counts), total


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0].replace(" ", "_"))
def test_the_kernels_equal_the_restatement_bit_for_bit(case, seed):
    name, v, f, density = case
    want = MS.sample(v, f, density, seed)
    got, total = _sample(v, f, density, seed)
    again, total2 = _sample(v, f, density, seed)
    print("%s, seed %d: %d triangles, %d samples" % (name, seed, len(f), total))
    assert total == total2 == len(want["points"]) == int(want["counts"].sum())
    same_bits(got, want, name)
    same_bits(again, got, name + ", run to run")
    assert np.all(got["points"][:, 3] == 1)


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0].replace(" ", "_"))
def test_every_sample_lies_on_its_triangle(case):
    from sobfu_amd import ops

    name, v, f, density = case
    vd, fd = _gpu(v), _gpu(f)
    grid = ops.TriangleGrid(vd, fd)
    p, tri = grid.sample(density=density, seed=3, tri=True)
    L = float(np.max(np.abs(np.concatenate([grid.origin, grid.origin + np.float32(grid.h) * np.asarray(grid.dims, np.float32)]))))
    d = _cpu(grid.query(p)[0])
    ph, th = _cpu(p), _cpu(tri)
    a, b, c = MS.corners(v, f)
    own = MS.point_triangle_distance(ph[:, :3], a[th], b[th], c[th])
    print("%s: %d samples, L = %.4g, max distance to the mesh %.3g, to the sample's own triangle %.3g, bound %.3g" % (name, len(d), L, d.max(), own.max(), MARGIN * L))
    assert len(d) > 300 and d.max() <= MARGIN * L and own.max() <= MARGIN * L


def test_edges():
    from sobfu_amd import ops

    v, f = MS.box()
    vd, fd = _gpu(v), _gpu(f)
    import torch

    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    rc, total, ws, _ = ops.mesh_sample_count(vd, none, 100.0)
    assert (rc, total) == (0, 0) and ops.mesh_sample(vd, none, density=100.0).shape == (0, 4)
    assert ops.mesh_sample_generate(vd, none, 0, ws, 0)[0] == 0
    rc, total, ws, areas = ops.mesh_sample_count(vd, fd, 0.0, areas=True)
    assert (rc, total) == (0, 0) and ops.mesh_sample(vd, fd, density=0.0).shape == (0, 4)
    assert np.array_equal(_cpu(areas).view(np.uint64), MS.areas(v, f).view(np.uint64))
    p, tri, bary = ops.mesh_sample(vd, fd, density=0.0, tri=True, bary=True)
    assert p.shape == (0, 4) and tri.shape == (0,) and bary.shape == (0, 2)
    # bad input: the flag, after the synchronisation; generate through that workspace is refused
    bad = f.copy()
    bad[5, 2] = 8
    rc, total, ws, _ = ops.mesh_sample_count(vd, _gpu(bad), 100.0)
    assert rc == -1
    assert ops.mesh_sample_generate(vd, _gpu(bad), 0, ws, 1000)[0] == -1
    assert ops.mesh_sample_generate(vd, fd, 0, ws, 1000)[0] == -1
    bad[5, 2] = -1
    assert ops.mesh_sample_count(vd, _gpu(bad), 100.0)[0] == -1
    nan = v.copy()
    nan[6, 0] = np.nan
    assert ops.mesh_sample_count(_gpu(nan), fd, 100.0)[0] == -1
    nan[6, 0] = np.inf
    assert ops.mesh_sample_count(_gpu(nan), fd, 100.0)[0] == -1
    with pytest.raises(ops._lib.HipError):
        ops.mesh_sample(_gpu(nan), fd, density=100.0)
    # more samples than an int holds: the total is still reported, nothing of that size is allocated
    tv, tf = MS.unit_right_triangle()
    rc, total, ws, _ = ops.mesh_sample_count(_gpu(tv), _gpu(tf), 1e10)
    print("area 1/2 at density 1e10: rc %d, total %d" % (rc, total))
    assert rc == -3 and abs(total - 5_000_000_000) <= 1 and ws.numel() < 1024
    assert ops.mesh_sample_generate(_gpu(tv), _gpu(tf), 0, ws, 16)[0] == -1
    rc, total, ws, _ = ops.mesh_sample_count(_gpu(tv), _gpu(tf), 1e300)
    assert rc == -3 and total >= 1 << 62
    # never truncates
    rc, total, ws, _ = ops.mesh_sample_count(vd, fd, 1150.3)
    assert rc == 0 and total > 1000
    assert ops.mesh_sample_generate(vd, fd, 0, ws, total - 1)[0] == -1
    rc, p, _, _ = ops.mesh_sample_generate(vd, fd, 0, ws, total + 5)
    assert rc == 0 and np.array_equal(_cpu(p)[:total].view(np.uint32), MS.sample(v, f, 1150.3, 0)["points"].view(np.uint32))
    assert ops.mesh_sample_generate(vd, fd[:11].contiguous(), 0, ws, total)[0] == -1  # counted for another mesh
    with pytest.raises(ValueError):
        ops.mesh_sample(vd, fd)
    with pytest.raises(ValueError):
        ops.mesh_sample(vd, fd, density=1.0, n=5)


@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0].replace(" ", "_"))
def test_n_lands_within_the_number_of_triangles(case):
    from sobfu_amd import ops

    name, v, f, _ = case
    for n in (0, 1, 1000, 12345):
        got = int(ops.mesh_sample(_gpu(v), _gpu(f), n=n, seed=7).shape[0])
        print("%s: n = %d -> %d samples (%d triangles)" % (name, n, got, len(f)))
        assert abs(got - n) <= len(f)


@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("n", [0, 1, 65, 4099])
def test_distance_score_equals_numpys_counts(n, K):
    from sobfu_amd import ops

    rng = np.random.default_rng(n + K)
    th = rng.uniform(0.0, 1.0, K).astype(np.float32)  # unsorted
    d = rng.uniform(0.0, 1.2, n).astype(np.float32)
    if n:
        d[rng.integers(0, n, max(1, n // 7))] = rng.choice(th, max(1, n // 7))  # exact ties
    if n > 1:
        d[rng.integers(0, n, n // 9 + 1)] = np.inf
        d[rng.integers(0, n, n // 11 + 1)] = np.nan
        d[rng.integers(0, n, n // 13 + 1)] = -np.inf
    dd = _gpu(d)
    own = _cpu(dd)
    within, finite = ops.distance_score(dd, th)
    fin = np.isfinite(own)
    want = np.array([int((fin & (own <= t)).sum()) for t in th], np.int64)
    print("n %d K %d: finite %d, ties %d, within %s" % (n, K, finite, int(np.isin(own, th).sum()), within.tolist()))
    assert within.dtype == np.int64 and np.array_equal(within, want) and finite == int(fin.sum())
    again, finite2 = ops.distance_score(dd, th)  # run to run
    assert np.array_equal(again, within) and finite2 == finite


def test_distance_score_refuses_bad_threshold_counts():
    from sobfu_amd import ops

    d = _gpu(np.zeros(4, np.float32))
    for th in ([], [0.1] * 17):
        with pytest.raises(ValueError):
            ops.distance_score(d, th)


def test_f_score_of_two_parallel_squares_is_exact():
    from sobfu_amd.evaluate import f_score

    delta = 2.0 ** -5
    (av, af), (bv, bf) = MS.rectangle(1.0, 1.0, 0.0), MS.rectangle(1.0, 1.0, delta)
    r = f_score(av, af, bv, bf, [delta / 2, 2 * delta], density=4000.0, seed=11)
    print(r)
    assert r["a_samples"] == 4000 and r["b_samples"] == 4000 and r["thresholds"] == [delta / 2, 2 * delta]
    assert r["precision"] == [0.0, 1.0] and r["recall"] == [0.0, 1.0] and r["f"] == [0.0, 1.0]
    assert r["a_to_b"]["n"] == 4000 and r["a_to_b"]["within"] == 4000 and abs(r["chamfer"] - delta) < 1e-6 and abs(r["hausdorff"] - delta) < 1e-6
    # beyond max_dist a sample has no match: a miss in the denominator
    far = f_score(av, af, bv, bf, [2 * delta], density=4000.0, seed=11, max_dist=delta / 4)
    assert far["precision"] == [0.0] and far["recall"] == [0.0] and far["f"] == [0.0] and far["a_to_b"]["within"] == 0
    m = f_score(av, af, bv, bf, [2 * delta], n=3000)
    assert abs(m["a_samples"] - 3000) <= 2 and abs(m["b_samples"] - 3000) <= 2
    with pytest.raises(ValueError):
        f_score(av, af, bv, bf, [delta])


def test_f_score_recall_of_half_a_rectangle():
    """A = [0, 1]^2, B = [0, 2] x [0, 1], coplanar: every sample of A lies on B; a sample of B is within tau of A iff x <= 1 + tau"""
    from sobfu_amd import ops
    from sobfu_amd.evaluate import compare_meshes, f_score

    (av, af), (bv, bf) = MS.rectangle(1.0, 1.0), MS.rectangle(2.0, 1.0)
    taus, seed, density = [0.3, 0.45, 0.26], 5, 10000.0
    r = f_score(av, af, bv, bf, taus, density=density, seed=seed)
    restated = MS.sample(bv, bf, density, seed + 1)
    d = _cpu(ops.TriangleGrid(_gpu(av), _gpu(af)).query(_gpu(restated["points"]))[0])
    N = len(d)
    vertex_only = compare_meshes(av, af, bv, bf)
    print("vertex-only compare_meshes: chamfer %.6g hausdorff %.6g b_to_a.mean %.6g (4 vertices); sampled: chamfer %.6g hausdorff %.6g b_to_a.mean %.6g (%d samples)" %
          (vertex_only["chamfer"], vertex_only["hausdorff"], vertex_only["b_to_a"]["mean"], r["chamfer"], r["hausdorff"], r["b_to_a"]["mean"], N))
    assert r["a_samples"] == 10000 and r["b_samples"] == N == 20000
    assert r["precision"] == [1.0, 1.0, 1.0]
    for tau, rec, p_, f_ in zip(r["thresholds"], r["recall"], r["precision"], r["f"]):
        p = (1.0 + tau) / 2.0
        sigma = np.sqrt(p * (1.0 - p) / N)
        print("tau %.9g: recall %.6f, expected %.6f, %.2f sigma" % (tau, rec, p, (rec - p) / sigma))
        assert abs(rec - p) <= 5.0 * sigma
        assert rec == int((d <= np.float32(tau)).sum()) / N
        assert f_ == 2.0 * p_ * rec / (p_ + rec)


def test_sobfusion_evaluate_with_f_score():
    from sobfu_amd import synthetic as S
    from sobfu_amd.evaluate import compare_meshes, f_score, format_f_score
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    import mesh_distance_reference as MD

    P = read_ini(CONFIG1)
    fusion = SobFusion(P)
    try:
        for n in range(2):
            fusion(_gpu(S.render_sphere_depth((0.005 * n, 0.0, 0.75), 0.1, P["intr"])))
        gv, gf = MD.icosphere(0.1, 3, (0.0, 0.0, -0.75))
        args = dict(thresholds=[0.002, 0.005], n=5000, seed=3)
        r, v, f, posed = fusion.evaluate(gv, gf, return_meshes=True, f_score=args)
        plain = fusion.evaluate(gv, gf)
        assert sorted(r) == ["a_to_b", "b_to_a", "chamfer", "f_score", "hausdorff"]
        assert plain == compare_meshes(v, f, gv, gf) and {k: r[k] for k in plain} == plain
        want = f_score(v, f, posed, gf, **args)
        print(format_f_score(want))
        # the model is the part of the sphere the camera saw: the ground truth is the larger mesh, and n lands on it
        assert r["f_score"] == want and abs(want["b_samples"] - 5000) <= len(gf) and 0 < want["a_samples"] < want["b_samples"]
        assert 0.0 <= want["f"][0] <= want["f"][1] <= 1.0 and want["f"][1] > 0.0
        live = fusion.evaluate(gv, gf, which="live", f_score=args)
        assert sorted(live) == sorted(r)
    finally:
        fusion.close()


EVAL = re.compile(r"^evaluate canonical (\d+): (.*)$", re.M)
FSCORE = re.compile(r"^fscore canonical (\d+): (.*)$", re.M)


def test_app_evaluate_fscore(tmp_path):
    from sobfu_amd import build_host, mesh_io
    from sobfu_amd.evaluate import f_score, format_f_score
    from sobfu_amd.params import read_ini

    import mesh_distance_reference as MD

    exe = build_host.build_app()  # over the library the package has loaded: nothing of it is built here
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    gv, gf = MD.icosphere(0.1, 4, (0.0, 0.0, -0.75))
    mesh_io.write_ply(tmp_path / "gt.ply", gv, gv, gf)
    common = [exe, CONFIG1, "--no-stats", "--synthetic", "2", "--evaluate", str(tmp_path / "gt.ply")]
    flags = ["--evaluate-fscore", "0.002,0.005", "--evaluate-samples", "20000"]
    r = subprocess.run(common + flags + ["--mesh", str(meshes), "--mesh-format", "ply"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    ((n, evaluated),), ((m, line),) = EVAL.findall(r.stdout), FSCORE.findall(r.stdout)
    print("fscore: " + line)
    assert int(n) == int(m) == 1 and r.stdout.index("evaluate canonical") < r.stdout.index("fscore canonical")
    limit = float(np.float32(5) * np.float32(read_ini(CONFIG1)["trunc"]))
    mv, _, mf, _ = mesh_io.read_ply(meshes / "phi_global_1.ply")
    pv, _, pf, _ = mesh_io.read_ply(tmp_path / "gt.ply")
    want = f_score(mv, mf, pv, pf, np.array([0.002, 0.005], np.float32), n=20000, seed=0, max_dist=limit)
    assert line == format_f_score(want)  # number for number at %.9g
    assert abs(want["b_samples"] - 20000) <= len(pf) and 0 < want["a_samples"] < want["b_samples"]  # the whole sphere is the larger mesh
    # the evaluate line does not notice the new flags; a density and a seed of one's own
    r0 = subprocess.run(common, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and EVAL.findall(r0.stdout) == [(n, evaluated)] and not FSCORE.findall(r0.stdout)
    r1 = subprocess.run(common + ["--evaluate-fscore", "0.004", "--evaluate-density", "150000", "--evaluate-seed", "4294967301"], capture_output=True, text=True,
                        timeout=600)
    assert r1.returncode == 0, r1.stdout[-3000:]
    assert FSCORE.findall(r1.stdout)[0][1] == format_f_score(f_score(mv, mf, pv, pf, np.array([0.004], np.float32), density=150000.0, seed=(1 << 32) + 5, max_dist=limit))
    bad = {"--evaluate-fscore": [["--evaluate-fscore", "0.002,,0.005"], ["--evaluate-fscore", "0.002,x"], ["--evaluate-fscore", "0.002,-0.001"],
                                 ["--evaluate-fscore", "0"], ["--evaluate-fscore", ",".join(["0.001"] * 17)], ["--evaluate-fscore", ""]],
           "--evaluate-samples": [flags + ["--evaluate-density", "100"], ["--evaluate-samples", "100"], ["--evaluate-fscore", "0.002", "--evaluate-samples", "-3"]],
           "--evaluate-density": [["--evaluate-density", "100"], ["--evaluate-fscore", "0.002", "--evaluate-density", "nan"]],
           "--evaluate-seed": [["--evaluate-seed", "3"]]}
    for flag, lists in bad.items():
        for extra in lists:
            rb = subprocess.run(common + extra, capture_output=True, text=True, timeout=60)
            assert rb.returncode == 2 and flag in rb.stdout and len(rb.stdout.strip().splitlines()) == 1, (extra, rb.stdout[-500:])
    rb = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "2"] + flags, capture_output=True, text=True, timeout=60)
    assert rb.returncode == 2 and "--evaluate-fscore" in rb.stdout
