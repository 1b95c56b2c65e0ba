"""Reconstruction error against a ground-truth mesh on the GPU: SobFusion.evaluate on config 1's translating sphere against an icosphere
of the analytic sphere, the solve left bit for bit as it is, the headless app's --evaluate / --evaluate-live / --error-mesh against the
Python front end on the files the app wrote, and the C++ compare_meshes against the Python one.

Measured on the MI355X (three frames, 5 mm per frame, metres; a = the model, b = the icosphere of 5120 faces): see profiles/mesh_distance.md."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_distance_reference as MD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
SHIFT, FRAMES = 0.005, 3
STATE = ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi", "psi", "psi_inv")


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _params():
    from sobfu_amd.params import read_ini

    return read_ini(CONFIG1)


def _gt(frame):
    """the analytic sphere of frame n -- centre (shift n, 0, 0.75), r = 0.1 in the camera frame -- in the frame of the meshes the app
    writes, (x, -y, -z): an icosphere of 5120 faces"""
    return MD.icosphere(0.1, 4, (SHIFT * frame, 0.0, -0.75))


def _rel(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b))


def _printed(got, want):
    """a value the app printed at %.9g against the Python one: relative 1e-9 (float64 sums in another order) plus the print's own
    rounding, half a unit of the ninth significant digit (up to 5e-9 relative when the leading digit is 1)"""
    half_digit = 0.5 * 10.0 ** (np.floor(np.log10(abs(want))) - 8) if want else 0.0
    return abs(got - want) <= 1e-9 * abs(want) + half_digit


def _flat(r):
    return {"%s.%s" % (s, k): r[s][k] for s in ("a_to_b", "b_to_a") for k in ("n", "within", "mean", "rms", "median", "max")} | {
        "chamfer": r["chamfer"], "hausdorff": r["hausdorff"]}


def test_sobfusion_evaluate_and_the_solve_is_untouched():
    from sobfu_amd import ops, synthetic as S
    from sobfu_amd.evaluate import compare_meshes, format_result
    from sobfu_amd.fusion import SobFusion

    P = _params()
    gv0, gf = _gt(0)
    assert len(gf) == 5120
    runs = []
    for probe in (True, False):
        f = SobFusion(P)
        for n in range(FRAMES):
            f(_gpu(S.render_sphere_depth((SHIFT * n, 0.0, 0.75), 0.1, P["intr"])))
            if not probe:
                continue
            for which, gv in (("canonical", gv0), ("live", _gt(n)[0])):
                r, mv, mf, gvd = f.evaluate(gv, gf, which=which, return_meshes=True)
                v, _, faces = ops.marching_cubes_indexed(f.phi_global, P["size"], P["R"], P["t"])
                if which == "live":
                    v = f.warp_to_live(v)
                assert np.array_equal(_bits(_cpu(mv)), _bits(_cpu(v))) and np.array_equal(_cpu(mf), _cpu(faces))
                by_hand = compare_meshes(_cpu(v), _cpu(faces), gv, gf)  # on the downloaded meshes
                assert r == by_hand and f.evaluate(_gpu(gv), _gpu(gf), which=which) == r
                print("frame %d %s: %s" % (n, which, format_result(r)))
                assert r["a_to_b"]["n"] == len(_cpu(v)) > 100 and r["a_to_b"]["within"] == r["a_to_b"]["n"] and r["b_to_a"]["n"] == len(gv)
                assert 0 < r["a_to_b"]["mean"] < float(P["trunc"])
                assert r["a_to_b"]["mean"] <= r["a_to_b"]["rms"] <= r["a_to_b"]["max"] <= r["hausdorff"]
            capped = f.evaluate(gv0, gf, max_dist=0.001)
            assert capped["a_to_b"]["within"] < capped["a_to_b"]["n"] and capped["a_to_b"]["max"] <= 0.001
            moved = np.eye(4, dtype=np.float32)
            moved[0, 3] = 0.25
            shifted = gv0.copy()
            shifted[:, 0] -= np.float32(0.25)
            posed = f.evaluate(shifted, gf, pose=moved)
            assert _rel(posed["a_to_b"]["mean"], f.evaluate(gv0, gf)["a_to_b"]["mean"], 1e-4)  # x - 0.25 + 0.25 rounds
        runs.append({k: _cpu(getattr(f, k)).copy() for k in STATE})
        with pytest.raises(ValueError):
            f.evaluate(gv0, gf, which="phi_n")
        f.close()
    for k in STATE:  # evaluate reads the volumes only
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k


LINE = re.compile(r"^evaluate (canonical|live) (\d+): (.*)$", re.M)


def _parse(text):
    out = {}
    for kv in text.split():
        k, v = kv.split("=")
        out[k] = int(v) if k.endswith(".n") or k.endswith(".within") else float(v)
    return out


def test_app_evaluate(tmp_path):
    from sobfu_amd import build, build_host, mesh_io
    from sobfu_amd.evaluate import compare_meshes

    build.build_hip()
    exe = build_host.build_app()
    meshes, errors = tmp_path / "meshes", tmp_path / "errors"
    meshes.mkdir()
    errors.mkdir()
    for n in range(FRAMES):
        gv, gf = _gt(n)
        nrm = gv.copy()
        nrm[:, :3] = (gv[:, :3] - np.array([SHIFT * n, 0, -0.75], np.float32)) / np.float32(0.1)
        mesh_io.write_ply(tmp_path / ("gt_%06d.ply" % n), gv, nrm, gf)
    r = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", str(FRAMES), "--mesh", str(meshes), "--mesh-format", "ply", "--warp-mesh",
                        "--evaluate", str(tmp_path / "gt_000000.ply"), "--evaluate-live", str(tmp_path / "gt_%06d.ply"), "--error-mesh", str(errors)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = LINE.findall(r.stdout)
    print("\n".join("evaluate %s %s: %s" % l for l in lines))
    assert [(k, int(n)) for k, n, _ in lines] == [("live", 1), ("live", 2), ("canonical", 2)]
    P = _params()
    limit = float(np.float32(5) * np.float32(P["trunc"]))
    for kind, n, text in lines:
        n = int(n)
        name = "phi_global_%d.ply" % n if kind == "canonical" else "phi_global_warped_%d.ply" % n
        mv, mn, mf, _ = mesh_io.read_ply(meshes / name)
        gv, _, gf, _ = mesh_io.read_ply(tmp_path / ("gt_%06d.ply" % (0 if kind == "canonical" else n)))
        want, d_model, _ = compare_meshes(mv, mf, gv, gf, max_dist=limit, return_distances=True)
        got, flat = _parse(text), _flat(want)
        assert sorted(got) == sorted(flat)
        for k in flat:
            assert (got[k] == flat[k]) if isinstance(flat[k], int) else _printed(got[k], flat[k]), (kind, n, k, got[k], flat[k])
        assert 0 < got["a_to_b.mean"] < float(P["trunc"])
        ev, en, ef, ec = mesh_io.read_ply(errors / ("error_%s_%d.ply" % (kind, n)))  # the evaluated mesh, coloured by error
        assert np.array_equal(_bits(ev), _bits(mv)) and np.array_equal(ef, mf) and np.array_equal(_bits(en), _bits(mn)) and ec is not None
        d = _cpu(d_model).astype(np.float64)
        fin = np.nonzero(np.isfinite(d))[0]
        for i in (fin[np.argmin(d[fin])], fin[np.argmax(d[fin])], fin[np.argsort(d[fin])[len(fin) // 2]]):
            t = min(1.0, max(0.0, d[i] / float(np.float32(limit))))
            assert list(ec[i, :3]) == [int(255.0 * (1.0 - t) + 0.5), 0, int(255.0 * t + 0.5)], (kind, n, i, d[i], ec[i])  # b, g, r
        assert len({tuple(c) for c in ec[:, :3]}) > 3
    # a tight limit: unmatched vertices are grey; a pose file moves the ground truth
    pose = tmp_path / "pose.txt"
    pose.write_text("1 0 0 0.25\n0 1 0 0\n0 0 1 0\n0 0 0 1\n")
    gv, _, gf, _ = mesh_io.read_ply(tmp_path / "gt_000000.ply")
    gv[:, 0] -= np.float32(0.25)
    mesh_io.write_ply(tmp_path / "gt_moved.ply", gv, gv, gf)
    r2 = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "2", "--evaluate", str(tmp_path / "gt_moved.ply"), "--evaluate-pose", str(pose),
                         "--evaluate-max-dist", "0.001", "--error-mesh", str(errors)], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-2000:]
    (kind, n, text), = LINE.findall(r2.stdout)
    got = _parse(text)
    assert kind == "canonical" and int(n) == 1 and 0 < got["a_to_b.within"] < got["a_to_b.n"] and got["a_to_b.max"] <= 0.001
    ec = mesh_io.read_ply(errors / "error_canonical_1.ply")[3]
    assert int((ec[:, :3] == 128).all(1).sum()) == got["a_to_b.n"] - got["a_to_b.within"]
    bad = subprocess.run([exe, CONFIG1, "--synthetic", "2", "--evaluate-live", str(tmp_path / "gt_%s.ply")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--evaluate-live" in bad.stdout
    missing = subprocess.run([exe, CONFIG1, "--no-stats", "--synthetic", "1", "--evaluate", str(tmp_path / "nowhere.ply")], capture_output=True, text=True,
                             timeout=600)
    assert missing.returncode == 2 and "cannot read ground truth" in missing.stdout


def test_cpp_compare_meshes_equals_python(tmp_path):
    from sobfu_amd import build, build_host, mesh_io
    from sobfu_amd.evaluate import compare_meshes

    build.build_hip()
    tool = build_host.build_mesh_eval_tool()
    av, af = MD.icosphere(0.1, 3, (0.01, -0.02, 0.5))
    bv, bf = MD.icosphere(0.11, 2, (0.0, 0.0, 0.5))
    mesh_io.write_ply(tmp_path / "a.ply", av, av, af)
    mesh_io.write_ply(tmp_path / "b.ply", bv, bv, bf)
    for limit in ("0", "0.012"):
        r = subprocess.run([tool, "compare", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), limit, str(tmp_path / "d")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want, d_ab, d_ba = compare_meshes(av, af, bv, bf, max_dist=float(limit) or None, return_distances=True)
        assert np.array_equal(_bits(np.fromfile(str(tmp_path / "d.ab"), np.float32)), _bits(_cpu(d_ab)))
        assert np.array_equal(_bits(np.fromfile(str(tmp_path / "d.ba"), np.float32)), _bits(_cpu(d_ba)))
        got, flat = _parse(r.stdout.strip().splitlines()[-1]), _flat(want)
        assert sorted(got) == sorted(flat)
        for k in flat:
            assert (got[k] == flat[k]) if isinstance(flat[k], int) else _rel(got[k], flat[k], 1e-9), (k, got[k], flat[k])
        assert (got["a_to_b.within"] < got["a_to_b.n"]) == (limit != "0")
    bv[3, 1] = np.nan
    bf[5, 0] = 3
    mesh_io.write_ply(tmp_path / "nan.ply", bv, bv, bf)
    r = subprocess.run([tool, "compare", str(tmp_path / "a.ply"), str(tmp_path / "nan.ply"), "0", str(tmp_path / "d")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "non-finite" in r.stdout
