"""The canonical mesh carried to live on the GPU (sobfu_amd/csrc/warp_points_kernels.hip): the two kernels against the numpy restatement
tests/mesh_warp_reference.py on random inputs (positions and TSDF samples bit for bit), in-place and repeated calls, the frame driver on the
translating sphere (the warped canonical mesh fits every solved frame better than the unwarped one), the solve left bit for bit as it is,
the headless app's --warp-mesh / --track-mesh / --fit-stats and the C++ shells against the Python front end."""
import os
import re
import subprocess

import numpy as np
import pytest

import mc_indexed_reference as MI
import mesh_warp_reference as MW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _random_case(rng, dims=(40, 36, 32), n=6000):
    """psi = identity + up to 0.7 voxel, some voxels thrown far outside the box (as test_gpu_colour._random_case and its callers do); a TSDF
    volume with a fifth of its weights 0; points in and around the box under a rotated pose; unit normals, some of them zero"""
    X, Y, Z = dims
    zz, yy, xx = np.meshgrid(*(np.arange(k, dtype=np.float32) for k in (Z, Y, X)), indexing="ij")
    psi = np.stack([xx, yy, zz, np.zeros_like(xx)], -1) + np.concatenate([rng.uniform(-0.7, 0.7, (Z, Y, X, 3)), np.zeros((Z, Y, X, 1))], -1)
    psi = psi.astype(np.float32)
    far = rng.random((Z, Y, X)) < 0.05
    psi[far, :3] = rng.uniform(-5, 45, (int(far.sum()), 3)).astype(np.float32)
    vol = np.stack([rng.uniform(-1, 1, (Z, Y, X)), rng.choice([0.0, 1.0, 1.0, 2.5, 7.0], (Z, Y, X))], -1).astype(np.float32)
    vs = (0.01, 0.011, 0.012)
    a = np.radians(8.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    t = np.array([-0.2, -0.2, 0.35], np.float32)
    g = rng.uniform(-3.0, np.array(dims) + 2.0, (n, 3))  # grid positions: most inside, some beyond every face
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = ((g + 0.5) * np.array(vs)) @ R.astype(np.float64).T + t
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.concatenate([nrm, np.ones((n, 1))], -1).astype(np.float32)
    nrm[::53, :3] = 0
    return psi, vol, vs, R, t, pts, nrm


@pytest.mark.parametrize("mc", [False, True])
def test_kernels_match_restatement(mc):
    from sobfu_amd import ops

    rng = np.random.default_rng(21 + mc)
    psi, vol, vs, R, t, pts, nrm = _random_case(rng)
    if mc:
        pts[:, 1:3] *= -1
    want_p, want_n = MW.warp_points(psi, vs, R, t, pts, nrm, mc_vertices=mc)
    dpsi, dp, dn = _gpu(psi), _gpu(pts), _gpu(nrm)
    got_p, got_n = ops.warp_points(dpsi, vs, R, t, dp, dn, mc_vertices=mc)
    got_p, got_n = _cpu(got_p), _cpu(got_n)
    moved = np.abs(want_p[:, :3] - pts[:, :3]).max(1)
    print("mc_vertices=%d: %d points, max displacement %.4g m, positions differing in bits: %d, max normal difference %.3g"
          % (mc, len(pts), moved.max(), int((_bits(got_p) != _bits(want_p)).any(1).sum()), np.abs(got_n - want_n).max()))
    assert (moved > 1e-4).mean() > 0.9
    assert np.array_equal(_bits(got_p), _bits(want_p))
    assert np.abs(got_n - want_n).max() <= 2e-6
    zero = ~nrm[:, :3].any(1)
    assert zero.sum() > 50 and np.array_equal(got_n[zero], np.tile(np.float32([0, 0, 0, 1]), (int(zero.sum()), 1)))
    ln = np.linalg.norm(got_n[~zero, :3].astype(np.float64), axis=1)
    assert np.abs(ln - 1).max() < 1e-5 and np.all(got_n[:, 3] == 1)
    # without normals: the same positions
    only_p = _cpu(ops.warp_points(dpsi, vs, R, t, dp, mc_vertices=mc))
    assert np.array_equal(_bits(only_p), _bits(want_p))
    # sample_tsdf: bit for bit, NaNs in the same places
    want_s = MW.sample_tsdf(vol, vs, R, t, pts, mc_vertices=mc)
    got_s = _cpu(ops.sample_tsdf(_gpu(vol), vs, R, t, dp, mc_vertices=mc))
    assert np.isnan(want_s).sum() > 100 and (~np.isnan(want_s)).sum() > 100
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s))
    ok = ~np.isnan(want_s)
    assert np.array_equal(_bits(got_s[ok]), _bits(want_s[ok]))


def test_in_place_repeat_and_empty():
    import torch

    from sobfu_amd import ops

    rng = np.random.default_rng(31)
    psi, vol, vs, R, t, pts, nrm = _random_case(rng, n=5003)
    dpsi, dp, dn = _gpu(psi), _gpu(pts), _gpu(nrm)
    p1, n1 = ops.warp_points(dpsi, vs, R, t, dp, dn, mc_vertices=True)
    p2, n2 = ops.warp_points(dpsi, vs, R, t, dp, dn, mc_vertices=True)
    assert np.array_equal(_bits(_cpu(p1)), _bits(_cpu(p2))) and np.array_equal(_bits(_cpu(n1)), _bits(_cpu(n2)))
    assert np.array_equal(_cpu(dp), pts) and np.array_equal(_cpu(dn), nrm)  # the inputs are left alone
    ip, inn = dp.clone(), dn.clone()
    rp, rn = ops.warp_points(dpsi, vs, R, t, ip, inn, mc_vertices=True, out=(ip, inn))
    assert rp is ip and rn is inn
    assert np.array_equal(_bits(_cpu(ip)), _bits(_cpu(p1))) and np.array_equal(_bits(_cpu(inn)), _bits(_cpu(n1)))
    ip = dp.clone()
    ops.warp_points(dpsi, vs, R, t, ip, mc_vertices=True, out=ip)
    assert np.array_equal(_bits(_cpu(ip)), _bits(_cpu(p1)))
    s1, s2 = ops.sample_tsdf(_gpu(vol), vs, R, t, dp), ops.sample_tsdf(_gpu(vol), vs, R, t, dp)
    assert np.array_equal(_bits(_cpu(s1)), _bits(_cpu(s2)))
    e = torch.zeros((0, 4), dtype=torch.float32, device="cuda")
    assert ops.warp_points(dpsi, vs, R, t, e).shape == (0, 4)
    ep, en = ops.warp_points(dpsi, vs, R, t, e, e.clone())
    assert ep.shape == (0, 4) and en.shape == (0, 4)
    assert ops.sample_tsdf(_gpu(vol), vs, R, t, e).shape == (0,)
    with pytest.raises(ValueError):
        ops.warp_points(dpsi, vs, R, t, dp, dn[:10])


# ---- the frame driver -------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    P.update(kw)
    return P


def _sphere(P, x=0.0):
    from sobfu_amd import synthetic as S

    return _gpu(S.render_sphere_depth((x, 0.0, 0.75), 0.1, P["intr"]))


STATE = ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi", "psi", "psi_inv")


def test_warped_canonical_mesh_follows_the_frames():
    """config 1's translating sphere (5 mm = 0.64 voxel per frame, 10 iterations per frame), v = the indexed mesh of phi_global after each
    frame.  Measured on the MI355X (rms fit in mm, valid samples of V welded vertices):
      frame 1: 2.3508 (648 of 1000) unwarped -> 1.2981 (712) through psi;  frame 2: 5.4020 (643 of 1070) -> 2.6597 (793)
      frame 3: 7.4693 (582 of 1098) -> 3.5879 (743);  frame 4: 9.3586 (553 of 1147) -> 4.3174 (729), x 0.461 (bar: 0.7)
      frame 4: mean |phi_global o psi_inv| at the vertices 3.6787 -> 0.9565 mm"""
    from sobfu_amd import ops
    from sobfu_amd.fusion import SobFusion

    P = _params()
    runs = []
    for probe in (True, False):
        f = SobFusion(P)
        for n in range(5):
            f(_sphere(P, 0.005 * n))
            if not probe:
                continue
            v, nr, faces = ops.marching_cubes_indexed(f.phi_global, P["size"], P["R"], P["t"])
            if n == 0:
                w = f.warp_to_live(v)
                assert w is v  # nothing is solved yet: the input comes back
                continue
            w, wn = f.warp_to_live(v, nr)
            assert w.shape == v.shape and wn.shape == nr.shape and w.data_ptr() != v.data_ptr()
            before, after = f.fit(v), f.fit(w)
            V = v.shape[0]
            print("frame %d: rms fit %.4f mm (%d of %d valid) unwarped -> %.4f mm (%d valid) through psi, x %.3f; mean |d| %.4f -> %.4f, max %.4f -> %.4f"
                  % (n, 1e3 * before["rms"], before["valid"], V, 1e3 * after["rms"], after["valid"], after["rms"] / before["rms"],
                     1e3 * before["mean_abs"], 1e3 * after["mean_abs"], 1e3 * before["max"], 1e3 * after["max"]))
            assert after["rms"] < before["rms"], n
            assert before["valid"] >= 0.4 * V and after["valid"] >= 0.4 * V, n
            ln = np.linalg.norm(_cpu(wn)[:, :3].astype(np.float64), axis=1)
            assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0))
            if n == 4:
                assert after["rms"] <= 0.7 * before["rms"]
                m = []
                for pts in (v, w):
                    d = _cpu(ops.sample_tsdf(f.phi_global_psi_inv, P["vs"], P["R"], P["t"], pts, mc_vertices=True)).astype(np.float64)
                    m.append(float(np.nanmean(np.abs(d)) * float(P["trunc"])))
                print("frame 4: mean |phi_global o psi_inv| at the vertices %.4f mm unwarped -> %.4f mm through psi" % (1e3 * m[0], 1e3 * m[1]))
                assert m[1] < m[0]
        runs.append({k: _cpu(getattr(f, k)).copy() for k in STATE})
        f.close()
    for k in STATE:  # warp_to_live / fit between the frames change nothing the solve sees
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k


# ---- the headless app -------------------------------------------------------------------------------------------------------------------
def _app(*args):
    from sobfu_amd import build, build_host

    build.build_hip()
    exe = build_host.build_app()
    r = subprocess.run([exe, CONFIG1, "--no-stats", *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


FIT = re.compile(r"^fit (\d+): (\d+) vertices, (\d+) valid, mean \|d\| ([0-9.]+) mm, rms ([0-9.]+) mm, max ([0-9.]+) mm \(unwarped rms ([0-9.]+) mm\)$", re.M)


def test_app_warp_mesh_track_mesh_fit_stats(tmp_path):
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir()
    off.mkdir()
    out = _app("--synthetic", "5", "--textured", "--mesh", str(on), "--mesh-format", "ply", "--warp-mesh", "--track-mesh", "1", "--fit-stats")
    solved = (1, 2, 3, 4)
    for n in solved:
        header, verts, faces = MI.read_ply(str(on / ("phi_global_warped_%d.ply" % n)))
        _, cverts, cfaces = MI.read_ply(str(on / ("phi_global_%d.ply" % n)))
        assert "property uchar red" in header  # the canonical colours travel with the vertices
        assert len(verts) == len(cverts) and np.array_equal(faces, cfaces)
        assert all(np.array_equal(verts[c], cverts[c]) for c in ("red", "green", "blue"))
        assert np.abs(verts["x"] - cverts["x"]).max() > 1e-4  # moved
    assert not (on / "phi_global_warped_0.ply").exists() and not (on / "tracked_0.ply").exists()
    tracked = [MI.read_ply(str(on / ("tracked_%d.ply" % n))) for n in solved]
    raw = [(on / ("tracked_%d.ply" % n)).read_bytes() for n in solved]
    nv, nf = len(tracked[0][1]), len(tracked[0][2])
    for (header, verts, faces), data in zip(tracked, raw):
        assert header == tracked[0][0] and len(verts) == nv
        assert data[-13 * nf:] == raw[0][-13 * nf:]  # the face block, byte for byte
    for a, b in zip(tracked, tracked[1:]):
        assert np.abs(a[1]["x"] - b[1]["x"]).max() > 1e-4  # positions move from frame to frame
    fits = FIT.findall(out)
    print("\n".join(l for l in out.splitlines() if l.startswith("fit ")))
    assert [int(m[0]) for m in fits] == list(solved)
    for m in fits:
        assert int(m[2]) > 0 and float(m[4]) < float(m[6]), m
    plain = _app("--synthetic", "5", "--textured", "--mesh", str(off), "--mesh-format", "ply")
    assert not list(off.glob("*_warped_*")) and not list(off.glob("tracked_*")) and not FIT.search(plain) and "fit " not in plain
    assert sorted(p.name for p in off.iterdir()) == sorted(p.name for p in on.iterdir() if "_warped_" not in p.name and not p.name.startswith("tracked_"))
    for p in off.iterdir():  # the files the app wrote before are the same bytes
        assert p.read_bytes() == (on / p.name).read_bytes(), p.name
    from sobfu_amd import build_host

    r = subprocess.run([build_host.build_app(), CONFIG1, "--synthetic", "2", "--warp-mesh"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mesh DIR" in r.stdout


# ---- the C++ shells -----------------------------------------------------------------------------------------------------------------------
def test_cpp_shells_match_the_python_front_end(tmp_path):
    from sobfu_amd import build, build_host, ops

    build.build_hip()
    tool = build_host.build_mesh_warp_tool()
    r = subprocess.run([tool, CONFIG1, "4", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    d = {k: np.load(tmp_path / (k + ".npy")) for k in ("psi", "phi_n", "canonical_vertices", "canonical_normals", "warped_vertices", "warped_normals",
                                                      "kept_vertices", "kept_normals", "faces", "fit_samples")}
    P = _params()
    v, n = d["canonical_vertices"], d["canonical_normals"]
    assert len(v) > 1000 and d["faces"].shape[1] == 3 and d["faces"].max() == len(v) - 1
    wp, wn = ops.warp_points(_gpu(d["psi"]), P["vs"], P["R"], P["t"], _gpu(v), _gpu(n), mc_vertices=True)
    wp, wn = _cpu(wp), _cpu(wn)
    assert np.abs(wp - v).max() > 1e-4
    for k in ("warped", "kept"):  # the device path and the upload path
        assert np.array_equal(_bits(d[k + "_vertices"]), _bits(wp)), k
        assert np.array_equal(_bits(d[k + "_normals"]), _bits(wn)), k
    s = _cpu(ops.sample_tsdf(_gpu(d["phi_n"]), P["vs"], P["R"], P["t"], _gpu(wp), mc_vertices=True))
    assert np.array_equal(np.isnan(s), np.isnan(d["fit_samples"]))
    ok = ~np.isnan(s)
    assert np.array_equal(_bits(s[ok]), _bits(d["fit_samples"][ok]))
    fit = [float(x) for x in re.search(r"^fit (.*)$", r.stdout, re.M).group(1).split()]
    a = np.abs(s[ok].astype(np.float64)) * float(np.float32(P["trunc"]))
    assert fit[0] == len(v) and fit[1] == ok.sum()
    assert np.allclose(fit[2:], [a.mean(), np.sqrt((a * a).mean()), a.max()], rtol=1e-6)
