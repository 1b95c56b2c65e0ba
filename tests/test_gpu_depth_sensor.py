"""The depth sensor model on the GPU (sobfu_hip_depth_sensor, sobfu_hip_philox4x32_10; sobfu_amd/csrc/depth_sensor_kernels.hip, DESIGN.md
4.13) against the numpy restatement tests/depth_sensor_reference.py, bit for bit in depth and flags: the analytic scene on odd, pitched,
1 x 1 and multi-tile frames under four settings; what the counters depend on; the identity against the real mesh renderer;
mesh_render.render_mesh_depth(sensor=...); SobFusion.render_model_depth; the C++ twin; and the headless app's --sensor and
--render-trajectory.

Measured on the MI355X (profiles/LABBOOK.md, "Depth sensor model"): the app's trajectory line on the slab / box / sphere scene, three frames
5 mm and 1 degree apart: clean frames ate 7.26e-05 m, with --sensor kinect --sensor-seed 3 ate 1.15e-03 m.  Nothing asserts them."""
import os
import re
import subprocess

import numpy as np
import pytest

import depth_sensor_reference as DS
import icp_reference as IR
import mesh_ray_reference as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
SETTINGS = {"base": {}, "z_max": dict(z_max=0.85), "lateral": dict(lateral=2.5), "radius3": dict(edge_radius=3)}
SHAPES = [(23, 37), (1, 1), (17, 65)]


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _model(reference_model):
    from sobfu_amd import ops

    return ops.SensorModel(**reference_model.__dict__)


def _run(P, N, model, seed=0, frame=0, flags=True, **kw):
    from sobfu_amd import ops

    out = ops.depth_sensor(_gpu(P), _gpu(N), _model(model), seed, frame, flags=flags, **kw)
    if flags:
        return _cpu(out[0]).view(np.uint16), _cpu(out[1])
    return _cpu(out).view(np.uint16)


def _same(got, want, what):
    for name, g, w in zip(("depth", "flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s %s differs at %d pixels, first %s: got %r want %r" % (what, name, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.fixture(scope="module")
def scenes():
    return {shape: DS.scene(*shape) for shape in SHAPES}


def test_philox_against_the_reference():
    import torch

    from sobfu_amd import ops

    for counter, key, want in DS.PHILOX_KNOWN_ANSWERS:
        c = np.array([counter], np.uint32)
        got = _cpu(ops.philox4x32_10(_gpu(c.view(np.int32)), key)).view(np.uint32)
        assert tuple(int(x) for x in got[0]) == want
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    key = (0xDEADBEEF, 0x0BADF00D)
    assert np.array_equal(_cpu(ops.philox4x32_10(_gpu(c.view(np.int32)), key)).view(np.uint32), DS.philox4x32_10(c, key))
    assert ops.philox4x32_10(torch.empty((0, 4), dtype=torch.int32, device="cuda"), key).shape == (0, 4)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_reference(scenes, shape, setting):
    import torch

    from sobfu_amd import ops

    rows, cols = shape
    P, N = scenes[shape]
    model = DS.parity_setting(**SETTINGS[setting])
    seed, frame = 0x1234567887654321, 5
    d, f, info = DS.depth_sensor(P, N, model, seed, frame, details=True)
    if shape == (23, 37):  # conditions on the input, so that no branch goes untested
        counts = DS.flag_counts(f)
        print(setting, counts)
        if setting == "z_max":
            assert all(v > 0 for v in counts.values()), counts
        if setting == "base":
            assert all(v > 0 for k, v in counts.items() if k != "range"), counts
        if setting == "lateral":
            assert (np.abs(info["du"]) == 4).any() and (np.abs(info["dv"]) == 4).any()
            assert (info["u"] + info["du"] != info["su"]).any() and (info["v"] + info["dv"] != info["sv"]).any()  # clamped at a border
    _same(_run(P, N, model, seed, frame), (d, f), "dense")
    if shape == (23, 37):  # every image pitched 5 pixels wider, prefilled so that a write past the frame shows
        extra = 5
        wp, wn = torch.full((rows, cols + extra, 4), 77.0, device="cuda"), torch.full((rows, cols + extra, 4), 77.0, device="cuda")
        wp[:, :cols], wn[:, :cols] = _gpu(P), _gpu(N)
        wd = torch.full((rows, cols + extra), 77, dtype=torch.int16, device="cuda")
        wf = torch.full((rows, cols + extra), 77, dtype=torch.uint8, device="cuda")
        gd, gf = ops.depth_sensor(wp[:, :cols], wn[:, :cols], _model(model), seed, frame, depth=wd[:, :cols], flags=wf[:, :cols])
        _same((_cpu(gd).view(np.uint16), _cpu(gf)), (d, f), "pitched")
        assert np.all(_cpu(wd)[:, cols:] == 77) and np.all(_cpu(wf)[:, cols:] == 77)  # nothing written between the rows


def test_what_the_frame_depends_on(scenes):
    rows, cols = 23, 37
    P, N = scenes[rows, cols]
    model = DS.parity_setting()
    d, f = _run(P, N, model, 9, 1)
    again = _run(P, N, model, 9, 1)
    assert np.array_equal(d, again[0]) and np.array_equal(f, again[1])  # computed twice
    assert np.array_equal(_run(P, N, model, 9, 1, flags=False), d)  # d_flags NULL
    # the same pixels embedded at an offset in a larger frame: other counters, another image -- and the reference says which
    big_rows, big_cols, v0, u0 = 40, 60, 9, 14
    BP, BN = np.zeros((big_rows, big_cols, 4), np.float32), np.zeros((big_rows, big_cols, 4), np.float32)
    BP[v0:v0 + rows, u0:u0 + cols], BN[v0:v0 + rows, u0:u0 + cols] = P, N
    bd, bf = _run(BP, BN, model, 9, 1)
    _same((bd, bf), DS.depth_sensor(BP, BN, model, 9, 1), "embedded")
    assert (bd[v0:v0 + rows, u0:u0 + cols] != d).any() and (bf[v0:v0 + rows, u0:u0 + cols] != f).any()
    # frame and seed each change the image
    for other in (_run(P, N, model, 9, 2), _run(P, N, model, 10, 1), _run(P, N, model, 9 + (1 << 32), 1)):
        assert (other[0] != d).any() and (other[1] != f).any()
    # ideal(): rint(1000 z) of every hit, whatever the seed
    hit = N[..., 3] == 1
    di, fi = _run(P, N, DS.ideal(), 9, 1)
    assert np.array_equal(di[hit], np.rint(np.float32(1000) * P[..., 2][hit]).astype(np.uint16)) and not di[~hit].any()
    assert np.array_equal(fi, np.where(hit, DS.VALID, DS.MISS))


def test_bad_parameters_are_refused():
    from sobfu_amd import _lib, ops

    P, N = (_gpu(a) for a in DS.scene(4, 4))
    with pytest.raises(_lib.HipError):
        ops.depth_sensor(P, N, ops.SensorModel.kinect(edge_radius=4))
    with pytest.raises(ValueError):
        ops.depth_sensor(P, N[:3], ops.SensorModel.kinect())


@pytest.fixture(scope="module")
def icosphere():
    """the scene of tests/test_gpu_mesh_render.py: an icosphere of 320 faces (r = 0.1), its centre 0.6 m in front of the camera"""
    centre = np.array([0.05, -0.03, 0.1])
    v, f = MR.icosphere(0.1, 2, centre)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + np.sin(0.4) * K + (1 - np.cos(0.4)) * K @ K).astype(np.float32)
    t = (np.array([0.02, -0.01, 0.6]) - R.astype(np.float64) @ centre).astype(np.float32)
    return dict(v=v, f=f, pose=(R, t), intr=(60.0, 61.0, 18.2, 10.7), rows=23, cols=37)


def test_identity_against_the_renderer_and_render_mesh_depth(icosphere):
    from sobfu_amd import mesh_render, ops

    s = icosphere
    g = ops.TriangleGrid(_gpu(s["v"]), _gpu(s["f"]))
    r = g.render(s["intr"], s["rows"], s["cols"], pose=s["pose"], outputs=("depth", "points", "normals"))
    clean = _cpu(r["depth"]).view(np.uint16)
    assert 150 < (clean > 0).sum() < clean.size
    assert np.array_equal(_cpu(ops.depth_sensor(r["points"], r["normals"], ops.SensorModel.ideal())).view(np.uint16), clean)
    P, N = _cpu(r["points"]), _cpu(r["normals"])
    want, flags = DS.depth_sensor(P, N, DS.kinect(), 7, 2)
    assert (want != clean).any() and (flags == DS.VALID).sum() > 100
    got = mesh_render.render_mesh_depth(s["v"], s["f"], s["intr"], s["rows"], s["cols"], pose=s["pose"], grid=g, sensor=ops.SensorModel.kinect(), seed=7, frame=2)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(mesh_render.render_mesh_depth(s["v"], s["f"], s["intr"], s["rows"], s["cols"], pose=s["pose"], grid=g), clean)


def test_render_model_depth_is_the_model_through_raycast_and_the_sensor():
    from sobfu_amd import ops, synthetic as S
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    F = SobFusion(P)
    try:
        with pytest.raises(RuntimeError):
            F.render_model_depth()
        F(_gpu(S.render_sphere_depth((0.0, 0.0, 0.75), 0.1, P["intr"]).view(np.int16)))
        pts, nrm = ops.raycast(F.phi_global, P["vs"], P["trunc"], *F.vol2cam(), P["intr"], rows=480, cols=640)
        pts, nrm = _cpu(pts), _cpu(nrm)
        hit = nrm[..., 3] == 1
        assert hit.sum() > 1000
        ideal = _cpu(F.render_model_depth()).view(np.uint16)
        assert np.array_equal(ideal[hit], np.rint(np.float32(1000) * pts[..., 2][hit]).astype(np.uint16)) and not ideal[~hit].any()
        noisy = _cpu(F.render_model_depth(ops.SensorModel.kinect(), seed=11)).view(np.uint16)
        assert np.array_equal(noisy, DS.depth_sensor(pts, nrm, DS.kinect(), 11, 1)[0]) and (noisy != ideal).any()  # one frame fused: frame 1
    finally:
        F.close()


def test_the_cpp_twin_writes_the_same_bytes(tmp_path, scenes):
    from sobfu_amd import build_host

    tool = build_host.build_depth_sensor_tool()
    rows, cols = 17, 65
    P, N = scenes[rows, cols]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([rows, cols], np.int32).tobytes() + P.tobytes() + N.tobytes())
    for name, model, extra in (("kinect", DS.kinect(drop=0.02, z_min=0.0), ["drop=0.02", "z_min=0"]), ("ideal", DS.ideal(), []),
                               ("kinect", DS.kinect(edge_radius=2, lateral=1.5), ["edge_radius=2", "lateral=1.5"])):
        r = subprocess.run([tool, name, str(0x500000003), "4", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), *extra], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        d, f = DS.depth_sensor(P, N, model, 0x500000003, 4)
        assert (tmp_path / "out.bin").read_bytes() == d.tobytes() + f.tobytes(), (name, extra)
    bad = subprocess.run([tool, "kinect", "0", "0", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "drop=2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 3


# ---- the headless app --------------------------------------------------------------------------------------------------------------------
def _box(lo, hi):
    x, y, z = zip(lo, hi)
    v = np.array([[x[i], y[j], z[k], 1.0] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.float32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def _scene_mesh():
    """a static, asymmetric mesh that pins all six degrees of freedom -- the slab, box and sphere of tests/icp_reference.py, inside config
    1's volume -- in the frame of the meshes the app writes, (x, -y, -z)"""
    parts = [_box(*IR.SLAB), _box(*IR.BOX), MR.icosphere(IR.SPHERE[1], 3, IR.SPHERE[0])]
    v, f, base = [], [], 0
    for pv, pf in parts:
        v.append(np.asarray(pv, np.float32) * np.array([1, -1, -1, 1], np.float32))
        f.append(np.asarray(pf, np.int32) + base)
        base += len(pv)
    return np.concatenate(v), np.concatenate(f)


@pytest.fixture(scope="module")
def app_and_mesh(tmp_path_factory):
    from sobfu_amd import build_host, mesh_io

    d = tmp_path_factory.mktemp("sensor_app")
    v, f = _scene_mesh()
    n = np.zeros_like(v)
    mesh_io.write_ply(d / "m.ply", v, n, f)
    return build_host.build_app(), d


def _app(exe, *args):
    r = subprocess.run([exe, CONFIG1, "--no-stats", *map(str, args)], capture_output=True, text=True, timeout=600)
    return r


def _dump(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def test_app_neutral_options_change_nothing_and_kinect_does(app_and_mesh):
    from sobfu_amd import trajectory as T

    exe, d = app_and_mesh
    T.write_tum(d / "identity.txt", np.tile([0, 0, 0, 0, 0, 0, 1.0], (2, 1)))
    runs = {"clean": [], "neutral": ["--sensor", "ideal", "--render-trajectory", d / "identity.txt"], "kinect": ["--sensor", "kinect", "--sensor-seed", 3]}
    dumps = {}
    for name, extra in runs.items():
        os.mkdir(d / name)
        r = _app(exe, "--render-mesh", d / "m.ply", "--render-frames", 2, "--dump", d / name, *extra)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        dumps[name] = _dump(d / name)
        assert "trajectory:" not in r.stdout
    assert sorted(dumps["clean"]) == ["phi_global.npy", "phi_global_psi_inv.npy", "phi_n.npy", "phi_n_psi.npy", "psi.npy", "psi_inv.npy"]
    assert dumps["neutral"] == dumps["clean"]
    assert sorted(dumps["kinect"]) == sorted(dumps["clean"]) and dumps["kinect"]["phi_n.npy"] != dumps["clean"]["phi_n.npy"]
    assert dumps["kinect"]["phi_global.npy"] != dumps["clean"]["phi_global.npy"]
    for args, message in ((["--sensor", "kinect", "--synthetic", 2], "need --render-mesh"), (["--render-mesh", d / "m.ply", "--sensor", "lidar"], "kinect or ideal"),
                          (["--render-mesh", d / "m.ply", "--sensor", "kinect", "--sensor-set", "gain=2"], "name=value"),
                          (["--render-mesh", d / "m.ply", "--sensor", "kinect", "--sensor-set", "drop=2"], "outside its range"),
                          (["--render-mesh", d / "m.ply", "--render-frames", 3, "--render-trajectory", d / "identity.txt"], "2 poses for 3 frames"),
                          (["--voxelise-mesh", d / "m.ply", "--render-trajectory", d / "identity.txt"], "need --render-mesh")):
        r = _app(exe, *args)
        assert r.returncode == 2 and message in r.stdout, (args, r.stdout[-500:])


def test_app_tracks_a_rendered_trajectory(app_and_mesh):
    """--track --render-trajectory on a static mesh and three poses 5 mm and 1 degree apart: the trajectory line is printed and the poses
    file parses.  No threshold on the errors: DESIGN.md 4.13 and profiles/LABBOOK.md record what was measured."""
    from sobfu_amd import trajectory as T

    exe, d = app_and_mesh
    step = np.array([0.6, -0.5, 0.62]) * 0.005 / np.linalg.norm([0.6, -0.5, 0.62])  # 5 mm and 1 degree per frame
    poses = np.stack([IR.pose(IR.rot((0.2, 1.0, 0.1), 1.0 * k), step * k) for k in range(3)])
    T.write_tum(d / "path.txt", poses)
    line = re.compile(r"^trajectory: ate=(\S+) rpe_trans=(\S+) rpe_rot=(\S+)$", re.M)
    for name, extra in (("clean", []), ("kinect", ["--sensor", "kinect", "--sensor-seed", 3])):
        out = d / ("tracked_%s.txt" % name)
        r = _app(exe, "--render-mesh", d / "m.ply", "--render-frames", 3, "--track", "--render-trajectory", d / "path.txt", "--poses", out, *extra)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        found = line.findall(r.stdout)
        assert len(found) == 1, r.stdout[-2000:]
        print(name, "trajectory: ate=%s rpe_trans=%s rpe_rot=%s" % found[0])
        assert all(np.isfinite(float(x)) and float(x) >= 0 for x in found[0])
        frames, tracked = T.read_tum(out)
        assert list(frames) == [0, 1, 2] and tracked.shape == (3, 7)
        assert abs(T.ate(tracked, poses) - float(found[0][0])) < 1e-6  # the app's figure is that of the file it wrote
        print(name, "largest position error without alignment: %.6g m" % np.abs(T.to_matrices(tracked)[:, :3, 3] - poses[:, :3, 3]).max())
