"""The colour kernels (sobfu_amd/csrc/colour_kernels.hip) on the GPU: byte for byte against the numpy restatement tests/colour_reference.py
on random inputs, known answers of the frame driver (a uniform colour, the running average, the cap), the geometry left bit for bit as it
is, the headless app (--textured, --data with masks) and the colour following psi on the translating textured sphere."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import colour_reference as CR

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


def _random_case(rng, dims=(40, 36, 32)):
    X, Y, Z = dims
    tsdf = np.zeros((Z, Y, X, 2), np.float32)
    kind = rng.integers(0, 6, (Z, Y, X))
    tsdf[..., 0] = np.select([kind == 0, kind == 1, kind == 2], [0.0, -1.0, 1.0], rng.uniform(-1, 1, (Z, Y, X)).astype(np.float32))
    tsdf[..., 1] = rng.choice(np.float32([0.0, 1.0, 1.0, 2.5]), (Z, Y, X))
    zz, yy, xx = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in (Z, Y, X)), indexing="ij")
    psi = np.stack([xx, yy, zz, np.zeros_like(xx)], -1) + np.concatenate([rng.uniform(-0.7, 0.7, (Z, Y, X, 3)), np.zeros((Z, Y, X, 1))], -1)
    colour = rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8)
    colour[..., 3] = rng.choice(np.uint8([0, 1, 7, 127, 128, 200, 254, 255]), (Z, Y, X))
    return tsdf, psi.astype(np.float32), colour


@pytest.mark.parametrize("use_psi", [True, False])
@pytest.mark.parametrize("cap", [128, 255])
def test_integrate_colour_matches_restatement(use_psi, cap):
    from sobfu_amd import ops

    rng = np.random.default_rng(11 + cap + use_psi)
    tsdf, psi, colour = _random_case(rng)
    rows, cols = 60, 80
    image = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    vs = (0.01, 0.011, 0.012)
    a = np.radians(8.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    t = np.array([-0.2, -0.2, 0.35], np.float32)
    intr = (60.0, 62.0, 40.0, 30.0)
    want = CR.integrate_colour(image, tsdf, psi if use_psi else None, colour, vs, R, t, intr, cap)
    col = _gpu(colour)
    ops.integrate_colour(_gpu(image), _gpu(tsdf), _gpu(psi) if use_psi else None, col, vs, R, t, intr, cap)
    got = _cpu(col)
    changed = (want != colour).any(-1)
    assert changed.sum() > 1000 and (~changed).sum() > 1000  # both branches are exercised
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


def test_apply_and_sample_colour_match_restatement():
    import torch

    from sobfu_amd import ops

    rng = np.random.default_rng(5)
    _, psi, colour = _random_case(rng, (24, 20, 18))
    colour[rng.random(colour.shape[:3]) < 0.3, 3] = 0
    psi[rng.random(psi.shape[:3]) < 0.05, :3] = rng.uniform(-5, 30, (1, 3)).astype(np.float32)  # some points beyond the box: clamped
    col = _gpu(colour)
    out = torch.empty_like(col)
    ops.apply_colour(col, out, _gpu(psi))
    want = CR.apply_colour(colour, psi)
    assert np.array_equal(_cpu(out), want)
    assert (want[..., 3] == 0).any() and (want[..., 3] == 1).any()
    vs = (0.01, 0.01, 0.02)
    R = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float32)
    t = np.array([0.05, 0.2, 0.5], np.float32)
    pts = np.concatenate([rng.uniform(-0.3, 0.7, (30, 50, 3)), np.zeros((30, 50, 1))], -1).astype(np.float32)
    nrm = np.zeros((30, 50, 4), np.float32)
    nrm[..., 3] = rng.random((30, 50)) < 0.8
    got = _cpu(ops.sample_colour(col, vs, R, t, _gpu(pts), _gpu(nrm)))
    assert np.array_equal(got, CR.sample_colour(colour, vs, R, t, pts, nrm))
    flat = pts.reshape(-1, 4)[:1234].copy()
    got = _cpu(ops.sample_colour(col, vs, R, t, _gpu(flat), mc_vertices=True))
    assert got.shape == (1234, 4) and np.array_equal(got, CR.sample_colour(colour, vs, R, t, flat, mc_vertices=True))


def test_render_colour_matches_restatement():
    from sobfu_amd import ops

    rng = np.random.default_rng(7)
    rows, cols = 37, 70
    pts = np.concatenate([rng.uniform(-0.3, 0.3, (rows, cols, 2)), rng.uniform(0.4, 1.0, (rows, cols, 1)), np.zeros((rows, cols, 1))], -1)
    n = rng.normal(size=(rows, cols, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nrm = np.concatenate([n, (rng.random((rows, cols, 1)) < 0.8)], -1).astype(np.float32)
    colours = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    colours[rng.random((rows, cols)) < 0.3, 3] = 0
    pts = pts.astype(np.float32)
    for light in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1)):
        got = _cpu(ops.render_colour(_gpu(pts), _gpu(nrm), _gpu(colours), light))
        assert np.array_equal(got, CR.render_colour(pts, nrm, colours, light))
    grey = _cpu(ops.render_image(_gpu(pts), _gpu(nrm)))
    nocol = colours.copy()
    nocol[..., 3] = 0
    assert np.array_equal(_cpu(ops.render_colour(_gpu(pts), _gpu(nrm), _gpu(nocol))), grey)  # no colour: render_image's grey


# ---- the frame driver ---------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    P.update(kw)
    return P


def _sphere(P, x=0.0, textured=False, colour=None):
    from sobfu_amd import synthetic as S

    d = S.render_sphere_depth((x, 0.0, 0.75), 0.1, P["intr"])
    if textured:
        c = S.render_textured_sphere_colour((x, 0.0, 0.75), 0.1, P["intr"])
    elif colour is not None:
        c = np.zeros(d.shape + (4,), np.uint8)
        c[...] = colour
    else:
        c = None
    return _gpu(d), None if c is None else _gpu(c)


def _inside_image(P, margin=1e-3):
    """voxels whose centre projects into the 640 x 480 image (float64, with a margin against the kernel's float32 rounding)"""
    X, Y, Z = P["dims"]
    vs = P["vs"].astype(np.float64)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in (Z, Y, X)), indexing="ij")
    cam = [q * vs[i] + vs[i] / 2 + float(P["t"][i]) for i, q in enumerate((x, y, z))]
    fx, fy, cx, cy = P["intr"]
    u, v = fx * cam[0] / cam[2] + cx, fy * cam[1] / cam[2] + cy
    inside = (u >= margin) & (v >= margin) & (u < 640 - margin) & (v < 480 - margin) & (cam[2] > 0)
    border = (u >= -margin) & (v >= -margin) & (u < 640 + margin) & (v < 480 + margin) & ~inside
    return inside, border


def test_frame0_uniform_colour_known_answer():
    from sobfu_amd.fusion import SobFusion

    P = _params()
    f = SobFusion(P)
    d, c = _sphere(P, colour=(17, 99, 230, 5))
    f(d, c)
    col, g = _cpu(f.colour_global), _cpu(f.phi_global)
    inside, border = _inside_image(P)
    shell = CR.observed(g) & (np.abs(g[..., 0]) < 1)
    assert (shell & inside).sum() > 1000
    assert (col[shell & inside] == (17, 99, 230, 1)).all()
    assert not col[~shell | (~inside & ~border)].any()
    f.close()


def test_two_frames_average_and_cap():
    from sobfu_amd.fusion import SobFusion

    P = _params(start_frame=5)
    f = SobFusion(P)
    f(*_sphere(P, colour=(10, 100, 201, 255)))
    f(*_sphere(P, colour=(21, 50, 0, 255)))
    col = _cpu(f.colour_global)
    has = col[..., 3] > 0
    assert has.sum() > 1000 and (col[has] == (16, 75, 100, 2)).all()  # rint(15.5) = 16, rint(100.5) = 100: half to even
    f.close()
    P = _params(start_frame=9, max_weight=3.0)
    f = SobFusion(P)
    for _ in range(5):
        f(*_sphere(P, colour=(40, 40, 40, 255)))
    col = _cpu(f.colour_global)
    assert col[..., 3].max() == 3 and (col[col[..., 3] > 0, :3] == 40).all()
    f.close()


def test_colour_leaves_geometry_bit_identical():
    from sobfu_amd.fusion import SobFusion

    P = _params()
    runs = []
    for textured in (False, True):
        f = SobFusion(P)
        for n in range(3):
            f(*_sphere(P, 0.005 * n, textured=textured))
        runs.append({k: _cpu(getattr(f, k)).copy() for k in ("phi_global", "phi_global_psi_inv", "phi_n", "phi_n_psi", "psi", "psi_inv")})
        assert (f.colour_global is None) == (not textured)
        if textured:
            img = _cpu(f.render("phi_global"))
            grey = _cpu(f.render("phi_global", colour=False))
            hit = grey[..., 3] > 0
            assert hit.sum() > 1000 and (img[hit] != grey[hit]).any() and np.array_equal(img[~hit], grey[~hit])
            assert _cpu(f.render("phi_global_psi_inv"))[..., 3].any()
        f.close()
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)), k


def test_colour_follows_psi():
    """The canonical mesh's vertex colours after a few solved frames of the translating textured sphere, compared with the frame-0 texture
    at the vertices: fused through psi they must be closer to it than fused at identity (psi = NULL)."""
    from sobfu_amd import ops, synthetic as S
    from sobfu_amd.fusion import SobFusion

    P = _params()
    f = SobFusion(P)
    identity = ops.new_colour_volume(P["dims"])
    cap = ops.colour_weight_cap(P["max_weight"])
    for n in range(5):
        d, c = _sphere(P, 0.005 * n, textured=True)
        f(d, c)
        tsdf = f.phi_global if n == 0 else f.phi_n_psi  # the volume SobFusion fused the colour through in this frame
        ops.integrate_colour(c, tsdf, None, identity, P["vs"], P["R"], P["t"], P["intr"], cap)
    errs = []
    for col in (f.colour_global, identity):
        v, _, vc = ops.marching_cubes(f.phi_global, P["size"], P["R"], P["t"], colour=col)
        v, vc = _cpu(v), _cpu(vc)
        p = np.stack([v[:, 0], -v[:, 1], -v[:, 2]], -1).astype(np.float64)  # the camera frame of frame 0
        want = S.texture_bgra(*S.sphere_directions(p[:, 0], p[:, 1], (0.0, 0.0, 0.75), 0.1))
        ok = (vc[:, 3] > 0) & (p[:, 2] < 0.75)  # coloured vertices on the camera's side
        assert ok.sum() > 1000
        errs.append((float(np.abs(vc[ok, :3].astype(float) - want[ok, :3]).mean()), int(ok.sum())))
    f.close()
    msg = "mean |colour - frame-0 texture| per channel: through psi %.3f (%d vertices), at identity %.3f (%d vertices)" % (*errs[0], *errs[1])
    print(msg)
    assert errs[0][0] < errs[1][0], msg


# ---- the headless app ------------------------------------------------------------------------------------------------------------------
def _app(*args):
    from sobfu_amd import build, build_host

    build.build_hip()
    exe = build_host.build_app()
    r = subprocess.run([exe, CONFIG1, "--no-stats", *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def _read_png_rgb(path):
    data = open(path, "rb").read()
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()  # the writer uses filter 0 only
    return raw[:, 1:].reshape(h, w, 3)


def test_app_textured_meshes_screenshots_dump(tmp_path):
    mesh, shots, dump = tmp_path / "mesh", tmp_path / "shots", tmp_path / "dump"
    for p in (mesh, shots, dump):
        p.mkdir()
    _app("--synthetic", "4", "--textured", "--mesh", str(mesh), "--screenshots", str(shots), "--dump", str(dump))
    for name in ("phi_global_3", "phi_global_psi_inv_3"):
        text = (mesh / (name + ".vtk")).read_text()
        npts = int(text.split("POINTS ")[1].split()[0])
        assert "POINT_DATA %d\nCOLOR_SCALARS rgb 3\n" % npts in text, name
        rgb = np.array([[float(x) for x in line.split()] for line in text.split("COLOR_SCALARS rgb 3\n")[1].strip().split("\n")])
        assert rgb.shape == (npts, 3) and rgb.std(0).min() > 0.05  # textured, not uniform
    assert "POINT_DATA" not in (mesh / "phi_n_3.vtk").read_text() and "POINT_DATA" not in (mesh / "phi_n_psi_3.vtk").read_text()
    img = _read_png_rgb(shots / "000003.png")
    for panel in (img[:, :640], img[:, 640:]):
        lit = panel.max(-1) > 0
        assert lit.sum() > 1000
        assert (panel[lit].max(-1) != panel[lit].min(-1)).mean() > 0.5  # coloured, not grey
    col = np.load(dump / "colour_global.npy")
    assert col.shape == (64, 64, 64, 4) and col.dtype == np.uint8 and (col[..., 3] > 0).sum() > 1000
    plain = tmp_path / "plain"
    plain.mkdir()
    _app("--synthetic", "2", "--dump", str(plain))
    assert not (plain / "colour_global.npy").exists()


def _write_pgm16(path, d):
    h, w = d.shape
    path.write_bytes(b"P5\n%d %d\n65535\n" % (w, h) + d.astype(">u2").tobytes())


def _write_ppm(path, bgra):
    h, w = bgra.shape[:2]
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(bgra[..., 2::-1]).tobytes())


def _write_png_grey(path, m):
    h, w = m.shape
    raw = b"".join(b"\0" + m[y].astype(np.uint8).tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) +
                     chunk(b"IEND", b""))


def test_app_data_dir_with_masks(tmp_path):
    from sobfu_amd import synthetic as S

    P = _params()
    a, b = tmp_path / "a", tmp_path / "b"
    for root in (a, b):
        for sub in ("depth", "color"):
            (root / sub).mkdir(parents=True)
    (a / "omask").mkdir()
    for n in range(3):
        centre = (0.005 * n, 0.0, 0.75)
        d = S.render_sphere_depth(centre, 0.1, P["intr"])
        c = S.render_textured_sphere_colour(centre, 0.1, P["intr"])
        m = np.zeros(d.shape, np.uint8)
        m[:, 300:] = 200  # the left of the sphere is masked out
        _write_pgm16(a / "depth" / ("%03d.pgm" % n), d)
        _write_ppm(a / "color" / ("%03d.ppm" % n), c)
        _write_png_grey(a / "omask" / ("%03d.png" % n), m)
        _write_pgm16(b / "depth" / ("%03d.pgm" % n), np.where(m == 0, 0, d))
        _write_ppm(b / "color" / ("%03d.ppm" % n), c)
    outs = []
    for root in (a, b):
        dump = root / "dump"
        dump.mkdir()
        _app("--data", str(root), "--dump", str(dump))
        outs.append({f: np.load(dump / f) for f in sorted(os.listdir(dump))})
    assert sorted(outs[0]) == sorted(outs[1]) and "colour_global.npy" in outs[0]
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    (a / "omask" / "002.png").unlink()  # a count mismatch is an error
    from sobfu_amd import build_host

    r = subprocess.run([build_host.build_app(), CONFIG1, "--no-stats", "--data", str(a)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "masks" in r.stdout
