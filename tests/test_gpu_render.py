"""The raycaster and shaders (sobfu_amd/csrc/render_kernels.hip) on the GPU: against closed forms (init_sphere / init_box volumes, axis-aligned
and rotated cameras), against the numpy restatement tests/render_reference.py, against the depth frame a volume was integrated from, at the
edges (cleared volume, axis-parallel rays, a camera inside the volume, a 1 x 1 image), through the C++ shells (--screenshots of the headless
app) and the Python front end (SobFusion.render)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import render_reference as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 240, 320
INTR = (570.342 / 2, 570.342 / 2, 160.0, 120.0)


def rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)


def look_at(R, target_vol, dist):
    """t of vol2cam = (R, t) for a camera whose optical axis passes through target_vol (volume metres) at depth `dist`"""
    cam = np.asarray(target_vol, np.float64) - R.T.astype(np.float64) @ np.array([0.0, 0.0, dist])
    return (-(R.astype(np.float64) @ cam)).astype(np.float32)


def rays(intr, rows, cols):
    fx, fy, cx, cy = intr
    u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)


def sphere_hits(R, t, centre_vol, r, intr, rows, cols):
    """float64: depth (0 = miss), unit normal, ray-to-centre distance, in the camera frame"""
    C = R.astype(np.float64) @ np.asarray(centre_vol, np.float64) + t.astype(np.float64)
    d = rays(intr, rows, cols)
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ C), C @ C - r * r
    disc = b * b - 4 * a * cc
    z = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    n = (z[..., None] * d - C) / r
    dist = np.linalg.norm(np.cross(d, C), axis=-1) / np.linalg.norm(d, axis=-1)
    return z, n, dist


def box_hits(R, t, centre_vol, half, intr, rows, cols):
    """float64 slab test of the box centre +- half (volume metres) -> depth (0 = miss), normal (camera frame), hit point (box frame)"""
    Rd = R.astype(np.float64)
    o = -Rd.T @ t.astype(np.float64) - np.asarray(centre_vol, np.float64)  # camera centre relative to the box centre
    d = rays(intr, rows, cols) @ Rd  # rows of R^T d
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-half - o) / d, (half - o) / d
    tn, tf = np.nanmax(np.minimum(t0, t1), -1), np.nanmin(np.maximum(t0, t1), -1)
    hit = (tn <= tf) & (tn > 0)
    z = np.where(hit, tn, 0.0)
    axis = np.nanargmax(np.minimum(t0, t1), -1)
    p = o + z[..., None] * d
    nb = np.zeros(p.shape)
    np.put_along_axis(nb, axis[..., None], np.sign(np.take_along_axis(p, axis[..., None], -1)), -1)
    return z, nb @ Rd.T, p


def gpu_volume(dims, fill):
    from sobfu_amd import ops

    vol = ops.new_volume(dims)
    fill(vol)
    return vol


def raycast_both(vol, vs, trunc, R, t, intr=INTR, rows=ROWS, cols=COLS, step_factor=0.75):
    """GPU (points, normals) and the restatement's on the same volume"""
    import torch

    from sobfu_amd import ops

    p, n = ops.raycast(vol, vs, trunc, R, t, intr, rows=rows, cols=cols, step_factor=step_factor)
    torch.cuda.synchronize()
    rp, rn = RR.raycast(vol.cpu().numpy(), vs, trunc, R, t, intr, rows, cols, step_factor=step_factor)
    return p.cpu().numpy(), n.cpu().numpy(), rp, rn


def assert_matches_restatement(p, n, rp, rn, vs):
    """exact: the same hit mask, the same bits in every point and normal (misses included), the same bytes from both shaders"""
    assert np.array_equal(n[..., 3] != 0, rn[..., 3] != 0)
    assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)) and np.array_equal(n.view(np.uint32), rn.view(np.uint32))
    import torch

    from sobfu_amd import ops

    img = ops.render_image(torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()).cpu().numpy()
    col = ops.render_normals(torch.from_numpy(n).cuda()).cpu().numpy()
    assert np.array_equal(img, RR.render_image(p, n))
    assert np.array_equal(col, RR.render_normals(n))


SPHERES = [((64, 64, 64), (0.5 / 64,) * 3), ((96, 80, 72), (0.006, 0.007, 0.0075))]


@pytest.mark.parametrize("deg", [0.0, 30.0])
@pytest.mark.parametrize("dims,vs", SPHERES)
def test_sphere_closed_form_and_restatement(dims, vs, deg):
    from sobfu_amd import ops

    vs = np.asarray(vs, np.float32)
    size = np.asarray(dims) * vs.astype(np.float64)
    centre, r = size / 2, 0.3 * float(size.min())
    trunc = np.float32(5) * vs.min()
    vol = gpu_volume(dims, lambda v: ops.init_sphere(v, vs, trunc, trunc, centre, r))  # eta = trunc: every corner observed
    R = rot_y(deg)
    t = look_at(R, centre, 0.75)
    p, n, rp, rn = raycast_both(vol, vs, trunc, R, t)
    z, nz, dist = sphere_hits(R, t, np.float32(centre).astype(np.float64), float(np.float32(r)), INTR, ROWS, COLS)
    hit, vox = n[..., 3] != 0, float(vs.max())
    inner = dist < r - 2 * vox
    assert inner.sum() > 2000
    far = np.abs(dist - r) > vox
    assert np.array_equal(hit[far], (dist < r)[far])
    assert np.abs(p[..., 2] - z)[inner].max() < 0.05 * float(vs.min())
    ang = np.degrees(np.arccos(np.clip((n[..., :3].astype(np.float64) * nz).sum(-1), -1, 1)))
    assert ang[inner].max() < 2.0
    assert_matches_restatement(p, n, rp, rn, vs)


@pytest.mark.parametrize("deg", [0.0, 30.0])
def test_box_closed_form_and_restatement(deg):
    from sobfu_amd import ops

    dims, vs = (64, 64, 64), np.full(3, 0.5 / 64, np.float32)
    half = np.array([0.1, 0.08, 0.12])
    trunc = np.float32(5) * vs[0]
    vol = gpu_volume(dims, lambda v: ops.init_box(v, vs, trunc, half))  # init_box centres the box in the volume
    centre = np.asarray(dims) * vs.astype(np.float64) / 2
    R = rot_y(deg)
    t = look_at(R, centre, 0.7)
    p, n, rp, rn = raycast_both(vol, vs, trunc, R, t)
    hf = np.float32(half).astype(np.float64)
    z, nb, pb = box_hits(R, t, centre, hf, INTR, ROWS, COLS)
    zg, _, _ = box_hits(R, t, centre, hf + float(vs[0]), INTR, ROWS, COLS)
    zs, _, _ = box_hits(R, t, centre, hf - float(vs[0]), INTR, ROWS, COLS)
    hit, vox = n[..., 3] != 0, float(vs[0])
    sure = (zg > 0) == (zs > 0)  # rays that pass further than a voxel from the silhouette
    assert np.array_equal(hit[sure], (z > 0)[sure])
    # faces, >= 2 voxels from every edge: at most one coordinate of the hit point is near its half extent
    off_edge = (z > 0) & ((np.abs(pb) <= hf - 2 * vox).sum(-1) >= 2)
    assert off_edge.sum() > 2000
    assert np.abs(p[..., 2] - z)[off_edge].max() < 0.05 * vox
    ang = np.degrees(np.arccos(np.clip((n[..., :3].astype(np.float64) * nb).sum(-1), -1, 1)))
    assert ang[off_edge].max() < 2.0
    assert_matches_restatement(p, n, rp, rn, vs)


def test_integrated_frame_matches_its_depth():
    """integrate(render_sphere_depth) into a cleared volume, raycast from the same camera: off the silhouette the depth is the input's
    within a voxel, and the GPU agrees with the restatement on the hit mask"""
    import torch

    from sobfu_amd import ops, params, synthetic

    P = params.read_ini(os.path.join(ROOT, "params", "config1_sphere_64.ini"))
    depth = synthetic.render_sphere_depth((0.0, 0.0, 0.75), 0.1, INTR, ROWS, COLS)
    dists = ops.compute_dists(torch.from_numpy(depth.astype(np.int16)).cuda(), INTR)
    vol = ops.new_volume(P["dims"])
    ops.clear_volume(vol)
    ops.integrate_depth(dists, vol, P["vs"], P["trunc"], P["eta"], P["R"], P["t"], INTR)
    p, n, rp, rn = raycast_both(vol, P["vs"], P["trunc"], P["R"], P["t"])
    _, _, dist = sphere_hits(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), (0.0, 0.0, 0.75), 0.1, INTR, ROWS, COLS)
    vox = float(P["vs"][0])
    hit = n[..., 3] != 0
    inner = dist < 0.1 - 3 * vox  # off the silhouette: 3 voxels (at 2, the sloped rim reaches 1.07 voxels in the restatement too)
    assert hit[inner].mean() > 0.9 and not hit[dist > 0.1 + 2 * vox].any()
    assert (np.abs(p[..., 2] - depth / 1000.0)[inner & hit]).max() <= vox
    assert_matches_restatement(p, n, rp, rn, P["vs"])


def test_edges():
    import torch

    from sobfu_amd import ops

    dims, vs = (48, 40, 56), np.full(3, 0.01, np.float32)
    trunc = np.float32(0.05)
    # an all-cleared volume: no hit, all outputs zero
    vol = gpu_volume(dims, ops.clear_volume)
    p, n = ops.raycast(vol, vs, trunc, np.eye(3), look_at(np.eye(3, dtype=np.float32), (0.24, 0.2, 0.28), 0.6), INTR, rows=ROWS, cols=COLS)
    assert not p.any().item() and not n.any().item()
    centre = np.array([0.24, 0.2, 0.28])
    vol = gpu_volume(dims, lambda v: ops.init_sphere(v, vs, trunc, trunc, centre, 0.1))
    # rays parallel to the axes: the centre pixel of an axis-aligned camera, and a camera looking along -x (rotation of 90 deg about y)
    for R in (np.eye(3, dtype=np.float32), np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)):  # the second: 90 deg about y
        t = look_at(R, centre, 0.5)
        p, n, rp, rn = raycast_both(vol, vs, trunc, R, t)
        c = (int(INTR[3]), int(INTR[2]))
        assert n[c][3] == 1 and abs(p[c][2] - 0.4) < 0.05 * 0.01 and n[c][2] < -0.999
        assert_matches_restatement(p, n, rp, rn, vs)
    # a camera inside the volume, 0.15 m in front of the sphere centre
    R = np.eye(3, dtype=np.float32)
    t = look_at(R, centre, 0.15)
    p, n, rp, rn = raycast_both(vol, vs, trunc, R, t)
    c = (int(INTR[3]), int(INTR[2]))
    assert n[c][3] == 1 and abs(p[c][2] - 0.05) < 0.05 * 0.01
    assert_matches_restatement(p, n, rp, rn, vs)
    # a 1 x 1 image (the pixel sees the centre through its principal point)
    p, n = ops.raycast(vol, vs, trunc, R, look_at(R, centre, 0.5), (500.0, 500.0, 0.0, 0.0), rows=1, cols=1)
    img = ops.render_image(p, n)
    torch.cuda.synchronize()
    assert p.shape == (1, 1, 4) and n[0, 0, 3].item() == 1 and abs(p[0, 0, 2].item() - 0.4) < 0.05 * 0.01
    assert img[0, 0].tolist() == [255, 255, 255, 255]


def test_sobfusion_render():
    import torch

    from sobfu_amd import fusion, params, synthetic

    P = params.read_ini(os.path.join(ROOT, "params", "config1_sphere_64.ini"))
    f = fusion.SobFusion(P, max_iter=2)
    try:
        for k in range(2):
            f(torch.from_numpy(synthetic.render_sphere_depth((0.005 * k, 0.0, 0.75), 0.1, P["intr"]).astype(np.int16)).cuda())
        img = f.render("phi_global").cpu().numpy()
        live = f.render("phi_global_psi_inv").cpu().numpy()
    finally:
        f.close()
    assert img.shape == (480, 640, 4) and img[240, 320].tolist() == [255, 255, 255, 255]
    assert live[240, 320, 0] >= 250 and (img[..., 3] == 255).sum() > 10000


def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", None, None
    while pos < len(data):
        (k,) = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + k]
        assert struct.unpack(">I", data[pos + 8 + k:pos + 12 + k])[0] == zlib.crc32(typ + body) & 0xFFFFFFFF
        if typ == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (8, 2)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + k
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 3 * w + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def _app(*args, cwd=None):
    from sobfu_amd import build, build_host

    build.build_hip()
    exe = build_host.build_app()
    r = subprocess.run([exe, os.path.join(ROOT, "params", "config1_sphere_64.ini"), "--synthetic", "2", "--no-stats", *args],
                       capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def test_app_screenshots(tmp_path):
    _app("--screenshots", str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["000000.png", "000001.png"]
    f0, f1 = read_png(tmp_path / "000000.png"), read_png(tmp_path / "000001.png")
    assert f0.shape == f1.shape == (480, 1280, 3)
    assert not f0[:, 640:].any()  # frame 0 has not been solved: the live panel is black
    assert f1[:, 640:].any()
    fx, fy, cx, cy = 570.342, 570.342, 320.0, 240.0
    _, _, dist = sphere_hits(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), (0.0, 0.0, 0.75), 0.1, (fx, fy, cx, cy), 480, 640)
    vox = 0.5 / 64
    lit = f0[:, :640].max(-1) > 0
    assert (f0[:, :640, 0] == f0[:, :640, 1]).all() and (f0[:, :640, 1] == f0[:, :640, 2]).all()  # grey
    assert not lit[dist > 0.1 + 2 * vox].any()
    assert lit[dist < 0.05].all()
    # the valid-sample rule (all 8 corners observed) with ETA = 2 voxels leaves a thin ring of misses where the crossing sample's corners
    # reach more than eta behind the sloped surface -- the restatement gives the same ring
    assert lit[dist < 0.1 - 2 * vox].mean() > 0.9
    assert f0[int(cy), int(cx)].min() >= 250 and f1[int(cy), int(cx)].min() >= 250  # the headlight faces the surface there


def test_app_screenshots_detailed_and_off(tmp_path):
    _app("--screenshots", str(tmp_path), "--screenshots-detailed")
    f1 = read_png(tmp_path / "000001.png")
    assert f1.shape == (960, 1280, 3)
    assert f1[:480, :640].any() and f1[:480, 640:].any() and f1[480:, :640].any() and f1[480:, 640:].any()
    f0 = read_png(tmp_path / "000000.png")
    assert not f0[:480].any() and f0[480:, :640].any() and not f0[480:, 640:].any()
    off = tmp_path / "off"
    off.mkdir()
    out = _app(cwd=str(off))
    assert "screenshot" not in out and not os.listdir(off)
