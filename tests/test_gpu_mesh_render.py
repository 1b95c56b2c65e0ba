"""The mesh camera on the GPU (sobfu_hip_mesh_render, sobfu_amd/csrc/mesh_ray_kernels.hip): depth, triangle index, points, normals and
colour against the numpy restatement tests/mesh_ray_reference.py bit for bit on an odd, pitched frame under a non-identity pose; depth
against the analytic sphere; the points and normals through ops.render_image; 1 x 1 and partial-tile frames."""
import numpy as np
import pytest

import mesh_ray_reference as MR

pytestmark = pytest.mark.gpu
ALL = ("depth", "tri", "points", "normals", "colour")


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    """an icosphere of 320 faces (r = 0.1) with unit vertex normals and random vertex colours, in a frame of its own; the pose puts its
    centre 0.6 m in front of the camera, about 10 pixels wide in radius at f = 60"""
    centre = np.array([0.05, -0.03, 0.1])
    v, f = MR.icosphere(0.1, 2, centre)
    n = np.zeros_like(v)
    n[:, :3] = (v[:, :3].astype(np.float64) - centre) / 0.1
    colours = np.random.default_rng(5).integers(0, 256, (len(v), 4)).astype(np.uint8)
    R = _rotation((1, 2, 3), 0.4)
    t = (np.array([0.02, -0.01, 0.6]) - R.astype(np.float64) @ centre).astype(np.float32)
    return dict(v=v, f=f, n=n, c=colours, R=R, t=t)


def _grid(scene):
    from sobfu_amd import ops

    return ops.TriangleGrid(_gpu(scene["v"]), _gpu(scene["f"]))


def _equal(got, want, what):
    for name in want:
        if name in got:
            g = np.ascontiguousarray(_cpu(got[name]))
            g = g.view(np.uint16) if name == "depth" else g
            assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
            bad = np.argwhere((g != want[name]) if g.ndim == 2 else (g.view(np.uint8 if g.dtype == np.uint8 else np.uint32) != want[name].view(
                np.uint8 if g.dtype == np.uint8 else np.uint32)).any(-1))
            assert len(bad) == 0, "%s %s differs at %d pixels, first %s: got %r want %r" % (what, name, len(bad), bad[0], g[tuple(bad[0])], want[name][tuple(bad[0])])


def _pitched(rows, cols, extra=5):
    """images whose rows are `extra` pixels wider than the frame, filled with a pattern that a write beyond the frame would disturb"""
    import torch

    kinds = {"depth": (torch.int16, 0), "tri": (torch.int32, 0), "points": (torch.float32, 4), "normals": (torch.float32, 4), "colour": (torch.uint8, 4)}
    whole = {k: torch.full((rows, cols + extra, ch) if ch else (rows, cols + extra), 77, dtype=dt, device="cuda") for k, (dt, ch) in kinds.items()}
    return whole, {k: w[:, :cols] for k, w in whole.items()}


def test_an_odd_pitched_frame_under_a_pose(scene):
    rows, cols, intr = 23, 37, (60.0, 61.0, 18.2, 10.7)
    g = _grid(scene)
    want = MR.render(scene["v"], scene["f"], intr, rows, cols, scene["R"], scene["t"], vertex_normals=scene["n"], vertex_colours=scene["c"])
    hit = want["tri"] >= 0
    assert 150 < hit.sum() < 0.6 * rows * cols and len(np.unique(want["tri"][hit])) > 50
    assert np.all(want["depth"][hit] > 450) and np.all(want["depth"][hit] < 650)
    for name in ("depth", "points", "normals", "colour"):  # the documented zeros of a miss
        assert not want[name][~hit].any() and want[name][hit].reshape(hit.sum(), -1).any(1).all(), name
    assert np.all(want["normals"][hit][:, 3] == 1) and np.all(want["points"][hit][:, 3] == 0) and np.all(want["colour"][hit][:, 3] == 255)
    assert np.all((want["normals"][hit][:, :3] * want["points"][hit][:, :3]).sum(1) <= 1e-6)  # they face the camera, up to the rotation's rounding
    kw = dict(pose=(scene["R"], scene["t"]), vertex_normals=_gpu(scene["n"]), vertex_colours=_gpu(scene["c"]))
    _equal(g.render(intr, rows, cols, outputs=ALL, **kw), want, "dense")
    whole, views = _pitched(rows, cols)
    got = g.render(intr, rows, cols, outputs=views, **kw)
    _equal(got, want, "pitched")
    for name, w in whole.items():
        assert np.all(_cpu(w)[:, cols:] == 77), name  # nothing written between the rows
    for left_out in ALL:  # every output pointer NULL in turn
        some = tuple(n for n in ALL if n != left_out)
        got = g.render(intr, rows, cols, outputs=some, **kw)
        assert sorted(got) == sorted(some)
        _equal(got, want, "without " + left_out)
    # without vertex normals: the face normals; depth limits
    flat = MR.render(scene["v"], scene["f"], intr, rows, cols, scene["R"], scene["t"])
    assert (flat["normals"] != want["normals"]).any()
    _equal(g.render(intr, rows, cols, pose=kw["pose"], outputs=("depth", "tri", "points", "normals")), flat, "face normals")
    z_min, z_max = 0.52, 0.58
    cut = MR.render(scene["v"], scene["f"], intr, rows, cols, scene["R"], scene["t"], z_min, z_max, scene["n"], scene["c"])
    assert 0 < (cut["tri"] >= 0).sum() and (cut["tri"] != want["tri"]).sum() > 20
    _equal(g.render(intr, rows, cols, z_min=z_min, z_max=z_max, outputs=ALL, **kw), cut, "depth limits")
    with pytest.raises(ValueError):
        g.render(intr, rows, cols, outputs=("colour",))
    with pytest.raises(ValueError):
        g.render(intr, rows, cols, outputs=("shadow",))


@pytest.mark.parametrize("rows, cols", [(1, 1), (9, 70)])
def test_size_cases(scene, rows, cols):
    """one pixel; partial 8 x 8 tiles on both axes"""
    intr = (60.0, 60.0, 0.3 if cols == 1 else 33.0, 0.2 if rows == 1 else 4.0)
    want = MR.render(scene["v"], scene["f"], intr, rows, cols, scene["R"], scene["t"], vertex_normals=scene["n"], vertex_colours=scene["c"])
    assert (want["tri"] >= 0).any()
    whole, views = _pitched(rows, cols, 3)
    got = _grid(scene).render(intr, rows, cols, pose=(scene["R"], scene["t"]), vertex_normals=_gpu(scene["n"]), vertex_colours=_gpu(scene["c"]), outputs=views)
    _equal(got, want, "%d x %d" % (rows, cols))
    for name, w in whole.items():
        assert np.all(_cpu(w)[:, cols:] == 77), name


def test_against_the_analytic_sphere_and_through_render_image():
    """An icosphere inscribed in the sphere (c, r) lies between that sphere and the concentric one of radius r_in, the distance from c to
    its nearest face plane.  A pixel whose ray passes c nearer than r_in hits the mesh, at a depth between the analytic depths of the two
    spheres (+- 1 mm: each is rounded to millimetres); one whose ray passes farther than r misses."""
    from sobfu_amd import mesh_render, ops, synthetic as S

    c, r, intr, rows, cols = np.array([0.01, 0.02, 0.75]), 0.1, (150.0, 150.0, 64.0, 48.0), 96, 128
    v, f = MR.icosphere(r, 3, c)
    tri = v[f][:, :, :3].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float((np.abs(((tri[:, 0] - c) * n).sum(1)) / np.linalg.norm(n, axis=1)).min())
    assert 0.98 * r < r_in < r
    u, w = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    d = np.stack([(u - intr[2]) / intr[0], (w - intr[3]) / intr[1], np.ones_like(u)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    passes = np.linalg.norm(c - (d @ c)[..., None] * d, axis=-1)
    depth = mesh_render.render_mesh_depth(v, f, intr, rows, cols)
    assert depth.dtype == np.uint16 and depth.shape == (rows, cols)
    outer, inner = S.render_sphere_depth(c, r, intr, rows, cols).astype(np.int64), S.render_sphere_depth(c, r_in, intr, rows, cols).astype(np.int64)
    must_hit, must_miss = passes < r_in, passes > r
    print("analytic sphere: r_in = %.6f, %d pixels must hit, %d must miss, %d in the band between" % (r_in, must_hit.sum(), must_miss.sum(), (~must_hit & ~must_miss).sum()))
    assert must_hit.sum() > 1000 and must_miss.sum() > 1000
    assert np.all(depth[must_hit] > 0) and np.all(depth[must_miss] == 0)
    assert np.all(depth[must_hit] >= outer[must_hit] - 1) and np.all(depth[must_hit] <= inner[must_hit] + 1)
    # the points and normals go through render_image unchanged: a non-black image on exactly the hit pixels
    g = mesh_render.mesh_grid(v, f)
    out = g.render(intr, rows, cols, outputs=("depth", "points", "normals"))
    assert np.array_equal(_cpu(out["depth"]).view(np.uint16), depth)
    image = _cpu(ops.render_image(out["points"], out["normals"]))
    assert np.array_equal(image[..., :3].any(-1), depth > 0) and np.array_equal(image.any(-1), depth > 0)
    # the colour twin: the corners' colours mixed, alpha 255 on exactly the hit pixels
    colours = np.random.default_rng(6).integers(0, 256, (len(v), 4)).astype(np.uint8)
    img = mesh_render.render_mesh_colour(v, f, colours, intr, rows, cols, grid=g)
    assert img.dtype == np.uint8 and img.shape == (rows, cols, 4) and np.array_equal(img[..., 3] == 255, depth > 0) and not img[depth == 0].any()
    assert np.array_equal(img, MR.render(v, f, intr, rows, cols, vertex_colours=colours)["colour"])
