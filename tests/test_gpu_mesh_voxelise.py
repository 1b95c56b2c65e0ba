"""Closed meshes into signed TSDF volumes on the GPU (sobfu_amd/csrc/mesh_voxel_kernels.hip): ops.TriangleGrid.voxelise and
.inside against the numpy restatement tests/mesh_parity_reference.py bit for bit (a cube whose faces, edges and corners lie exactly on
voxel centres), across grids, modes and runs (an icosphere), against the analytic volumes of init_box and init_sphere, on an open mesh
and on degenerate inputs; and SobFusion.integrate_mesh beside the depth-camera path it replaces, with signed evaluation."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_parity_reference as MP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
MARGIN = 1e-4  # kMeshMargin: the project's bound on one point-triangle distance, in units of the largest coordinate magnitude
VS = 1.0 / 64  # a power of two: voxel centres (i + 1/2) / 64 are exact, and so are the cube's corners on them
TRUNC, ETA = 4 * VS, 2 * VS


def _gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _grid(v, f, cell=None):
    from sobfu_amd import ops

    return ops.TriangleGrid(_gpu(v), _gpu(f), cell=cell)


# the cube of each volume: corners on the voxel centres (i0, i1) per axis, i0 + i1 = dim - 1 (centred, as init_box wants it)
CUBES = {(20, 12, 9): ((4, 15), (3, 8), (2, 6)), (40, 33, 29): ((8, 31), (6, 26), (5, 23)), (70, 9, 5): ((5, 64), (2, 6), (1, 3))}


def _cube(dims, drop=None):
    idx = CUBES[dims]
    lo, hi = [(i0 + 0.5) * VS for i0, _ in idx], [(i1 + 0.5) * VS for _, i1 in idx]
    return MP.cube(lo, hi, drop) + (lo, hi)


@pytest.mark.parametrize("dims", sorted(CUBES))
def test_cube_brute_path_equals_the_restatement_and_init_box(dims):
    """12 triangles (mode auto takes the brute path); ragged bricks; one, two and three mask words, the last one ragged"""
    import torch

    from sobfu_amd import ops

    v, f, lo, hi = _cube(dims)
    vs = (VS, VS, VS)
    g = _grid(v, f)
    vol, open_rows = g.voxelise(dims, vs, TRUNC, ETA)
    want, want_open, want_inside = MP.voxelise(v, f, dims, vs, TRUNC, ETA)
    got = _cpu(vol)
    on_surface = int((MP.box_sdf(MP.voxel_centres(dims, vs)[..., :3], lo, hi) == 0).sum())
    print("cube %s: %d voxels inside, %d exactly on the surface, %d saturated" % (dims, int(want_inside.sum()), on_surface, int((np.abs(want[..., 0]) == 1).sum())))
    assert on_surface > 50 and want_open == 0 and int(open_rows) == 0
    assert np.array_equal(_bits(got[..., 0]), _bits(want[..., 0])), "tsdf differs at %d voxels" % int((_bits(got[..., 0]) != _bits(want[..., 0])).sum())
    assert np.array_equal(_bits(got[..., 1]), _bits(want[..., 1])), "weight differs at %d voxels" % int((_bits(got[..., 1]) != _bits(want[..., 1])).sum())
    for mode in ("grid", "brute"):
        again, o = g.voxelise(dims, vs, TRUNC, ETA, mode=mode)
        assert torch.equal(again.view(torch.int32), vol.view(torch.int32)) and int(o) == 0, mode
    # the analytic box: init_box centres the volume, and the cube is centred in it
    box = ops.new_volume(dims)
    ops.init_box(box, vs, TRUNC, [(i1 - i0) / 2 * VS for i0, i1 in CUBES[dims]])
    ref = _cpu(box)[..., 0].astype(np.float64)
    L = max(dims) * VS
    err = np.abs(got[..., 0].astype(np.float64) - ref).max()
    print("cube %s: |tsdf - init_box| <= %.3g (bound %.3g)" % (dims, err, MARGIN * L / TRUNC))
    assert err <= MARGIN * L / TRUNC
    far = np.abs(ref) * TRUNC > MARGIN * L
    assert far.sum() == ref.size - on_surface  # the next voxel is a whole voxel away from the surface
    assert np.array_equal(got[..., 0][far] < 0, ref[far] < 0)


SPHERE_C, SPHERE_R = (0.16, 0.15, 0.17), 0.1


@pytest.fixture(scope="module")
def sphere():
    """an icosphere of 5120 faces in a 32^3 volume, with two spare vertices that no face uses: they stretch the grid's box to
    0.33 x 0.26 x 0.2, so that cubic cells give it different numbers of cells per axis"""
    v, f = MP.icosphere(SPHERE_R, 4, SPHERE_C)
    assert len(f) == 5120
    spare = np.array([[SPHERE_C[0] - SPHERE_R + 0.33, SPHERE_C[1], SPHERE_C[2], 1], [SPHERE_C[0], SPHERE_C[1] - SPHERE_R + 0.26, SPHERE_C[2], 1]], np.float32)
    v = np.concatenate([v, spare])
    a, b, c = (x.astype(np.float64) for x in MP.corners(v, f))
    n = np.cross(b - a, c - a)
    r_in = float((np.abs(((a - SPHERE_C) * n).sum(1)) / np.linalg.norm(n, axis=1)).min())
    return dict(v=v, f=f, sagitta=SPHERE_R - r_in)


def test_icosphere_grid_path_is_one_volume_whatever_the_cells_and_close_to_init_sphere(sphere):
    import torch

    from sobfu_amd import ops

    dims, vs, trunc, eta = (32, 32, 32), (0.01, 0.01, 0.01), 0.03, 0.01
    v, f = sphere["v"], sphere["f"]
    vols = []
    # 41 x 33 x 25: cells a quarter of the truncation distance, so that a brick's gather radius grows in steps before it stops
    for cell, cells in ((0.5, (1, 1, 1)), (0.07, (5, 4, 3)), (0.049, (7, 6, 5)), (0.0081, (41, 33, 25))):
        g = _grid(v, f, cell)
        assert g.dims == cells
        for mode in ("grid", "grid", "brute") if cells == (5, 4, 3) else ("grid",):
            vol, open_rows = g.voxelise(dims, vs, trunc, eta, mode=mode)
            assert int(open_rows) == 0
            vols.append(vol)
    for vol in vols[1:]:
        assert torch.equal(vol.view(torch.int32), vols[0].view(torch.int32))
    got = _cpu(vols[0])
    ref = ops.new_volume(dims)
    ops.init_sphere(ref, vs, trunc, eta, SPHERE_C, SPHERE_R)
    ref = _cpu(ref)
    L = float(max(np.abs(v[:, :3]).max(), MP.voxel_centres(dims, vs)[..., :3].max()))  # the spare vertex at x = 0.39
    assert 0.38 < L < 0.4
    bound = sphere["sagitta"] + MARGIN * L
    err = float(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]).max())
    print("icosphere: sagitta %.3g, |tsdf - init_sphere| <= %.3g (bound %.3g), %d voxels inside" % (sphere["sagitta"], err, bound / trunc, int((got[..., 0] < 0).sum())))
    assert (got[..., 0] < 0).sum() > 3000 and (np.abs(got[..., 0]) < 1).sum() > 5000
    assert err <= bound / trunc
    sdf = np.linalg.norm(MP.voxel_centres(dims, vs)[..., :3].astype(np.float64) - SPHERE_C, axis=-1) - SPHERE_R
    clear = np.abs(sdf + np.float32(eta)) > bound
    assert clear.sum() > 0.97 * sdf.size and np.array_equal(got[..., 1][clear], ref[..., 1][clear])
    assert set(np.unique(got[..., 1])) == {0.0, 1.0}


@pytest.mark.parametrize("shape", ["cube", "sphere"])
def test_two_schedules_one_rule(shape, sphere):
    """inside(voxel centres), one lane per point, equals the sign bits of voxelise, one wave per row: also where centres lie exactly on
    the cube's faces, edges and corners (d = 0: the sign of the zero)"""
    if shape == "cube":
        dims, vs, trunc, eta = (40, 33, 29), (VS, VS, VS), TRUNC, ETA
        v, f = _cube(dims)[:2]
    else:
        dims, vs, trunc, eta = (32, 32, 32), (0.01, 0.01, 0.01), 0.03, 0.01
        v, f = sphere["v"], sphere["f"]
    p = _gpu(MP.voxel_centres(dims, vs).reshape(-1, 4))
    for mode in ("grid", "brute"):
        g = _grid(v, f, 0.07 if shape == "sphere" else None)
        vol, _ = g.voxelise(dims, vs, trunc, eta, mode=mode)
        ins, opn = g.inside(p, mode=mode)
        sign = np.signbit(_cpu(vol)[..., 0]).reshape(-1)
        assert np.array_equal(_cpu(ins) == 1, sign) and not _cpu(opn).any() and sign.sum() > 1000, (shape, mode)
        if shape == "cube":
            want, want_open = MP.inside(_cpu(p), v, f)
            assert np.array_equal(_cpu(ins), want) and np.array_equal(_cpu(opn), want_open)
            zero = _cpu(vol)[..., 0] == 0
            assert zero.sum() > 50 and np.signbit(_cpu(vol)[..., 0][zero]).any() and not np.signbit(_cpu(vol)[..., 0][zero]).all()


@pytest.mark.parametrize("X,inside", [(1, 4), (32, 40), (33, 44), (512, 640)])
def test_row_lengths(X, inside):
    """one voxel, one full bit word, two words with a ragged second, and the widest row: a closed cube off the lattice, so every row that
    meets it has both signs.  The sign bits are in the format that the winding rows write too (sobfu_mesh_rows.hpp)."""
    import torch

    dims, vs = (X, 3, 2), (0.32 / X, 0.05, 0.05)
    v, f = MP.cube((0.1, 0.02, 0.02), (0.2, 0.12, 0.08))
    want, want_open, want_inside = MP.voxelise(v, f, dims, vs, 0.03, 0.01)
    assert want_open == 0 and int(want_inside.sum()) == inside and not want_inside.all()
    p = _gpu(MP.voxel_centres(dims, vs).reshape(-1, 4))
    g = _grid(v, f)
    for mode in ("grid", "brute"):
        vol, open_rows = g.voxelise(dims, vs, 0.03, 0.01, mode=mode)
        got = _cpu(vol)
        assert np.array_equal(_bits(got), _bits(want)), "X = %d, %s: %d values differ" % (X, mode, int((_bits(got) != _bits(want)).sum()))
        assert int(open_rows) == 0
        ins, opn = g.inside(p, mode=mode)
        assert np.array_equal(_cpu(ins).reshape(-1) == 1, np.signbit(got[..., 0]).reshape(-1)) and not _cpu(opn).any(), (X, mode)
        wvol, _ = g.voxelise(dims, vs, 0.03, 0.01, mode=mode, sign="winding")
        assert torch.equal(wvol.view(torch.int32), vol.view(torch.int32)), (X, mode)


def test_open_cube_is_reported_and_refused_by_integrate_mesh():
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    dims, vs = (40, 33, 29), (VS, VS, VS)
    v, f, lo, hi = _cube(dims, drop=[2])
    want = MP.sign_bits(v, f, dims, vs)[1]
    for mode in ("grid", "brute"):
        assert int(_grid(v, f).voxelise(dims, vs, TRUNC, ETA, mode=mode)[1]) == want > 100, mode
    p = MP.voxel_centres(dims, vs).reshape(-1, 4)
    assert int(_cpu(_grid(v, f).inside(_gpu(p))[1]).sum()) == want * dims[0]
    # a cube of 0.2 m around (0, 0, 0.75) in the camera frame, given in the frame of the meshes the app writes; one triangle missing
    P = read_ini(CONFIG1)
    ov, of = MP.cube((-0.1, -0.1, -0.85), (0.1, 0.1, -0.65), drop=[2])
    fusion = SobFusion(P)
    with pytest.raises(ValueError, match="not closed"):
        fusion.integrate_mesh(ov, of)
    assert fusion.frame == 0 and fusion.phi_global is None and fusion.poses == []
    assert fusion.integrate_mesh(ov, of, allow_open=True) is None and fusion.frame == 1
    fusion.close()


def test_a_refused_grid_and_an_empty_mesh_are_empty_space():
    import torch

    from sobfu_amd import _lib, ops

    dims, vs = (20, 12, 9), (VS, VS, VS)
    v, f = _cube(dims)[:2]
    g = _grid(v, f, 0.05)
    g.faces[5, 1] = 8  # a face index out of range: building again into the same workspace is refused and leaves it unmarked
    refs = C.c_int(0)
    rc = _lib.lib().sobfu_hip_mesh_grid_build(*g._mesh(), *g._plan, *ops._ws(g.workspace), C.c_int(g.references), C.byref(refs), ops._stream())
    assert rc == -1
    empty = ops.TriangleGrid(_gpu(v), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    p = _gpu(MP.voxel_centres(dims, vs).reshape(-1, 4))
    for grid in (g, empty):
        for mode in ("auto", "grid", "brute"):
            vol, open_rows = grid.voxelise(dims, vs, TRUNC, ETA, out=torch.full((9, 12, 20, 2), 7.0, device="cuda"), mode=mode)
            assert int(open_rows) == 0 and torch.all(vol == 1.0)
            ins, opn = grid.inside(p, mode=mode)
            assert not ins.any() and not opn.any()


def _depth_frame(fusion, depth):
    """SobFusion.__call__ as it stood before integrate_mesh split it: the same C-ABI calls in the same order"""
    ops, P = fusion.ops, fusion.P
    fusion.image_shape = tuple(depth.shape)
    dims, vs = P["dims"], tuple(float(v) for v in P["vs"])
    ks, ss, sd = P["bilateral"]
    d = ops.bilateral_filter(depth, ks, ss, sd)
    ops.truncate_depth(d, P["trunc_depth"])
    dists = ops.compute_dists(d, P["intr"])
    fusion.poses.append(fusion.pose.copy())
    R, t = fusion.vol2cam()
    if fusion.frame == 0:
        fusion.phi_global = ops.new_volume(dims)
        ops.integrate_depth(dists, fusion.phi_global, vs, P["trunc"], P["eta"], R, t, P["intr"])
        fusion.phi_global_psi_inv, fusion.phi_n, fusion.phi_n_psi = ops.new_volume(dims), ops.new_volume(dims), ops.new_volume(dims)
        fusion.psi, fusion.psi_inv = ops.new_field(dims), ops.new_field(dims)
        ops.init_identity(fusion.psi)
        ops.init_identity(fusion.psi_inv)
        fusion.solver = ops.Solver(dims, max_iter=fusion.max_iter, alpha=P["alpha"], w_reg=P["w_reg"], s=P["s"], lam=P["lam"], max_update_norm=P["max_update_norm"])
        fusion.frame += 1
        return
    ops.clear_volume(fusion.phi_n)
    ops.integrate_depth(dists, fusion.phi_n, vs, P["trunc"], P["eta"], R, t, P["intr"])
    fusion.last_report = fusion.solver.estimate_psi(fusion.phi_global, fusion.phi_global_psi_inv, fusion.phi_n, fusion.phi_n_psi, fusion.psi, fusion.psi_inv)
    ops.integrate_fuse(fusion.phi_global, fusion.phi_n_psi, P["max_weight"])
    fusion.frame += 1


SHIFT, FRAMES, RADIUS = 0.005, 2, 0.1


def _gt(frame):
    """the icosphere of tests/test_gpu_mesh_frames.py: 5120 faces around (shift n, 0, 0.75) in the camera frame, given as (x, -y, -z)"""
    return MP.icosphere(RADIUS, 4, (SHIFT * frame, 0.0, -0.75))


def test_fusion_driven_by_voxelised_meshes_beside_the_rendered_path():
    """config 1, two frames, the sphere moved 5 mm: integrate_mesh against render_mesh_depth + __call__ (the yardstick), both scored by
    evaluate(which="live") against the last frame's icosphere.  The rendered path carries 1 mm of depth quantisation that the voxelised
    one lacks: rms(voxelised) <= rms(rendered) + sagitta.  __call__ itself still makes the bits its body made before it was split."""
    import torch

    from sobfu_amd import mesh_render
    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    gv, gf = _gt(FRAMES - 1)
    a, b, c = (x.astype(np.float64) for x in MP.corners(gv, gf))
    n = np.cross(b - a, c - a)
    sagitta = RADIUS - float((np.abs(((a - [SHIFT * (FRAMES - 1), 0.0, -0.75]) * n).sum(1)) / np.linalg.norm(n, axis=1)).min())
    assert 0 < sagitta < 2e-4
    depths = [_gpu(mesh_render.render_mesh_depth(*_gt(k), P["intr"], pose=mesh_render.MESH_FRAME)) for k in range(FRAMES)]
    runs = {}
    for source in ("voxelised", "rendered", "rendered, the former body"):
        fusion = SobFusion(P)
        for k in range(FRAMES):
            if source == "voxelised":
                fusion.integrate_mesh(*_gt(k))
            elif source == "rendered":
                fusion(depths[k])
            else:
                _depth_frame(fusion, depths[k])
        assert fusion.frame == FRAMES and len(fusion.poses) == FRAMES and fusion.last_report is not None
        r = fusion.evaluate(gv, gf, which="live", signed=True)
        plain = fusion.evaluate(gv, gf, which="live")
        runs[source] = dict(r=r, psi=fusion.psi.clone(), phi=fusion.phi_global.clone())
        for side in ("a_to_b", "b_to_a"):
            assert set(r[side]) == set(plain[side]) | {"signed_mean", "inside", "open"}
            assert all(r[side][k] == plain[side][k] for k in plain[side])
        assert r["chamfer"] == plain["chamfer"] and r["hausdorff"] == plain["hausdorff"]
        ab = r["a_to_b"]
        print("%s: a_to_b rms %.6g mean %.6g signed_mean %.6g, %d of %d model vertices inside the ground truth, %d on open rows"
              % (source, ab["rms"], ab["mean"], ab["signed_mean"], ab["inside"], ab["within"], ab["open"]))
        assert ab["within"] == ab["n"] > 100 and ab["open"] == 0  # the ground truth is closed
        assert np.isfinite(ab["signed_mean"]) and abs(ab["signed_mean"]) <= ab["mean"] and 0 <= ab["inside"] <= ab["within"]
        fusion.close()
    for key in ("psi", "phi"):
        assert torch.equal(runs["rendered"][key].view(torch.int32), runs["rendered, the former body"][key].view(torch.int32)), key
    vox, ren = runs["voxelised"]["r"]["a_to_b"]["rms"], runs["rendered"]["r"]["a_to_b"]["rms"]
    print("a_to_b rms: voxelised %.6g m, rendered %.6g m, sagitta %.3g m" % (vox, ren, sagitta))
    assert vox <= ren + sagitta


def test_app_voxelise_mesh_and_evaluate_signed(tmp_path):
    """sobfu_headless --voxelise-mesh PATTERN --evaluate-live PATTERN --evaluate-signed on two written .ply files: the meshes are fused as
    volumes and every solved frame (frame 0 is never solved) prints one evaluate line, with the signed fields; without --evaluate-signed
    the line is the one --render-mesh prints; an open mesh ends the run"""
    import re
    import subprocess

    from sobfu_amd import build, build_host, mesh_io
    from sobfu_amd.params import read_ini

    build.build_hip()
    exe = build_host.build_app()
    for n in range(2):
        gv, gf = _gt(n)
        nrm = gv.copy()
        nrm[:, :3] = (gv[:, :3] - np.array([SHIFT * n, 0, -0.75], np.float32)) / np.float32(RADIUS)
        mesh_io.write_ply(tmp_path / ("gt_%06d.ply" % n), gv, nrm, gf)
        cap = gv[gf][:, :, 0].mean(1) > SHIFT * n + 0.08  # the faces around the +x pole: a hole 0.12 m across, seen along the rows
        assert 50 < cap.sum() < 1000
        mesh_io.write_ply(tmp_path / ("open_%06d.ply" % n), gv, nrm, gf[~cap])
    pattern = str(tmp_path / "gt_%06d.ply")
    line = re.compile(r"^evaluate live (\d+): (.*)$", re.M)
    P = read_ini(CONFIG1)
    fields = {}
    for extra in (["--evaluate-signed"], []):
        r = subprocess.run([exe, CONFIG1, "--no-stats", "--voxelise-mesh", pattern, "--evaluate-live", pattern] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        lines = line.findall(r.stdout)
        print("\n".join("evaluate live %s: %s" % l for l in lines))
        assert [int(n) for n, _ in lines] == [1]
        fields[bool(extra)] = dict(kv.split("=") for kv in lines[0][1].split())
    got, plain = fields[True], fields[False]
    assert set(got) == set(plain) | {side + "." + k for side in ("a_to_b", "b_to_a") for k in ("signed_mean", "inside", "open")}
    assert all(got[k] == plain[k] for k in plain)
    assert int(got["a_to_b.within"]) == int(got["a_to_b.n"]) > 100 and int(got["a_to_b.open"]) == 0
    assert abs(float(got["a_to_b.signed_mean"])) <= float(got["a_to_b.mean"]) <= float(got["a_to_b.rms"]) < float(P["trunc"])
    assert 0 <= int(got["a_to_b.inside"]) <= int(got["a_to_b.within"])
    bad = subprocess.run([exe, CONFIG1, "--no-stats", "--voxelise-mesh", str(tmp_path / "open_%06d.ply")], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 2 and "not closed" in bad.stdout
    both = subprocess.run([exe, CONFIG1, "--voxelise-mesh", pattern, "--render-mesh", pattern], capture_output=True, text=True, timeout=60)
    assert both.returncode == 2 and "exclude each other" in both.stdout
