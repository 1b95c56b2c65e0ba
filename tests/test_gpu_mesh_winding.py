"""Generalised winding numbers on the GPU (sobfu_amd/csrc/mesh_winding_kernels.hip): ops.TriangleGrid.winding and
voxelise(sign="winding") against the parity path on closed meshes (bit for bit), against the float64 restatement
tests/mesh_winding_reference.py and the independent definition (mode="sum") on open meshes, across grids, walks and runs, at the edges of
the interface, and through SobFusion.integrate_mesh and compare_meshes."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_parity_reference as MP
import mesh_winding_reference as MW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG1 = os.path.join(ROOT, "params", "config1_sphere_64.ini")
VS = 1.0 / 64  # a power of two: the cube's corners lie exactly on voxel centres
TRUNC, ETA = 4 * VS, 2 * VS
CUBES = {(20, 12, 9): ((4, 15), (3, 8), (2, 6)), (70, 9, 5): ((5, 64), (2, 6), (1, 3))}
SPHERE_C, SPHERE_R = (0.16, 0.15, 0.17), 0.1
SPHERE = dict(dims=(32, 32, 32), vs=(0.01, 0.01, 0.01), trunc=0.03, eta=0.01)
# max |w_gpu - w_restatement| farther than a voxel from the boundary edges, measured on the MI355X: the output is a float32, and half an ulp
# of a float32 in [1, 2) is 6.0e-8 (the doubled soup reaches |w| > 1); the float64 sum itself agrees to 1e-15.  The tests hold 16 x that.
MEASURED = 5.96e-8
BOUND = 16 * MEASURED
assert BOUND < 1e-3


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


def _box(dims):
    idx = CUBES[dims]
    return [(i0 + 0.5) * VS for i0, _ in idx], [(i1 + 0.5) * VS for _, i1 in idx]


def _cube(dims, drop=None):
    return MP.cube(*_box(dims), drop)


def _with_spares(v):
    """two spare vertices that no face uses stretch the grid's box, as in tests/test_gpu_mesh_voxelise.py: cubic cells then give it
    different numbers of cells per axis"""
    spare = np.array([[SPHERE_C[0] - SPHERE_R + 0.33, SPHERE_C[1], SPHERE_C[2], 1], [SPHERE_C[0], SPHERE_C[1] - SPHERE_R + 0.26, SPHERE_C[2], 1]], np.float32)
    return np.concatenate([v, spare])


def _reference(v, f, dims, vs, stride=1, box=None):
    """-> dict: p (n, 4) the voxel centres, w the restatement's boundary formula at all of them (float64), seam, far (farther than one voxel
    from every boundary edge and off the mesh, where w jumps: `box`, the (lo, hi) of a lattice-aligned cube whose faces hold centres),
    sub / w_def: every `stride`-th centre and the restatement's DEFINITION there"""
    p = MP.voxel_centres(dims, vs).reshape(-1, 4)
    N, open_rows = MW.crossings_beyond_centres(v, f, dims, vs)
    w, seam = MW.winding_boundary(p, v, f, return_seam=True, N=N)
    chain = MW.boundary_chain(f, len(v))
    far = MW.distance_to_edges(p, v, chain) > max(vs)
    if box is not None:
        far &= MP.box_sdf(p[:, :3], *box) != 0
    sub = np.arange(0, len(p), stride)
    return dict(p=p, w=w, seam=seam, far=far, chain=chain, open_rows=open_rows, sub=sub, w_def=MW.winding_sum(p[sub], v, f))


@pytest.fixture(scope="module")
def capped():
    """the 5120-face icosphere without the faces whose centroid lies above 0.8 r along x -- the rows look through the hole -- in 32^3"""
    v, f = MW.capped_icosphere(SPHERE_R, 4, SPHERE_C, 0.8, axis=0)
    v = _with_spares(v)
    ref = _reference(v, f, SPHERE["dims"], SPHERE["vs"], stride=17)
    assert len(f) == 4604 and len(ref["chain"]) == 68 and np.all(np.abs(ref["chain"][:, 2]) == 1)
    return dict(v=v, f=f, ref=ref)


OPEN = ["two faces off", "capped icosphere", "doubled triangle"]


@pytest.fixture(scope="module")
def open_meshes(capped):
    """name -> dict(v, f, dims, vs, trunc, eta, ref): the three open inputs, each with its reference, computed once"""
    dims = (20, 12, 9)
    out = {"capped icosphere": dict(capped, **SPHERE)}
    v, f = _cube(dims, [2, 3, 6, 7])  # +x and +y off: ties and seams
    out["two faces off"] = dict(v=v, f=f, dims=dims, vs=(VS,) * 3, trunc=TRUNC, eta=ETA, ref=_reference(v, f, dims, (VS,) * 3, box=_box(dims)))
    # a soup: the cube without +x, moved off the lattice, one triangle of its -y face listed twice and one of -z listed three times
    v, f = _cube(dims, [2, 3])
    v = v.copy()
    v[:, :3] += np.float32(0.37 * VS)
    f = np.ascontiguousarray(np.concatenate([f, f[2:3], f[6:7], f[6:7]]))
    out["doubled triangle"] = dict(v=v, f=f, dims=dims, vs=(VS,) * 3, trunc=TRUNC, eta=ETA, ref=_reference(v, f, dims, (VS,) * 3))
    assert sorted(set(np.abs(out["doubled triangle"]["ref"]["chain"][:, 2]).tolist())) == [1, 2]
    return out


# ---- 1. closed meshes: nothing changes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cube 20 x 12 x 9", "cube 70 x 9 x 5", "icosphere"])
def test_closed_meshes_give_the_parity_volume_bit_for_bit_and_w_is_inside(shape):
    import torch

    if shape == "icosphere":
        a = dict(SPHERE)
        v, f = MP.icosphere(SPHERE_R, 4, SPHERE_C)
        assert len(f) == 5120
    else:
        dims = (20, 12, 9) if "20" in shape else (70, 9, 5)
        a = dict(dims=dims, vs=(VS,) * 3, trunc=TRUNC, eta=ETA)
        v, f = _cube(dims)
    X, Y, Z = a["dims"]
    g = _grid(v, f)
    assert g.boundary.shape == (0, 2, 4)
    vol, open_rows = g.voxelise(a["dims"], a["vs"], a["trunc"], a["eta"])
    wout = torch.full((Z, Y, X), 7.0, device="cuda")
    wvol, wopen = g.voxelise(a["dims"], a["vs"], a["trunc"], a["eta"], sign="winding", winding_out=wout)
    assert int(open_rows) == 0 and int(wopen) == 0
    assert torch.equal(wvol.view(torch.int32), vol.view(torch.int32))
    p = _gpu(MP.voxel_centres(a["dims"], a["vs"]).reshape(-1, 4))
    ins = g.inside(p)[0]
    for mode in ("boundary",):
        w = g.winding(p, mode=mode)
        assert torch.equal(w, ins.to(torch.float32)) and set(np.unique(_cpu(w))) == {0.0, 1.0}
    assert torch.equal(wout.reshape(-1), ins.to(torch.float32))
    print("%s: %d voxels inside" % (shape, int(ins.sum())))


# ---- 2. open meshes: the boundary formula against the restatement and the definition --------------------------------------------------
@pytest.mark.parametrize("name", OPEN)
def test_open_meshes_boundary_mode_against_the_restatement_and_the_sum(name, open_meshes):
    m = open_meshes[name]
    ref = m["ref"]
    g = _grid(m["v"], m["f"])
    assert g.boundary.shape == (len(ref["chain"]), 2, 4) and np.array_equal(g.boundary_edges, ref["chain"])
    p = _gpu(ref["p"])
    w_b, w_s = _cpu(g.winding(p)).astype(np.float64), _cpu(g.winding(p, mode="sum")).astype(np.float64)
    far, sub = ref["far"], ref["sub"]
    e_restated = np.abs(w_b - ref["w"])[far].max()
    e_sum = np.abs(w_b - w_s)[far].max()
    e_def = np.abs(w_b[sub] - ref["w_def"])[far[sub]].max()
    e_sum_def = np.abs(w_s[sub] - ref["w_def"])[far[sub]].max()
    print("%s: %d edges, %d of %d centres farther than a voxel from them, %d seam points; max |w - restatement| %.3g, |w - sum mode| %.3g, "
          "|w - float64 definition| %.3g, |sum mode - float64 definition| %.3g (bound %.3g); everywhere: %.3g; w in [%.4f, %.4f]"
          % (name, len(ref["chain"]), int(far.sum()), len(far), int(ref["seam"].sum()), e_restated, e_sum, e_def, e_sum_def, BOUND,
             np.abs(w_b - ref["w"]).max(), w_b.min(), w_b.max()))
    assert far.sum() > 0.5 * len(far)
    assert e_restated <= BOUND and e_def <= BOUND and e_sum <= BOUND and e_sum_def <= BOUND
    if name == "two faces off":
        assert (ref["seam"] & far).sum() > 0  # the seam fallback runs on the GPU too


# ---- 3. signs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPEN)
def test_open_meshes_sign_bits_and_unchanged_magnitudes(name, open_meshes):
    import torch

    m = open_meshes[name]
    ref = m["ref"]
    X, Y, Z = m["dims"]
    g = _grid(m["v"], m["f"])
    wout = torch.empty((Z, Y, X), device="cuda")
    vol, open_rows = g.voxelise(m["dims"], m["vs"], m["trunc"], m["eta"], sign="winding", winding_out=wout)
    parity, parity_open = g.voxelise(m["dims"], m["vs"], m["trunc"], m["eta"])
    assert int(open_rows) == int(parity_open) == ref["open_rows"] > 0
    got, old = _cpu(vol).reshape(-1, 2), _cpu(parity).reshape(-1, 2)
    clear = np.abs(ref["w"] - 0.5) > 1e-3
    inside = np.signbit(got[:, 0])
    excluded = 1.0 - clear.mean()
    flipped = int((inside != np.signbit(old[:, 0])).sum())
    print("%s: %.2f %% of the centres within 1e-3 of the 1/2 level, %d inside, %d signs differ from the parity volume's, %d open rows"
          % (name, 100 * excluded, int(inside.sum()), flipped, int(open_rows)))
    assert excluded <= 0.02
    assert np.array_equal(inside[clear], (ref["w"] > 0.5)[clear]) and inside.sum() > 100
    assert np.array_equal(inside[clear], (_cpu(wout).reshape(-1) > 0.5)[clear])
    # the distances do not depend on the sign rule
    assert np.array_equal(_bits(np.abs(got[:, 0])), _bits(np.abs(old[:, 0])))
    same = inside == np.signbit(old[:, 0])
    assert np.array_equal(_bits(got[same]), _bits(old[same])) and flipped > 0
    # and the volume is the restatement's: its distances with these signs, the weight by the signed distance (checked where the distance
    # is clear of eta: pack_tsdf divides by the truncation distance and this multiplies it back)
    if name != "capped icosphere":  # (its 1.5e8 point-triangle pairs take numpy a quarter of a minute; the parity volume above has them)
        want = MP.voxelise(m["v"], m["f"], m["dims"], m["vs"], m["trunc"], m["eta"])[0].reshape(-1, 2)
        assert np.array_equal(_bits(np.abs(want[:, 0])), _bits(np.abs(got[:, 0])))
    d = np.abs(got[:, 0].astype(np.float64)) * m["trunc"]
    decided = (np.abs(got[:, 0]) == 1) | (np.abs(d - m["eta"]) > 1e-6)
    assert np.array_equal(got[:, 1][decided], np.where(inside & (d >= m["eta"]), 0.0, 1.0).astype(np.float32)[decided]) and decided.mean() > 0.8


# ---- 4. determinism, grids and walks ----------------------------------------------------------------------------------------------------
def test_one_w_and_one_volume_whatever_the_cells_the_walk_and_the_run(capped):
    import torch

    X, Y, Z = SPHERE["dims"]
    p = _gpu(capped["ref"]["p"])
    ws, vols = [], []
    for cell, cells in ((0.5, (1, 1, 1)), (0.07, (5, 4, 3)), (0.0081, (41, 33, 25))):
        g = _grid(capped["v"], capped["f"], cell)
        assert g.dims == cells
        for mode in ("grid", "grid", "brute") if cells == (5, 4, 3) else ("grid",):
            wout = torch.empty((Z, Y, X), device="cuda")
            vol, _ = g.voxelise(SPHERE["dims"], SPHERE["vs"], SPHERE["trunc"], SPHERE["eta"], mode=mode, sign="winding", winding_out=wout)
            vols.append(vol)
            ws += [wout.reshape(-1), g.winding(p, walk=mode)]  # the row kernel and the point kernel: two schedules, one rule
    for w in ws[1:]:
        assert torch.equal(w.view(torch.int32), ws[0].view(torch.int32))
    for vol in vols[1:]:
        assert torch.equal(vol.view(torch.int32), vols[0].view(torch.int32))
    s = [g.winding(p, mode="sum") for _ in range(2)]
    assert torch.equal(s[0].view(torch.int32), s[1].view(torch.int32))


# ---- 5. the edges of the interface --------------------------------------------------------------------------------------------------------
def test_nothing_to_do():
    import torch

    from sobfu_amd import _lib, ops

    dims, vs = (20, 12, 9), (VS,) * 3
    v, f = _cube(dims, [2, 3])
    g = _grid(v, f, 0.05)
    p = _gpu(MP.voxel_centres(dims, vs).reshape(-1, 4))
    for mode in ("boundary", "sum"):
        assert g.winding(p[:0], mode=mode).shape == (0,)
    assert g.boundary.shape == (4, 2, 4)
    g.faces[5, 1] = 8  # a face index out of range: building again into the same workspace is refused and leaves it unmarked
    refs = C.c_int(0)
    rc = _lib.lib().sobfu_hip_mesh_grid_build(*g._mesh(), *g._plan, *ops._ws(g.workspace), C.c_int(g.references), C.byref(refs), ops._stream())
    assert rc == -1
    empty = ops.TriangleGrid(_gpu(v), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert empty.boundary.shape == (0, 2, 4)
    for grid in (g, empty):
        for mode in ("auto", "grid", "brute"):
            wout = torch.full((9, 12, 20), 7.0, device="cuda")
            vol, open_rows = grid.voxelise(dims, vs, TRUNC, ETA, out=torch.full((9, 12, 20, 2), 7.0, device="cuda"), mode=mode, sign="winding", winding_out=wout)
            assert int(open_rows) == 0 and torch.all(vol == 1.0) and torch.all(wout == 0.0)
            assert torch.all(grid.winding(p, walk=mode) == 0.0) and torch.all(grid.winding(p, mode="sum") == 0.0)
    with pytest.raises(ValueError):
        empty.voxelise(dims, vs, TRUNC, ETA, sign="odd")
    with pytest.raises(ValueError):
        empty.voxelise(dims, vs, TRUNC, ETA, winding_out=torch.empty((9, 12, 20), device="cuda"))
    with pytest.raises(ValueError):
        empty.voxelise((513, 2, 2), vs, TRUNC, ETA, sign="winding")
    with pytest.raises(ValueError):
        empty.winding(p, mode="strips")


@pytest.mark.parametrize("X", [1, 33, 512])
def test_row_lengths(X):
    """one voxel, two bit words with a ragged second, and the widest row: the cube without +x and +y, off the lattice"""
    import torch

    dims, vs = (X, 3, 2), (0.32 / X, 0.05, 0.05)
    v, f = MP.cube((0.1, 0.02, 0.02), (0.2, 0.12, 0.08), [2, 3, 6, 7])
    ref = _reference(v, f, dims, vs)
    g = _grid(v, f)
    wout = torch.empty((2, 3, X), device="cuda")
    vol, _ = g.voxelise(dims, vs, 0.03, 0.01, sign="winding", winding_out=wout)
    w = _cpu(wout).reshape(-1).astype(np.float64)
    err = np.abs(w - ref["w"]).max()
    clear = np.abs(ref["w"] - 0.5) > 1e-3
    print("X = %d: max |w - restatement| %.3g over all %d centres, %d inside" % (X, err, len(w), int((ref["w"] > 0.5).sum())))
    assert err <= BOUND
    assert np.array_equal(np.signbit(_cpu(vol)[..., 0]).reshape(-1)[clear], (ref["w"] > 0.5)[clear])
    assert torch.equal(g.winding(_gpu(ref["p"])).view(torch.int32), wout.reshape(-1).view(torch.int32))


def test_a_boundary_longer_than_one_stage():
    """the open cube as a soup -- every triangle with corners of its own, so every edge is a boundary edge -- twelve times over: 288 edges
    (the rows stage 64, the points 256), coincident edges cancelling in the sum, coefficients adding up: w = 12 x the single cube's"""
    import torch

    dims, vs = (20, 12, 9), (VS,) * 3
    v1, f1 = _cube(dims, [2, 3, 6, 7])
    v1 = v1.copy()
    v1[:, :3] += np.float32(0.37 * VS)
    single = _reference(v1, f1, dims, vs)
    v = np.tile(v1[f1.reshape(-1)], (12, 1))
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    ref = _reference(v, f, dims, vs)
    assert len(ref["chain"]) == 288 and len(f) == 96
    g = _grid(v, f)
    wout = torch.empty((9, 12, 20), device="cuda")
    g.voxelise(dims, vs, TRUNC, ETA, sign="winding", winding_out=wout)
    w_rows, w_points = _cpu(wout).reshape(-1).astype(np.float64), _cpu(g.winding(_gpu(ref["p"]))).astype(np.float64)
    far = single["far"]
    e_rows, e_points, e_single = np.abs(w_rows - ref["w"])[far].max(), np.abs(w_points - ref["w"])[far].max(), np.abs(w_rows - 12 * single["w"])[far].max()
    print("288 edges: max |w - restatement| rows %.3g, points %.3g; |w - 12 w_single| %.3g; w in [%.3f, %.3f]" % (e_rows, e_points, e_single, w_rows.min(), w_rows.max()))
    # |w| reaches 12: half an ulp of a float32 in [8, 16) is 8 x that of [1, 2)
    assert e_rows <= 8 * BOUND and e_points <= 8 * BOUND and e_single <= 8 * BOUND
    assert np.array_equal(w_rows, w_points) and w_rows.max() > 6


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
SHIFT, FRAMES, RADIUS = 0.005, 2, 0.1


def _gt(frame, capped):
    """the icosphere of tests/test_gpu_mesh_voxelise.py around (shift n, 0, 0.75) in the camera frame, given as (x, -y, -z); capped: without
    the faces around its +x pole, a hole 0.12 m across that the rows look through"""
    v, f = MP.icosphere(RADIUS, 4, (SHIFT * frame, 0.0, -0.75))
    if capped:
        f = np.ascontiguousarray(f[v[f][:, :, 0].mean(1) <= SHIFT * frame + 0.08])
    return v, f


def test_fusion_takes_an_open_mesh_with_the_winding_sign():
    import torch

    from sobfu_amd.fusion import SobFusion
    from sobfu_amd.params import read_ini

    P = read_ini(CONFIG1)
    refused = SobFusion(P)
    with pytest.raises(ValueError, match="not closed"):
        refused.integrate_mesh(*_gt(0, True))
    assert refused.frame == 0 and refused.phi_global is None
    refused.close()
    runs = {}
    for source in ("open, winding", "closed, parity", "closed, winding"):
        fusion = SobFusion(P)
        first = None
        for k in range(FRAMES):
            fusion.integrate_mesh(*_gt(k, source.startswith("open")), sign="winding" if "winding" in source else "parity")
            first = fusion.phi_global.clone() if k == 0 else first
        assert fusion.frame == FRAMES and len(fusion.poses) == FRAMES and fusion.last_report is not None
        r = fusion.evaluate(*_gt(FRAMES - 1, False), which="live", signed="winding")
        runs[source] = dict(first=first, phi=fusion.phi_global.clone(), r=r)
        print("%s: a_to_b rms %.6g signed_mean %.6g inside %d of %d" % (source, r["a_to_b"]["rms"], r["a_to_b"]["signed_mean"], r["a_to_b"]["inside"], r["a_to_b"]["within"]))
        fusion.close()
    for key in ("first", "phi"):  # a closed mesh: the sign rule changes nothing
        assert torch.equal(runs["closed, winding"][key].view(torch.int32), runs["closed, parity"][key].view(torch.int32)), key
    a, b = _cpu(runs["open, winding"]["first"]), _cpu(runs["closed, parity"]["first"])
    differ = np.signbit(a[..., 0]) != np.signbit(b[..., 0])
    print("frame 0: %d of %d voxels change sign with the cap removed" % (int(differ.sum()), differ.size))
    assert 0 < differ.sum() < 0.03 * differ.size and np.signbit(a[..., 0]).sum() > 0.9 * np.signbit(b[..., 0]).sum()
    rms = runs["open, winding"]["r"]["a_to_b"]["rms"]
    assert np.isfinite(rms) and rms < float(P["trunc"])


def test_compare_meshes_signed_by_the_winding_number():
    """a sphere moved by 0.3 r along y against the capped sphere (winding) and against its closed original (parity): the 1/2 level across
    the hole is the flat disc of its rim, so only vertices beyond the rim's plane may change sides"""
    from sobfu_amd.evaluate import compare_meshes

    bv, bf = MP.icosphere(RADIUS, 4, (0.0, 0.0, -0.75))
    cv, cf = _gt(0, True)
    av = bv.copy()
    av[:, 1] += np.float32(0.3 * RADIUS)
    closed = compare_meshes(av, bf, bv, bf, signed=True)
    closed_w = compare_meshes(av, bf, bv, bf, signed="winding")
    capped = compare_meshes(av, bf, cv, cf, signed="winding")
    rim = float(cv[np.unique(MW.boundary_chain(cf, len(cv))[:, :2]), 0].min())
    beyond = int((av[:, 0] > rim).sum())
    n, i_closed, i_capped = closed["a_to_b"]["n"], closed["a_to_b"]["inside"], capped["a_to_b"]["inside"]
    print("a_to_b inside: %d of %d against the closed sphere, %d against the capped one; %d vertices beyond the rim's plane x = %.4f; open %d"
          % (i_closed, n, i_capped, beyond, rim, capped["a_to_b"]["open"]))
    assert closed_w["a_to_b"] == closed["a_to_b"] and closed_w["b_to_a"] == closed["b_to_a"]  # closed meshes: one answer
    assert 0.3 * n < i_closed < 0.6 * n and 0 < i_closed - i_capped <= beyond < 0.15 * n
    assert capped["a_to_b"]["open"] > 0 and closed["a_to_b"]["open"] == 0
    assert set(capped["a_to_b"]) == set(closed["a_to_b"])


def test_app_mesh_sign_winding(tmp_path):
    """sobfu_headless --voxelise-mesh on two written .ply files of the capped icosphere: refused with the default sign, fused with
    --mesh-sign winding through the C++ shells (TriangleGrid::boundary / voxelise / winding) and scored with signs against the closed
    ground truth; an unknown rule ends the run"""
    import re
    import subprocess

    from sobfu_amd import build, build_host, mesh_io

    build.build_hip()
    exe = build_host.build_app()
    for n in range(FRAMES):
        for name, capped in (("gt", False), ("open", True)):
            v, f = _gt(n, capped)
            nrm = v.copy()
            nrm[:, :3] = (v[:, :3] - np.array([SHIFT * n, 0, -0.75], np.float32)) / np.float32(RADIUS)
            mesh_io.write_ply(tmp_path / ("%s_%06d.ply" % (name, n)), v, nrm, f)
    gt, opened = str(tmp_path / "gt_%06d.ply"), str(tmp_path / "open_%06d.ply")
    line = re.compile(r"^evaluate live (\d+): (.*)$", re.M)

    def run(*args):
        r = subprocess.run([exe, CONFIG1, "--no-stats", *args], capture_output=True, text=True, timeout=600)
        return r.returncode, r.stdout + r.stderr

    rc, out = run("--voxelise-mesh", opened)
    assert rc == 2 and "not closed" in out
    rc, out = run("--voxelise-mesh", opened, "--mesh-sign", "winding", "--evaluate-live", gt, "--evaluate-signed")
    assert rc == 0, out[-3000:]
    lines = line.findall(out)
    print("\n".join("evaluate live %s: %s" % l for l in lines))
    assert [int(n) for n, _ in lines] == [1]
    got = dict(kv.split("=") for kv in lines[0][1].split())
    assert int(got["a_to_b.within"]) == int(got["a_to_b.n"]) > 100 and int(got["a_to_b.open"]) == 0  # the ground truth scored against is closed
    assert 0 < int(got["a_to_b.inside"]) < int(got["a_to_b.within"]) and float(got["a_to_b.rms"]) < 0.005
    rc, out = run("--voxelise-mesh", gt, "--mesh-sign", "odd")
    assert rc == 2 and "parity or winding" in out
