"""The cases of tests/test_gpu_mc_edges.py, checked on the CPU with the oracle and the numpy restatement alone (tests/mc_cases.py,
tests/mc_indexed_reference.py): every case reaches the code it claims to reach (the second slab of scan_blocks, both sides of a chunk
seam, the degenerate decisions), the two references agree with each other, `plane` agrees with its float64 closed form, and the bounds
written into mc_cases.py are the ones measured here.  Run with -s to see the figures."""
import numpy as np
import pytest

import mc_cases as K
import mc_indexed_reference as MI


def _active_set(vol):
    return np.nonzero(MI.classify(vol)[1].reshape(-1))[0]


@pytest.mark.parametrize("name", K.VOLUME_CASES)
def test_references_agree_and_chunk_claims(name):
    vol, size, R, t = K.case(name)
    r = K.reference(name)
    m, idx = r["indexed"], r["occ"][0].astype(np.int64)
    X, Y, Z = K.dims_of(vol)
    N = X * Y * Z
    assert vol.nbytes < 20e6
    # the oracle's soup has exactly three vertices per face of the restatement's mesh, and the same active cells
    assert r["count"] == m["active"] and np.array_equal(idx, _active_set(vol)) and np.all(np.diff(idx) > 0)
    assert r["total"] == len(r["soup_v"]) == 3 * len(m["faces"]) == int(r["occ"][1].sum())
    assert np.array_equal(r["occ"][2], np.cumsum(r["occ"][1]) - r["occ"][1])
    ch = K.chunk_of(idx)
    late = int((ch >= K.SLAB).sum())
    print(f"\n{name}: {r['count']} active cells of {N} in chunks {ch.min() if len(ch) else '-'}..{ch.max() if len(ch) else '-'} of "
          f"{-(-N // K.CHUNK)}, {late} in chunks >= {K.SLAB}; {len(m['vertices'])} welded vertices, {len(m['faces'])} faces")
    if name == "carry":
        assert (N, -(-N // K.CHUNK)) == (2_293_760, 1120) and -(-N // K.CHUNK) > K.SLAB  # two slabs of scan_blocks
        assert (r["count"], int(ch.min()), int(ch.max()), late) == (46_735, 0, 1116, 3_936)
        # the carry matters to all three scanned arrays: cells, soup vertices and welded vertices exist on both sides of chunk 1024
        own = K.chunk_of(K.vertex_owners(m["mask"])[0])
        assert (own < K.SLAB).any() and (own >= K.SLAB).any() and int(r["occ"][1][ch < K.SLAB].sum()) > 0
    elif name in K.FLAT_CASES:
        assert r["count"] == 0 and len(m["vertices"]) == 0 and len(r["soup_v"]) == 0
    elif name.startswith("tiny_"):
        assert r["count"] >= 1 and (r["count"] == 1) == (name == "tiny_2x2x2")
    elif name in K.SEAM_CASES and N > K.CHUNK + 1:
        assert N < 2 * K.CHUNK or (X, Y, Z) == (2050, 2, 2)  # two chunks, the second nearly empty; or one row of cells across the seam
        mask = m["mask"].reshape(-1)
        cells = [K.seam_owner_cell(i, (X, Y, Z)) for i in (K.CHUNK - 1, K.CHUNK)]
        if name.endswith("_own"):
            # voxels 2047 and 2048 each own a vertex on their +x edge, used by an active cell: the one on voxel 2048 from chunk 0
            assert mask[K.CHUNK - 1] & 1 and mask[K.CHUNK] & 1 and all(c in idx for c in cells)
            assert (cells == [K.CHUNK - 1, K.CHUNK]) == ((X, Y, Z) in K.SEAM_CELLS)
            if (X, Y, Z) not in K.SEAM_CELLS:
                assert cells[1] < K.CHUNK
        else:
            assert vol.reshape(-1, 2)[K.CHUNK, 1] == 0
            lost = np.setdiff1d(K.reference(name.replace("_unobs", "_own"))["occ"][0], idx)
            assert len(lost) >= 2 and (lost < K.CHUNK).any() and cells[0] in lost  # cells of chunk 0 silenced by a corner in chunk 1
            assert np.setdiff1d(idx, K.reference(name.replace("_unobs", "_own"))["occ"][0]).size == 0
    elif name in K.SEAM_CASES:
        assert N == K.CHUNK and r["count"] > 100  # one chunk, full to its last lane


def test_seam_dims_sit_next_to_the_tile_sizes():
    n = sorted(d[0] * d[1] * d[2] for d in K.SEAM_DIMS)
    assert n == [2048, 2050, 2176, 2295, 2313, 2700, 8200]
    assert 2176 == 2048 + 128 and 2295 == 9 * 255 and 2313 == 9 * 257  # x rows of 255 / 257: a wave and a workgroup straddle rows
    for dims in K.SEAM_CELLS:  # voxels 2047 and 2048 are cells, neighbours in one x row
        x, y, z = K.coords(K.CHUNK - 1, dims)
        assert x + 2 < dims[0] and y + 1 < dims[1] and z + 1 < dims[2]


def test_plane_against_float64():
    vol, size, R, t = K.case("plane")
    r = K.reference("plane")
    m = r["indexed"]
    f = vol[..., 0]
    # crossing cells stay unclipped: the reference of this case is the plane itself
    nv = MI.classify(vol)[1]
    z, y, x = np.nonzero(nv)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                assert np.abs(f[z + dz, y + dy, x + dx]).max() < 0.5
    assert r["count"] == 731
    res = max(K.plane_residual(r["soup_v"]), K.plane_residual(m["vertices"]))
    nerr = K.plane_indexed_normal_error(m["normals"])
    serr, finite = K.plane_soup_normal_error(r["soup_n"])
    print(f"\nplane: residual {res:.3e} grid units, indexed normals {nerr:.3e}, soup normals {serr:.3e} over {finite} of {len(r['soup_n'])}")
    for got, written in ((res, K.PLANE_RESIDUAL_MEASURED), (nerr, K.PLANE_NORMAL_MEASURED), (serr, K.PLANE_SOUP_NORMAL_MEASURED)):
        assert 0.9 * written <= got <= written, (got, written)  # what is written there is what is measured here
    assert K.PLANE_RESIDUAL_BOUND == 4 * K.PLANE_RESIDUAL_MEASURED < 1e-5  # far below anything a misplaced half cell (0.5) would give
    assert K.PLANE_NORMAL_BOUND == 4 * K.PLANE_NORMAL_MEASURED and K.PLANE_SOUP_NORMAL_BOUND == 4 * K.PLANE_SOUP_NORMAL_MEASURED
    assert finite > 0.95 * len(r["soup_n"])  # one sign: an error near 2 would be a normal that points the other way
    # the winding, in float64 on the un-posed vertices: soup cross(v3 - v1, v2 - v1) and the faces' cross(p1 - p0, p2 - p0) both point up
    # the gradient, towards positive TSDF
    g = K.plane_unit_normal()
    p = K.unpose(r["soup_v"], R, t).reshape(-1, 3, 3)
    c = np.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0])
    area = np.linalg.norm(c, axis=1)
    big = area > 1e-3 * area.max()
    assert big.sum() > 1000 and np.all((c[big] @ g) / area[big] > 1 - 1e-6)
    q = K.unpose(m["vertices"], R, t)[m["faces"]]
    c = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    assert np.all((c[big] @ g) / np.linalg.norm(c[big], axis=1) > 1 - 1e-6)


def test_the_closed_form_rejects_a_lost_half_cell_and_a_lost_flip():
    vol, size, R, t = K.case("plane")
    v = K.reference("plane")["soup_v"]
    cs = K.cell_sizes(size, K.PLANE_DIMS)
    shifted = v.copy()
    shifted[:, :3] = ((K.unpose(v, R, t) - 0.5 * cs) @ np.asarray(R, np.float64).T + t) * K.FLIP  # nodes at x cs, not (x + 0.5) cs
    assert K.plane_residual(shifted) > 0.1
    unflipped = v.copy()
    unflipped[:, 1:3] *= -1
    assert K.plane_residual(unflipped) > 1


def test_soup_against_indexed():
    worst = {}
    for name in K.VOLUME_CASES:
        r = K.reference(name)
        m = r["indexed"]
        keep = K.weld_keep(name)
        worst[name] = K.weld_error_ulps(r["soup_v"], m["vertices"], m["faces"], keep)
        print(f"\n{name}: soup against indexed {worst[name]:.3f} ulps of the largest coordinate ({int((~keep).sum())} of {len(keep)} vertices set aside)")
        if name not in ("degenerate", "degenerate_nan"):
            assert keep.all()
    assert max(worst.values()) == K.WELD_ULPS_MEASURED and K.WELD_ULPS_BOUND == 2 * K.WELD_ULPS_MEASURED
    assert worst["plane"] == 1.0 and worst["carry"] == 1.0
    # the edges set aside: with |fb - fa| far below the 1e-15f of interp each walk stays at its own end -- a whole cell apart
    r, keep = K.reference("degenerate"), K.weld_keep("degenerate")
    assert 10 < (~keep).sum() < keep.sum()
    assert K.weld_error_ulps(r["soup_v"], r["indexed"]["vertices"], r["indexed"]["faces"], ~keep) >= 2 ** 20


def test_degenerate_values_decide():
    vol, size, R, t = K.case("degenerate")
    r = K.reference("degenerate")
    m = r["indexed"]
    f = vol[..., 0]
    tiny = np.finfo(np.float32).tiny
    for v in K.DEGENERATE_VALUES:
        assert (f.view(np.uint32) == np.float32(v).view(np.uint32)).sum() > 20  # by bits: -0.0 and the subnormals are really there
    assert ((f != 0) & (np.abs(f) < tiny)).sum() > 50 and (vol[..., 1] == 0).sum() > 5
    # each rule changes the active cells when it is bent: f <= 0 for f < 0, and subnormals flushed to zero
    base = _active_set(vol)
    le = vol.copy()
    le[..., 0] = np.where(f == 0, np.float32(-1), f)
    ftz = vol.copy()
    ftz[..., 0] = np.where(np.abs(f) < tiny, np.float32(0), f)
    assert not np.array_equal(_active_set(le), base) and not np.array_equal(_active_set(ftz), base)
    assert np.array_equal(r["occ"][0], base)  # the oracle and the restatement agree on the active cells
    # wherever an end of a cut edge holds 0.0 or -0.0 the vertex lies exactly on a grid node (unit cells, identity pose), in both meshes
    fa, fb = K.vertex_edge_values("degenerate")
    zero = (fa == 0) | (fb == 0)
    assert zero.sum() > 50
    on_node = lambda p: np.all((p[..., :3] * K.FLIP.astype(np.float32) - np.float32(0.5)) % 1 == 0, axis=-1)
    assert on_node(m["vertices"][zero]).all() and not on_node(m["vertices"][np.abs(fa - fb) == 1.5]).any()  # t = 1/3 or 2/3
    corners = m["faces"][:, [0, 2, 1]]
    assert on_node(r["soup_v"].reshape(-1, 3, 4)[zero[corners]]).all()
    # the other decisions are present: zero gradients (len2 > 0), degenerate triangles (NaN soup normals), no non-finite vertex
    assert (np.abs(m["normals"][:, :3]).max(1) == 0).sum() >= 10 and np.isnan(r["soup_n"]).any(1).sum() >= 100
    assert np.isfinite(r["soup_v"]).all() and np.isfinite(m["vertices"]).all() and np.isfinite(m["normals"]).all()
    print(f"\ndegenerate: {r['count']} active cells, {len(r['soup_v']) // 3} triangles, {int(np.isnan(r['soup_n']).any(1).sum())} rows with NaN "
          f"normals, {len(m['vertices'])} welded vertices, {int((np.abs(m['normals'][:, :3]).max(1) == 0).sum())} zero normals")


def test_nan_volume():
    vol = K.case("degenerate_nan")[0]
    r = K.reference("degenerate_nan")
    m = r["indexed"]
    assert 5 < np.isnan(vol[..., 0]).sum() < 30
    assert np.array_equal(r["occ"][0], _active_set(vol))
    bad_s, bad_w = ~np.isfinite(r["soup_v"]).all(1), ~np.isfinite(m["vertices"]).all(1)
    assert 10 < bad_s.sum() < len(bad_s) // 4 and 3 < bad_w.sum() < len(bad_w) // 4  # a NaN is not negative: it sits on cut edges
    assert np.isfinite(m["normals"]).all()  # len2 > 0 is false for a NaN gradient: the normal is (0, 0, 0)
    # the same vertices are non-finite in both meshes
    assert np.array_equal(bad_w[m["faces"][:, [0, 2, 1]]].reshape(-1), bad_s)


def test_caps_and_offset_inputs():
    count, total = K.caps_counts()
    assert (count, total) == (14_326, 139_830) and total % 3 == 0
    assert K.caps_max_voxels() == (1, count - 1, count, count + 1) and K.caps_max_vertices() == (3, 4, 5, total - 1, total, total + 1)
    assert -(-count // K.CHUNK) == 7  # mc_offsets runs seven chunks on the uncapped count
    nbs = [-(-c // K.CHUNK) for c in K.OFFSET_COUNTS]
    assert nbs == [1] * 9 + [2, 3, 1024, 1024, 1025]  # one chunk, two, and scan_blocks' second slab by exactly one chunk sum
    for c in (1, 257, 2049):
        occ, want, tot = K.offsets_input(c)
        assert occ.shape == (3, c + K.OFFSET_PAD) and set(np.unique(occ[1, :c])) <= {3, 6, 9, 12, 15}
        assert want[0] == 0 and tot == int(occ[1, :c].sum()) and np.all(occ[1, c:] == K.OFFSET_BEYOND) and np.all(occ[[0, 2]] == K.OFFSET_SENTINEL)
    assert K.offsets_input(K.OFFSET_COUNTS[-1])[2] < 2 ** 31
