"""Marching cubes and its scan on the GPU at their edges (sobfu_amd/csrc/mc_kernels.hip, sobfu_amd/csrc/sobfu_scan.hpp): the cases of
tests/mc_cases.py -- shown meaningful on the CPU by tests/test_mc_cases_cpu.py -- against the oracle (soup) and the numpy restatement
(indexed), bit for bit; mc_offsets on synthetic counts at the sizes where the scan changes regime; the caps, with sentinels behind
every buffer."""
import ctypes as C

import numpy as np
import pytest

import mc_cases as K
import mc_indexed_reference as MI

pytestmark = pytest.mark.gpu
POISON = 0xA5  # workspaces start out dirty: nothing may rely on what a workspace held before the call


def _np(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, nan=False):
    """bit for bit; in a volume with NaNs by value, NaN == NaN (a NaN's sign and payload differ between the host and the device)"""
    got = _np(got) if not isinstance(got, np.ndarray) else got
    if got.shape != want.shape:
        return False
    return np.array_equal(got, want, equal_nan=True) if nan else np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _dirty(n):
    import torch

    return torch.full((int(n),), POISON, dtype=torch.uint8, device="cuda")


def _count_call(d, ws):
    import torch

    from sobfu_amd import _lib, ops

    a, nv, nt = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().sobfu_hip_mc_indexed_count(stream, C.c_void_p(d.data_ptr()), *ops._xyz(d), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()),
                                               C.byref(a), C.byref(nv), C.byref(nt))
    assert rc == 0
    return a.value, nv.value, nt.value


@pytest.mark.parametrize("name", K.VOLUME_CASES)
def test_volume_case_matches_the_references(name):
    import torch

    from sobfu_amd import ops

    vol, size, R, t = K.case(name)
    r = K.reference(name)
    m = r["indexed"]
    nan = name in K.NAN_CASES
    d = torch.from_numpy(vol.copy()).cuda()
    mv, mx = r["count"] + 3, r["total"] + 3  # just above the counts: the default caps allocate 200 MB of output per call
    ws = _dirty(ops.mc_workspace(d).numel())
    # the three steps of the soup path: with a kept workspace (twice) and with none
    for w in (ws, ws, None):
        occ, count = ops.mc_occupied_voxels(d, mv, w)
        assert count == r["count"]
        assert ops.mc_offsets(occ, count, w) == r["total"]
        occ = _np(occ)
        assert np.array_equal(occ[:, :count], r["occ"]) and np.all(occ[:, count:] == 0)
    soups = [ops.marching_cubes(d, size, R, t, max_voxels=mv, max_vertices=mx, workspace=w) for w in (ws, ws, None)]
    for sv, sn in soups:
        assert _same(sv, r["soup_v"], nan) and np.array_equal(_np(sn), r["soup_n"], equal_nan=True)
        assert _same(sv, _np(soups[0][0])) and _same(sn, _np(soups[0][1]))  # run to run by bits, NaNs included
    # the indexed path
    wsi = _dirty(ops.mc_indexed_workspace(d).numel())
    meshes = [ops.marching_cubes_indexed(d, size, R, t, workspace=w) for w in (wsi, wsi, None)]
    for v, n, f in meshes:
        assert f.dtype == torch.int32 and f.shape == m["faces"].shape
        assert _same(v, m["vertices"], nan) and np.array_equal(_np(f), m["faces"])
        n_ = _np(n)
        assert n_.shape == m["normals"].shape and np.isfinite(n_).all()
        assert np.abs(n_ - m["normals"]).max(initial=0) <= 2e-6
        assert _same(v, _np(meshes[0][0])) and _same(n, _np(meshes[0][1])) and torch.equal(f, meshes[0][2])
    assert _count_call(d, wsi) == (m["active"], len(m["vertices"]), len(m["faces"]))
    # the bounds measured on the references hold on the device's own outputs, with no further margin
    sv, (v, n, f) = _np(soups[0][0]), [_np(a) for a in meshes[0]]
    assert K.weld_error_ulps(sv, v, f, K.weld_keep(name)) <= K.WELD_ULPS_BOUND
    if name == "plane":
        assert K.plane_residual(sv) <= K.PLANE_RESIDUAL_BOUND and K.plane_residual(v) <= K.PLANE_RESIDUAL_BOUND
        assert K.plane_indexed_normal_error(n) <= K.PLANE_NORMAL_BOUND
        err, finite = K.plane_soup_normal_error(_np(soups[0][1]))
        assert err <= K.PLANE_SOUP_NORMAL_BOUND and finite == K.plane_soup_normal_error(r["soup_n"])[1]


def test_carry_indexed_generate_refuses_a_short_buffer():
    """the never-truncate contract where the totals come from the second slab of scan_blocks3_kernel"""
    import torch

    from sobfu_amd import _lib, ops

    vol, size, R, t = K.case("carry")
    m = K.reference("carry")["indexed"]
    d = torch.from_numpy(vol.copy()).cuda()
    ws = _dirty(ops.mc_indexed_workspace(d).numel())
    a, nv, nt = _count_call(d, ws)
    assert (a, nv, nt) == (m["active"], len(m["vertices"]), len(m["faces"]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    R9, t3 = (C.c_float * 9)(*np.asarray(R, np.float32).reshape(9).tolist()), (C.c_float * 3)(*np.asarray(t, np.float32).tolist())
    bv = torch.full((nv, 4), 7.0, dtype=torch.float32, device="cuda")
    bn = torch.full_like(bv, 7.0)
    bf = torch.full((nt, 3), -5, dtype=torch.int32, device="cuda")
    for mv, mt in ((nv - 1, nt), (nv, nt - 1)):
        rc = _lib.lib().sobfu_hip_mc_indexed_generate(stream, C.c_void_p(d.data_ptr()), *ops._xyz(d), *[C.c_float(s) for s in size], R9, t3,
                                                      C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), C.c_void_p(bv.data_ptr()),
                                                      C.c_void_p(bn.data_ptr()), C.c_int(mv), C.c_void_p(bf.data_ptr()), C.c_int(mt))
        assert rc == -1, (mv, mt, rc)
    torch.cuda.synchronize()
    assert bool((bv == 7).all()) and bool((bn == 7).all()) and bool((bf == -5).all())


# ---- mc_offsets on synthetic counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", K.OFFSET_COUNTS)
def test_mc_offsets_at_count_boundaries(count):
    import torch

    from sobfu_amd import ops

    occ, want, total = K.offsets_input(count)
    need, guard = (-(-count // K.CHUNK) + 1) * 4, 64
    for kind in ("caller", "none", "short"):
        d = torch.from_numpy(occ).cuda()
        buf = _dirty(need + guard)
        ws = {"caller": buf[:need], "none": None, "short": buf[:16]}[kind]
        assert ops.mc_offsets(d, count, ws) == total, kind
        got, buf = _np(d), _np(buf)
        assert np.array_equal(got[2, :count], want), kind
        assert np.array_equal(got[:2], occ[:2]) and np.all(got[2, count:] == K.OFFSET_SENTINEL), kind  # rows 0, 1 and the tail untouched
        assert np.all(buf[need:] == POISON), kind  # nothing behind the workspace
        if kind == "short" and need > 16:
            assert np.all(buf == POISON)  # too small: left alone, the scratch is the call's own


# ---- caps -----------------------------------------------------------------------------------------------------------------------------
def _occupied(d, stride, max_size, fill=-7):
    import torch

    from sobfu_amd import _lib, ops

    occ = torch.full((3, stride), fill, dtype=torch.int32, device="cuda")
    n = C.c_int(-1)
    rc = _lib.lib().sobfu_hip_mc_occupied_voxels(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(d.data_ptr()), *ops._xyz(d),
                                                 C.c_void_p(occ.data_ptr()), C.c_int(stride), C.c_int(max_size), C.byref(n), None, C.c_size_t(0))
    assert rc == 0
    return occ, n.value


def _max_voxels_ids():
    return ["one", "count-1", "count", "count+1"]


@pytest.mark.parametrize("which", range(4), ids=_max_voxels_ids())
def test_max_voxels_cap_and_wide_stride(which):
    """count = min(found, max_size), the first max_size cells in index order, a stride wider than max_size, nothing written past the cap"""
    import torch

    from sobfu_amd import ops

    found, _ = K.caps_counts()
    mv = K.caps_max_voxels()[which]
    ref = K.caps_reference(mv)
    d = torch.from_numpy(K.caps_volume().copy()).cuda()
    stride = mv + K.CAPS_EXTRA_STRIDE
    occ, count = _occupied(d, stride, mv)
    assert count == min(found, mv) == ref["count"]
    got = _np(occ)
    assert np.array_equal(got[:2, :count], ref["occ"][:2])
    assert np.all(got[:2, count:] == -7) and np.all(got[2] == -7)  # rows 0 and 1 past the cap, and all of row 2, keep the sentinel
    assert ops.mc_offsets(occ, count) == ref["total"]
    got = _np(occ)
    assert np.array_equal(got[:, :count], ref["occ"]) and np.all(got[:, count:] == -7)
    total = ref["total"]
    v = torch.full((total + 8, 4), 7.0, dtype=torch.float32, device="cuda")
    n = torch.full_like(v, 7.0)
    ops.mc_generate_triangles(d, occ, count, MI.SIZE, MI.POSE_R, MI.POSE_T, v[:total], n[:total])
    assert _same(v[:total], ref["soup_v"]) and np.array_equal(_np(n[:total]), ref["soup_n"], equal_nan=True)
    assert bool((v[total:] == 7).all()) and bool((n[total:] == 7).all())
    sv, sn = ops.marching_cubes(d, MI.SIZE, MI.POSE_R, MI.POSE_T, max_voxels=mv, max_vertices=total + 3)
    assert _same(sv, ref["soup_v"]) and np.array_equal(_np(sn), ref["soup_n"], equal_nan=True)


@pytest.mark.parametrize("which", range(6), ids=["3", "4", "5", "total-1", "total", "total+1"])
def test_max_vertices_cap_keeps_whole_triangles(which):
    import torch

    from sobfu_amd import ops

    found, total = K.caps_counts()
    mx = K.caps_max_vertices()[which]
    whole = min(mx // 3 * 3, total)
    ref = K.caps_reference(found + 1, mx)
    assert len(ref["soup_v"]) == whole
    d = torch.from_numpy(K.caps_volume().copy()).cuda()
    occ, count = ops.mc_occupied_voxels(d, found + 1)
    assert count == found and ops.mc_offsets(occ, count) == total
    v = torch.full((mx + 8, 4), 7.0, dtype=torch.float32, device="cuda")
    n = torch.full_like(v, 7.0)
    ops.mc_generate_triangles(d, occ, count, MI.SIZE, MI.POSE_R, MI.POSE_T, v[:mx], n[:mx])
    assert _same(v[:whole], ref["soup_v"]) and np.array_equal(_np(n[:whole]), ref["soup_n"], equal_nan=True)
    assert bool((v[whole:] == 7).all()) and bool((n[whole:] == 7).all())  # the cut triangle's slots and everything behind the buffer
    sv, sn = ops.marching_cubes(d, MI.SIZE, MI.POSE_R, MI.POSE_T, max_voxels=found + 1, max_vertices=mx)
    assert _same(sv, ref["soup_v"]) and np.array_equal(_np(sn), ref["soup_n"], equal_nan=True)
