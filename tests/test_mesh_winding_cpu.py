"""Generalised winding numbers from the boundary, on the CPU: the C ABI's entry points (exported, ABI version unchanged,
argument checks before any device call, the host-only boundary chain), the numpy restatement tests/mesh_winding_reference.py against the
headers themselves as a host compiler takes them (sobfu_amd/csrc/sobfu_mesh_winding.hpp, sobfu_mesh_boundary.hpp), the restatement's
boundary formula against its own definition on lattice-aligned cubes (ties and seams included), and the same cases through a build of the
tool with the address and undefined-behaviour sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_parity_reference as MP
import mesh_winding_reference as MW

F3, I3 = C.c_float * 3, C.c_int * 3
A, B, D, E, G, H, K = (C.c_void_p(4096 * k) for k in range(1, 8))  # 16-byte aligned addresses that are never dereferenced
VS = 1.0 / 64
DIMS = (20, 12, 9)
IDX = ((4, 15), (3, 8), (2, 6))  # the cube's corners on these voxel centres, as in tests/test_gpu_mesh_voxelise.py
LO, HI = [(i0 + 0.5) * VS for i0, _ in IDX], [(i1 + 0.5) * VS for _, i1 in IDX]
CASES = {"closed": None, "one face off": [2, 3], "two faces off": [2, 3, 6, 7]}  # +x; +x and +y


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_winding_tool()


@pytest.fixture(scope="module")
def sanitized_tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_winding_tool(flags=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], out="mesh_winding_tool_sanitized")


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_mesh_boundary", "sobfu_hip_mesh_winding", "sobfu_hip_mesh_voxelise_winding", "sobfu_hip_mesh_voxelise_winding_workspace_bytes"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


# ---- argument checks: every case is refused (or n = 0) before any device call ---------------------------------------------------------
def _winding(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), b=K, nb=3, p=E, n=4, w=G, mode=0, walk=0)
    a.update(kw)
    return lib.sobfu_hip_mesh_winding(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"],
                                      a["b"], a["nb"], a["p"], a["n"], a["w"], a["mode"], a["walk"], None)


def _voxelise(lib, **kw):
    a = dict(ws=D, ws_bytes=1 << 20, v=A, nv=8, f=B, nt=4, origin=F3(0, 0, 0), h=0.5, dims=I3(2, 2, 2), b=K, nb=3, vol=E, X=40, Y=8, Z=4,
             vs=F3(0.01, 0.01, 0.01), trunc=0.03, eta=0.01, mode=0, bits=G, bits_bytes=1 << 14, open_rows=H, winding=None)
    a.update(kw)
    return lib.sobfu_hip_mesh_voxelise_winding(a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]),
                                               a["dims"], a["b"], a["nb"], a["vol"], a["X"], a["Y"], a["Z"], a["vs"], C.c_float(a["trunc"]),
                                               C.c_float(a["eta"]), a["mode"], a["bits"], C.c_size_t(a["bits_bytes"]), a["open_rows"], a["winding"], None)


GRID_BAD = [dict(ws=None), dict(ws=C.c_void_p(4104)), dict(ws_bytes=16), dict(origin=None), dict(dims=None), dict(h=0.0), dict(h=float("nan")),
            dict(origin=F3(0, float("nan"), 0)), dict(dims=I3(0, 2, 2)), dict(dims=I3(2, 2, 129)), dict(v=None), dict(f=None),
            dict(v=C.c_void_p(4100)), dict(f=C.c_void_p(8194)), dict(nv=-1), dict(nt=-1)]
BOUNDARY_BAD = [dict(b=None), dict(b=C.c_void_p(K.value + 8)), dict(nb=-1)]
INF = float("inf")


@pytest.mark.parametrize("kw", GRID_BAD + BOUNDARY_BAD + [dict(p=None), dict(p=C.c_void_p(E.value + 8)), dict(w=None), dict(w=C.c_void_p(G.value + 2)), dict(n=-1),
                                                         dict(mode=-1), dict(mode=2), dict(walk=-1), dict(walk=3)])
def test_winding_bad_arguments(lib, kw):
    assert _winding(lib, **kw) == -1


WS_NEEDED = 4 * 2 * 8 * 4 + 16 + 40 * 8 * 4 * 4  # two words per row, the seam counter, one int per voxel


@pytest.mark.parametrize("kw", GRID_BAD + BOUNDARY_BAD + [dict(mode=-1), dict(mode=3), dict(vol=None), dict(vol=C.c_void_p(E.value + 4)), dict(X=0), dict(Y=0),
                                                         dict(Z=-1), dict(X=513), dict(vs=None), dict(vs=F3(0.01, 0, 0.01)),
                                                         dict(vs=F3(0.01, 0.01, float("nan"))), dict(trunc=0.0), dict(trunc=INF), dict(eta=float("nan")),
                                                         dict(bits=None), dict(bits=C.c_void_p(G.value + 4)), dict(bits_bytes=WS_NEEDED - 1),
                                                         dict(open_rows=None), dict(open_rows=C.c_void_p(H.value + 2)), dict(winding=C.c_void_p(K.value + 2))])
def test_voxelise_winding_bad_arguments(lib, kw):
    assert _voxelise(lib, **kw) == -1


def test_workspace_bytes_and_nothing_to_do(lib):
    wb = lib.sobfu_hip_mesh_voxelise_winding_workspace_bytes
    assert wb(40, 8, 4) == WS_NEEDED and wb(512, 3, 5) == 16 * 4 * 15 + 16 + 512 * 15 * 4 and wb(33, 1, 1) == 16 + 16 + 33 * 4
    assert wb(513, 3, 5) == 0 and wb(0, 3, 5) == 0 and wb(8, 0, 5) == 0 and wb(8, 3, -1) == 0 and wb(8, 1 << 16, 1 << 16) == 0
    assert _winding(lib, n=0) == 0 and _winding(lib, n=0, nb=0, b=None) == 0
    assert _winding(lib, n=0, ws=None) == -1 and _winding(lib, n=0, w=None) == -1  # the checks come first


# ---- the boundary chain ----------------------------------------------------------------------------------------------------------------
def _chain_tool(tool, tmp_path, faces, n_vertices):
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([len(f), n_vertices], np.int32).tobytes() + f.tobytes())
    subprocess.run([tool, "boundary", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    return bool(raw[0]), raw[2:].reshape(-1, 3)


def _chain_abi(lib, faces, n_vertices):
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    fp = f.ctypes.data_as(C.POINTER(C.c_int)) if len(f) else None
    count = C.c_int(-1)
    rc = lib.sobfu_hip_mesh_boundary(fp, len(f), n_vertices, None, 0, C.byref(count))
    if rc:
        return rc, None
    out = np.zeros((count.value, 3), np.int32)
    if count.value:
        assert lib.sobfu_hip_mesh_boundary(fp, len(f), n_vertices, out.ctypes.data_as(C.POINTER(C.c_int)), count.value - 1, C.byref(count)) == -3
        assert lib.sobfu_hip_mesh_boundary(fp, len(f), n_vertices, out.ctypes.data_as(C.POINTER(C.c_int)), count.value, C.byref(count)) == 0
    return 0, out


def _chains():
    """(what, faces, vertices, the chain's rows as a set or None for an error)"""
    tri, mirror = [(0, 1, 2)], [(0, 2, 1)]
    yield "closed cube", MP.cube(LO, HI)[1], 8, set()
    yield "cube, +x off", MP.cube(LO, HI, [2, 3])[1], 8, {(1, 3, -1), (1, 5, 1), (3, 7, -1), (5, 7, 1)}  # the diagonal 1-7 cancels
    yield "a triangle twice", tri + tri, 3, {(0, 1, 2), (1, 2, 2), (0, 2, -2)}
    yield "a triangle and its mirror image", tri + mirror, 3, set()
    yield "neighbours, one flipped", [(0, 1, 2), (1, 2, 3)], 4, {(0, 1, 1), (0, 2, -1), (1, 2, 2), (1, 3, -1), (2, 3, 1)}
    yield "neighbours, consistent", [(0, 1, 2), (2, 1, 3)], 4, {(0, 1, 1), (0, 2, -1), (1, 3, 1), (2, 3, -1)}
    yield "a bad index", [(0, 1, 3)], 3, None
    yield "a negative index", [(0, -1, 2)], 3, None
    yield "no faces", np.zeros((0, 3), np.int32), 5, set()
    yield "a repeated corner", [(0, 0, 1)], 2, set()  # 0 -> 0 has no direction; 0 -> 1 and 1 -> 0 cancel


def test_boundary_chain(lib, tool, tmp_path):
    for what, faces, nv, want in _chains():
        ok, got = _chain_tool(tool, tmp_path, faces, nv)
        rc, abi = _chain_abi(lib, faces, nv)
        if want is None:
            assert not ok and rc == -1, what
            with pytest.raises(ValueError):
                MW.boundary_chain(faces, nv)
            continue
        ref = MW.boundary_chain(faces, nv)
        print("%s: %d edges %s" % (what, len(got), got.tolist() if len(got) < 8 else ""))
        assert ok and rc == 0 and np.array_equal(got, ref) and np.array_equal(abi, ref), what
        assert {tuple(r) for r in got.tolist()} == want, what
        assert np.all(got[:, 0] < got[:, 1]) and np.all(got[:, 2] != 0)
        key = got[:, 0].astype(np.int64) * nv + got[:, 1]
        assert np.all(np.diff(key) > 0)  # sorted by (u, v), every edge once
    v, f = MW.capped_icosphere(0.1, 3, (0.0, 0.0, 0.5), 0.8)
    ok, got = _chain_tool(tool, tmp_path, f, len(v))
    assert ok and np.array_equal(got, MW.boundary_chain(f, len(v))) and len(got) > 10 and np.all(np.abs(got[:, 2]) == 1)
    # one closed loop: every boundary vertex on exactly two edges
    assert np.all(np.bincount(got[:, :2].ravel())[np.unique(got[:, :2])] == 2)


# ---- the headers through a host compiler -----------------------------------------------------------------------------------------------
def _run(tool, tmp_path, what, first, second):
    first, second = np.ascontiguousarray(first, np.float32), np.ascontiguousarray(second, np.float32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([len(first), len(second)], np.int32).tobytes() + first.tobytes() + second.tobytes())
    subprocess.run([tool, what, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=300)
    return np.fromfile(tmp_path / "out.bin", np.uint8)


def _few_ulp(got, want, what, ulps=4):
    err = np.abs(got - want) / np.spacing(np.maximum(np.abs(want), 1e-300))
    print("%s: %d values, max %.3g ulp, %d differ" % (what, got.size, float(err.max()), int((got != want).sum())))
    assert np.isfinite(got).all() and err.max() <= ulps, what


def _header_equals_restatement(tool, tmp_path, v, f, points, what):
    a, b, c = MP.corners(v, f)
    tris = np.concatenate([a, b, c], 1)
    n, T = len(points), len(tris)
    raw = _run(tool, tmp_path, "crossings", points[:, 1:3], tris)
    sign, X = raw[:n * T].view(np.int8).reshape(n, T), raw[n * T:].view(np.float64).reshape(n, T)
    want_sign, want_X = MW.signed_crossings(points[:, 1:3], v, f)
    assert np.array_equal(sign, want_sign), "%s: the sign differs at %d pairs" % (what, int((sign != want_sign).sum()))
    assert np.array_equal(X.view(np.uint64), want_X.view(np.uint64)), "%s: X differs" % what
    hit, Xp = MP.crossings(points[:, 1:3], v, f)  # signed_row_crossing with sign != 0
    assert np.array_equal(sign != 0, hit) and np.array_equal(X.view(np.uint64), Xp.view(np.uint64))
    got = _run(tool, tmp_path, "triangles", points[:, :3], tris).view(np.float64).reshape(n, T)
    q = points[:, None, :3].astype(np.float64)
    _few_ulp(got, MW.triangle_angle(a[None].astype(np.float64) - q, b[None].astype(np.float64) - q, c[None].astype(np.float64) - q), what + ", triangle angles")
    chain = MW.boundary_chain(f, len(v))
    if len(chain):
        uv = np.concatenate([v[chain[:, 0], :3], v[chain[:, 1], :3]], 1)
        got = _run(tool, tmp_path, "strips", points[:, :3], uv).view(np.float64).reshape(n, len(chain))
        _few_ulp(got, MW.strip_angle(points, uv[:, :3], uv[:, 3:]), what + ", strip angles")
        bv = v[np.unique(chain[:, :2]), :3]
        seams = _run(tool, tmp_path, "seams", points[:, :3], bv).reshape(n, len(bv)).any(1)
        assert np.array_equal(seams, MW.seam(points, v, chain)), what
        return int(seams.sum())
    return 0


def _cases():
    p = MP.voxel_centres(DIMS, (VS,) * 3).reshape(-1, 4)
    for name, drop in CASES.items():
        yield name, MP.cube(LO, HI, drop), p
    rng = np.random.default_rng(5)
    v, f = MW.capped_icosphere(0.1, 2, (0.01, -0.02, 0.5), 0.7, axis=0)
    yield "capped icosphere", (v, f), np.concatenate([rng.uniform(-0.15, 0.15, (300, 3)) + (0.01, -0.02, 0.5), v[::7, :3]]).astype(np.float32)
    _, v, f, lo, hi = MP.indexed_soup()
    yield "degenerate soup", (v, f[:120]), np.concatenate([rng.uniform(lo, hi, (200, 3)), v[f[:40, 0], :3]]).astype(np.float32)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_headers_on_the_cpu_equal_the_restatement(which, tool, sanitized_tool, tmp_path):
    """signed crossings bit for bit (sign and X), strip and triangle angles within 4 ulp (atan2 is libm's on both sides), the seam
    predicate exactly; the second round runs the same cases through the tool built with -fsanitize=address,undefined"""
    seams = {}
    for name, (v, f), p in _cases():
        seams[name] = _header_equals_restatement(sanitized_tool if which == "sanitized" else tool, tmp_path, v, f, p, name)
    print(seams)
    assert seams["closed"] == 0 and seams["one face off"] > 0 and seams["two faces off"] > 0


def test_the_boundary_formula_equals_the_definition_on_lattice_cubes():
    """corners on voxel centres: rows through vertices and along edges (parity_sign ties), centres on the strips' planes and on seams.
    <= 1e-12 at every centre off the mesh, the seam points through the definition; without that fallback they are off by up to 3 / 4"""
    p = MP.voxel_centres(DIMS, (VS,) * 3).reshape(-1, 4)
    off = MP.box_sdf(p[:, :3], LO, HI) != 0  # off the closed cube's surface, so off every sub-mesh
    for name, drop in CASES.items():
        v, f = MP.cube(LO, HI, drop)
        N, open_rows = MW.crossings_beyond_centres(v, f, DIMS, (VS,) * 3)
        assert np.array_equal(N.reshape(-1), MW.crossings_beyond(p, v, f)), name  # the row kernel's counters = the point kernel's count
        w, seam = MW.winding_boundary(p, v, f, return_seam=True, N=N)
        want = MW.winding_sum(p, v, f)
        chain = MW.boundary_chain(f, len(v))
        raw = N.reshape(-1).astype(np.float64)
        if len(chain):
            raw = raw + (MW.strip_angle(p, v[chain[:, 0], :3], v[chain[:, 1], :3]) * chain[:, 2]).sum(1) / MW.FOUR_PI
        err, raw_err = np.abs(w - want)[off], np.abs(raw - want)[off]
        print("%s: %d edges, %d open rows, %d seam points, max |boundary - definition| %.3g (%.3g without the fallback, %d points beyond 1e-12, all seams: %s), min |w - 1/2| %.4f"
              % (name, len(chain), open_rows, int(seam.sum()), err.max(), raw_err.max(), int((raw_err > 1e-12).sum()), bool(seam[off][raw_err > 1e-12].all()),
                 np.abs(want[off] - 0.5).min()))
        assert err.max() <= 1e-12, name
        assert seam[off][raw_err > 1e-12].all(), name  # no failure off a seam
        if drop is None:
            ins, _ = MP.inside(p, v, f)
            assert len(chain) == 0 and not seam.any() and np.array_equal(w, ins.astype(np.float64)) and open_rows == 0
        else:
            assert (seam & off).sum() > 0 and (raw_err > 1e-12).sum() > 0 and open_rows > 0, name  # the fallback is exercised, and needed
    assert abs(np.abs(want[off] - 0.5).min() - 0.0138) < 1e-3  # two faces off: no centre near the 1/2 level
