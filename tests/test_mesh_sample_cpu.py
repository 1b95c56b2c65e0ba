"""Area-weighted mesh sampling on the CPU: the C ABI's entry points (exported, ABI version unchanged, every argument check
before any device call), the numpy restatement tests/mesh_sample_reference.py against the header itself as a host compiler takes it
(sobfu_amd/csrc/sobfu_mesh_sample.hpp) bit for bit, the same cases through a build of the tool with the address and undefined-behaviour
sanitizers, and the properties of the restatement -- which the GPU shares, because tests/test_gpu_mesh_sample.py holds it to the
restatement bit for bit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mesh_sample_reference as MS

A, B, D, E, G, H, K = (C.c_void_p(4096 * k) for k in range(1, 8))  # 16-byte aligned addresses that are never dereferenced
SEEDS, cases, same_bits = MS.SEEDS, MS.cases, MS.same_bits


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_sample_tool()


@pytest.fixture(scope="module")
def sanitized_tool():
    from sobfu_amd import build_host

    return build_host.build_mesh_sample_tool(flags=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], out="mesh_sample_tool_sanitized")


def test_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_mesh_sample_workspace_bytes", "sobfu_hip_mesh_sample_count", "sobfu_hip_mesh_sample_generate", "sobfu_hip_distance_score"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


def test_workspace_bytes(lib):
    wb = lib.sobfu_hip_mesh_sample_workspace_bytes
    # a header of 16 ints, T + 1 counts, T + 1 offsets, one block sum per 2048 counts and the total
    assert wb(0) == 4 * (16 + 2 + 2) and wb(12) == 4 * (16 + 26 + 2) and wb(2047) == 4 * (16 + 4096 + 2) and wb(2048) == 4 * (16 + 4098 + 3)
    assert wb(-1) == 0


# ---- argument checks: every case is refused before any device call ---------------------------------------------------------------------
def _count(lib, **kw):
    total = C.c_longlong(-7)
    a = dict(v=A, nv=8, f=B, nt=4, density=10.0, seed=0, ws=D, ws_bytes=1 << 12, areas=E, total=C.byref(total))
    a.update(kw)
    return lib.sobfu_hip_mesh_sample_count(a["v"], a["nv"], a["f"], a["nt"], C.c_double(a["density"]), C.c_uint64(a["seed"]), a["ws"], C.c_size_t(a["ws_bytes"]),
                                           a["areas"], a["total"], None)


def _generate(lib, **kw):
    a = dict(v=A, nv=8, f=B, nt=4, seed=0, ws=D, ws_bytes=1 << 12, p=E, tri=G, bary=H, max_samples=100)
    a.update(kw)
    return lib.sobfu_hip_mesh_sample_generate(a["v"], a["nv"], a["f"], a["nt"], C.c_uint64(a["seed"]), a["ws"], C.c_size_t(a["ws_bytes"]), a["p"], a["tri"],
                                              a["bary"], a["max_samples"], None)


def _score(lib, **kw):
    a = dict(d=A, n=10, th=(C.c_float * 16)(*([0.1] * 16)), k=2, counts=B)
    a.update(kw)
    return lib.sobfu_hip_distance_score(a["d"], a["n"], a["th"], a["k"], a["counts"], None)


MESH_BAD = [dict(v=None), dict(f=None), dict(v=C.c_void_p(4100)), dict(f=C.c_void_p(8194)), dict(nv=-1), dict(nt=-1)]
WS_NEEDED = 4 * (16 + 2 * 5 + 2)
WS_BAD = [dict(ws=None), dict(ws=C.c_void_p(D.value + 8)), dict(ws_bytes=WS_NEEDED - 1), dict(ws_bytes=0)]


@pytest.mark.parametrize("kw", MESH_BAD + WS_BAD + [dict(density=-1.0), dict(density=float("nan")), dict(density=float("inf")), dict(density=-0.5e-300),
                                                   dict(areas=C.c_void_p(E.value + 4)), dict(total=None)])
def test_count_bad_arguments(lib, kw):
    assert _count(lib, **kw) == -1


@pytest.mark.parametrize("kw", MESH_BAD + WS_BAD + [dict(p=None), dict(p=C.c_void_p(E.value + 8)), dict(tri=C.c_void_p(G.value + 2)), dict(bary=C.c_void_p(H.value + 4)),
                                                   dict(max_samples=-1)])
def test_generate_bad_arguments(lib, kw):
    assert _generate(lib, **kw) == -1


@pytest.mark.parametrize("kw", [dict(d=None), dict(d=C.c_void_p(A.value + 2)), dict(n=-1), dict(th=None), dict(k=0), dict(k=17), dict(k=-1), dict(counts=None),
                                dict(counts=C.c_void_p(B.value + 4))])
def test_score_bad_arguments(lib, kw):
    assert _score(lib, **kw) == -1


# ---- the header through a host compiler ------------------------------------------------------------------------------------------------
def _run(tool, tmp_path, v, f, density, seed):
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([len(v), len(f)], np.int32).tobytes() + np.array([density], np.float64).tobytes() + np.array([seed], np.uint64).tobytes() +
                 v.tobytes() + f.tobytes())
    r = subprocess.run([tool, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=300)
    if r.returncode:
        return r.returncode, None
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    T, at = len(f), 0

    def take(dtype, count):
        nonlocal at
        out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += out.nbytes
        return out

    areas, counts = take(np.float64, T), take(np.int64, T)
    N = int(take(np.int64, 1)[0])
    out = dict(areas=areas, counts=counts, points=take(np.float32, 4 * N).reshape(N, 4), tri=take(np.int32, N), bary=take(np.float32, 2 * N).reshape(N, 2))
    assert at == raw.size
    return 0, out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_on_the_cpu_equals_the_restatement(which, tool, sanitized_tool, tmp_path):
    """areas, counts, points, triangles and barycentrics bit for bit; the second round runs the same cases through the tool built with
    -fsanitize=address,undefined"""
    exe = sanitized_tool if which == "sanitized" else tool
    for name, v, f, density in cases():
        for seed in SEEDS:
            rc, got = _run(exe, tmp_path, v, f, density, seed)
            want = MS.sample(v, f, density, seed)
            assert rc == 0, name
            print("%s, seed %d: %d triangles, %d samples, %d empty triangles" % (name, seed, len(f), len(want["points"]), int((want["counts"] == 0).sum())))
            same_bits(got, want, "%s, seed %d" % (name, seed))
    v, f = MS.box()
    bad = f.copy()
    bad[3, 1] = 8
    assert _run(exe, tmp_path, v, bad, 10.0, 0)[0] == 3
    nan = v.copy()
    nan[2, 1] = np.nan
    assert _run(exe, tmp_path, nan, f, 10.0, 0)[0] == 3
    rc, got = _run(exe, tmp_path, v, f[:0], 10.0, 0)
    assert rc == 0 and len(got["points"]) == 0
    rc, got = _run(exe, tmp_path, v, f, 0.0, 0)
    assert rc == 0 and len(got["points"]) == 0 and np.array_equal(got["areas"], MS.areas(v, f))


def test_the_cases_are_what_the_gpu_tests_need():
    got = {name: MS.sample(v, f, density, 0) for name, v, f, density in cases()}
    assert len(got["box"]["counts"]) == 12 and 1900 < len(got["box"]["points"]) < 2100 and got["box"]["counts"].min() > 50
    lat = got["lattice"]
    assert len(lat["counts"]) == 4608 and set(lat["counts"].tolist()) == {0, 1} and abs(len(lat["points"]) - 1555) < 60 and (lat["counts"] == 0).sum() > 2900
    assert lat["counts"][:2048].sum() > 0 and lat["counts"][2048:].sum() > 0  # both sides of a scan chunk
    big = got["one big among small"]
    assert len(big["counts"]) == 301 and big["counts"][150] == 5000 and big["counts"].sum() == 5000
    deg = got["degenerate"]
    assert deg["areas"][1] == 0 and deg["areas"][2] == 0 and deg["counts"][1] == 0 and deg["counts"][2] == 0 and deg["counts"][0] > 300 and deg["counts"][3] > 300


# ---- properties of the restatement -----------------------------------------------------------------------------------------------------
def test_counts_are_floor_or_floor_plus_one_and_barycentrics_stay_inside():
    for name, v, f, density in cases():
        for seed in SEEDS + (1, 2):
            s = MS.sample(v, f, density, seed)
            fl = np.floor(s["areas"] * density).astype(np.int64)
            assert np.all((s["counts"] == fl) | (s["counts"] == fl + 1)), name
            assert np.all(s["counts"][s["areas"] == 0] == 0)
            r1, r2 = s["bary"][:, 0], s["bary"][:, 1]
            assert r1.dtype == np.float32 and np.all(r1 >= 0) and np.all(r2 >= 0)
            assert np.all(r1 + r2 <= np.float32(1)) and np.all(r1.astype(np.float64) + r2.astype(np.float64) <= 1.0), name  # in fp32 and exactly
            assert np.array_equal(np.diff(s["offsets"]), s["counts"]) and np.all(np.diff(s["tri"]) >= 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uniform_inside_a_triangle(seed):
    """the unit right triangle at density 80 000: exactly 40 000 samples; each of the four congruent sub-triangles holds 10 000 within
    5 sigma, sigma = sqrt(40 000 / 4 x 3 / 4) = 86.6"""
    s = MS.sample(*MS.unit_right_triangle(), 80000.0, seed)
    r1, r2 = s["bary"][:, 0].astype(np.float64), s["bary"][:, 1].astype(np.float64)
    assert len(r1) == 40000
    at_b, at_c = r1 >= 0.5, r2 >= 0.5
    at_a = ~at_b & ~at_c & (r1 + r2 < 0.5)
    middle = ~at_b & ~at_c & ~at_a
    parts = [int(at_b.sum()), int(at_c.sum()), int(middle.sum()), int(at_a.sum())]
    print("seed %d: sub-triangles %s" % (seed, parts))
    assert sum(parts) == 40000 and not (at_b & at_c).any()
    for c in parts:
        assert abs(c - 10000) <= 433


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uniform_across_triangles(seed):
    """[0, 2] x [0, 1] of two triangles at density 10 000: 20 000 samples; the share with x <= 1 + tau is within 5 sigma of (1 + tau) / 2"""
    s = MS.sample(*MS.rectangle(2.0, 1.0), 10000.0, seed)
    x = s["points"][:, 0].astype(np.float64)
    N = len(x)
    assert N == 20000
    for tau in (0.26, 0.3, 0.375, 0.45, 0.49):
        p = (1.0 + tau) / 2.0
        share, sigma = float((x <= 1.0 + tau).mean()), np.sqrt(p * (1.0 - p) / N)
        print("seed %d tau %.3f: share %.5f, expected %.5f, %.2f sigma" % (seed, tau, share, p, (share - p) / sigma))
        assert abs(share - p) <= 5.0 * sigma
