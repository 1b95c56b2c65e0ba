"""The colour feature on the CPU: the C ABI's colour entry points (exported, argument checks before any device call, ABI version unchanged),
sobfu_amd::read_colour on well-formed and malformed PNG / PPM files, the uint8 .npy writer, write_vtk with and without colours (without: the
geometry-only format, byte for byte), and the numpy restatement tests/colour_reference.py against closed forms."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import colour_reference as CR

F9, F3 = C.c_float * 9, C.c_float * 3
A = C.c_void_p(4096)  # a 16-byte aligned address that is never dereferenced: every case below is refused before any device call


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build, build_host

    build.build_hip()
    return build_host.build_colour_tool()


NAMES = ("sobfu_hip_integrate_colour", "sobfu_hip_apply_colour", "sobfu_hip_sample_colour", "sobfu_hip_render_colour")


def test_colour_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in NAMES:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


def _integrate(lib, **kw):
    a = dict(image=A, image_step=16, rows=4, cols=4, tsdf=A, psi=None, colour=A, X=8, Y=8, Z=8, vs=F3(0.01, 0.01, 0.01),
             R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1), t=F3(0, 0, 0), fx=500.0, fy=500.0, cx=2.0, cy=2.0, cap=128)
    a.update(kw)
    f = C.c_float
    return lib.sobfu_hip_integrate_colour(a["image"], a["image_step"], a["rows"], a["cols"], a["tsdf"], a["psi"], a["colour"], a["X"], a["Y"],
                                          a["Z"], a["vs"], a["R"], a["t"], f(a["fx"]), f(a["fy"]), f(a["cx"]), f(a["cy"]), a["cap"], None)


def _apply(lib, **kw):
    a = dict(colour=A, warped=C.c_void_p(8192), psi_inv=A, X=8, Y=8, Z=8)
    a.update(kw)
    return lib.sobfu_hip_apply_colour(a["colour"], a["warped"], a["psi_inv"], a["X"], a["Y"], a["Z"], None)


def _sample(lib, **kw):
    a = dict(colour=A, X=8, Y=8, Z=8, vs=F3(0.01, 0.01, 0.01), R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1), t=F3(0, 0, 0), mc=0, points=A, points_step=64,
             normals=None, normals_step=0, rows=4, cols=4, out=A, out_step=16)
    a.update(kw)
    return lib.sobfu_hip_sample_colour(a["colour"], a["X"], a["Y"], a["Z"], a["vs"], a["R"], a["t"], a["mc"], a["points"], a["points_step"],
                                       a["normals"], a["normals_step"], a["rows"], a["cols"], a["out"], a["out_step"], None)


def _render(lib, **kw):
    a = dict(points=A, points_step=64, normals=A, normals_step=64, colours=A, colours_step=16, rows=4, cols=4, image=A, image_step=16)
    a.update(kw)
    f = C.c_float
    return lib.sobfu_hip_render_colour(a["points"], a["points_step"], a["normals"], a["normals_step"], a["colours"], a["colours_step"],
                                       a["rows"], a["cols"], f(0), f(0), f(0), a["image"], a["image_step"], None)


@pytest.mark.parametrize("kw", [
    dict(image=None), dict(tsdf=None), dict(colour=None), dict(vs=None), dict(R=None), dict(t=None),
    dict(X=0), dict(Y=-1), dict(Z=0), dict(Z=70000), dict(rows=0), dict(cols=0), dict(image_step=12),
    dict(image=C.c_void_p(4098)), dict(image_step=18), dict(colour=C.c_void_p(4098)), dict(tsdf=C.c_void_p(4100)), dict(psi=C.c_void_p(4104)),
    dict(cap=0), dict(cap=256), dict(cap=-3),
    dict(vs=F3(0, 0.01, 0.01)), dict(vs=F3(0.01, float("nan"), 0.01)), dict(vs=F3(0.01, 0.01, float("inf"))),
    dict(fx=0.0), dict(fy=float("nan")), dict(cx=float("inf")),
])
def test_integrate_colour_bad_arguments(lib, kw):
    assert _integrate(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(colour=None), dict(warped=None), dict(psi_inv=None), dict(warped=A), dict(X=0), dict(Z=-1),
    dict(colour=C.c_void_p(4097)), dict(warped=C.c_void_p(8194)), dict(psi_inv=C.c_void_p(4104)),
])
def test_apply_colour_bad_arguments(lib, kw):
    assert _apply(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(colour=None), dict(vs=None), dict(R=None), dict(t=None), dict(points=None), dict(out=None), dict(X=0), dict(rows=0), dict(cols=0),
    dict(points_step=48), dict(out_step=12), dict(normals=A, normals_step=48), dict(points=C.c_void_p(4104)), dict(points_step=72),
    dict(out=C.c_void_p(4098)), dict(normals=C.c_void_p(4104), normals_step=64), dict(vs=F3(0.01, 0, 0.01)), dict(colour=C.c_void_p(4097)),
])
def test_sample_colour_bad_arguments(lib, kw):
    assert _sample(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(points=None), dict(normals=None), dict(colours=None), dict(image=None), dict(rows=0), dict(cols=0), dict(points_step=48),
    dict(normals_step=48), dict(colours_step=12), dict(image_step=12), dict(points=C.c_void_p(4104)), dict(colours=C.c_void_p(4098)),
    dict(image=C.c_void_p(4098)),
])
def test_render_colour_bad_arguments(lib, kw):
    assert _render(lib, **kw) == -1


# ---- read_colour ---------------------------------------------------------------------------------------------------------------------
def _chunk(kind, body, crc=None):
    c = zlib.crc32(kind + body) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", c)


def _filter_rows(px, bpp, filters):
    """px (h, w * bpp) uint8 -> the filtered scanlines (filter byte + bytes) for the chosen filter per row"""
    h = px.shape[0]
    rows = px.astype(np.int32)
    prev = np.zeros(rows.shape[1], np.int32)
    raw = bytearray()
    for y in range(h):
        cur, ft = rows[y], filters[y % len(filters)]
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        if ft == 0:
            out = cur
        elif ft == 1:
            out = cur - a
        elif ft == 2:
            out = cur - prev
        elif ft == 3:
            out = cur - ((a + prev) >> 1)
        else:
            p = a + prev - c
            pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
            out = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        raw.append(ft)
        raw += bytes((out & 255).astype(np.uint8))
        prev = cur
    return bytes(raw)


def png(img, color_type, filters=(0, 1, 2, 3, 4), depth=8, interlace=0, idat_split=2, raw=None):
    h, w = img.shape[:2]
    bpp = {0: 1, 2: 3, 6: 4}[color_type]
    data = zlib.compress(raw if raw is not None else _filter_rows(img.reshape(h, w * bpp), bpp, filters))
    k = max(1, len(data) // idat_split)
    idats = b"".join(_chunk(b"IDAT", data[i:i + k]) for i in range(0, len(data), k))
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace)) + idats +
            _chunk(b"IEND", b""))


def ppm(img, maxval=255, comment=True):
    h, w = img.shape[:2]
    head = b"P6\n" + (b"# a comment\n" if comment else b"") + b"%d %d\n%d\n" % (w, h, maxval)
    return head + img.astype(np.uint8).tobytes()


def _read(tool, tmp_path, data, rows, cols):
    f, out = tmp_path / "in.bin", tmp_path / "out.raw"
    f.write_bytes(data)
    r = subprocess.run([tool, "read", str(f), str(rows), str(cols), str(out)], capture_output=True, text=True, timeout=60)
    if r.returncode != 0:
        return None, r.stdout
    return np.fromfile(out, np.uint8).reshape(rows, cols, 4), r.stdout


def _rgb(rows, cols, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


@pytest.mark.parametrize("color_type", [0, 2, 6])
def test_read_colour_png(tool, tmp_path, color_type):
    rows, cols = 13, 17
    rgb = _rgb(rows, cols, color_type)
    if color_type == 0:
        img, want = rgb[..., :1], np.concatenate([rgb[..., :1]] * 3, -1)
    elif color_type == 2:
        img, want = rgb, rgb
    else:
        img, want = np.concatenate([rgb, _rgb(rows, cols, 9)[..., :1]], -1), rgb
    got, msg = _read(tool, tmp_path, png(img, color_type), rows, cols)
    assert got is not None, msg
    assert np.array_equal(got[..., 0], want[..., 2]) and np.array_equal(got[..., 1], want[..., 1]) and np.array_equal(got[..., 2], want[..., 0])
    assert (got[..., 3] == 255).all()


def test_read_colour_ppm(tool, tmp_path):
    rgb = _rgb(9, 11)
    for comment in (True, False):
        got, msg = _read(tool, tmp_path, ppm(rgb, comment=comment), 9, 11)
        assert got is not None, msg
        assert np.array_equal(got[..., :3], rgb[..., ::-1]) and (got[..., 3] == 255).all()


def _malformed():
    rgb = _rgb(6, 5)
    good = png(rgb, 2)
    scan = bytearray(_filter_rows(rgb.reshape(6, 15), 3, (0,)))
    scan[16 * 2] = 5  # the filter byte of row 2
    absurd = bytearray(good)
    absurd[33:37] = struct.pack(">I", 0xFFFFFFF0)  # the length of the first IDAT (after the signature and the 25-byte IHDR chunk)
    bad_crc = bytearray(good)
    bad_crc[8 + 8 + 13] ^= 0xFF  # IHDR's CRC
    return {  # case: (file, what the refusal says)
        "truncated chunk": (good[:len(good) - 14], "truncated chunk"),
        "absurd length": (bytes(absurd), "truncated chunk"),
        "wrong size": (good, "size differs"),  # read as 7 x 5
        "filter byte above 4": (png(rgb, 2, raw=bytes(scan)), "bad row filter"),
        "crc": (bytes(bad_crc), "CRC mismatch"),
        "16-bit": (png(np.zeros((6, 5, 3), np.uint8), 2, depth=16, raw=b"\0" * (6 * 31)), "only 8-bit"),
        "palette": (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 6, 8, 3, 0, 0, 0)) + _chunk(b"IEND", b"") + b"\0" * 8,
                    "only 8-bit"),
        "interlaced": (png(rgb, 2, interlace=1), "interlaced"),
        "no IHDR": (b"\x89PNG\r\n\x1a\n" + _chunk(b"IEND", b"") + b"\0" * 30, "no IHDR"),
        "bad inflate": (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 6, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", b"xx") +
                        _chunk(b"IEND", b""), "inflate failed"),
        "short inflate": (png(rgb, 2, raw=_filter_rows(rgb.reshape(6, 15), 3, (0,))[:-16]), "inflate failed"),
        "ppm truncated": (ppm(rgb)[:-1], "truncated PPM"),
        "ppm maxval": (ppm(rgb, maxval=1023), "only 8-bit"),
        "ppm header": (b"P6\n5 x\n255\n" + b"\0" * 90, "bad PPM header"),
        "ppm wrong size": (ppm(_rgb(6, 4)), "size differs"),
        "not an image": (b"GIF89a" + b"\0" * 100, "not a PNG"),
        "empty": (b"", "not a PNG"),
    }


@pytest.mark.parametrize("case", sorted(_malformed()))
def test_read_colour_refuses_malformed(tool, tmp_path, case):
    data, why = _malformed()[case]
    rows = 7 if case == "wrong size" else 6
    got, msg = _read(tool, tmp_path, data, rows, 5)
    assert got is None and msg.startswith("error: ") and why in msg, (case, msg)


def test_read_colour_missing_file(tool, tmp_path):
    r = subprocess.run([tool, "read", str(tmp_path / "none.png"), "4", "4", str(tmp_path / "o")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stdout


def test_write_npy_uint8(tool, tmp_path):
    f = tmp_path / "c.npy"
    assert subprocess.run([tool, "npy", str(f), "3", "5", "7", "4"], timeout=60).returncode == 0
    a = np.load(f)
    assert a.dtype == np.uint8 and a.shape == (3, 5, 7, 4)
    assert np.array_equal(a.reshape(-1), (np.arange(a.size) & 255).astype(np.uint8))


def _vtk_geometry(n):
    """the geometry-only legacy VTK text of write_vtk before colour existed"""
    v = [(np.float32(0.5) * np.float32(i), np.float32(-0.25) * np.float32(i), np.float32(i) / np.float32(3)) for i in range(n)]
    s = "# vtk DataFile Version 3.0\nvtk output\nASCII\nDATASET POLYDATA\nPOINTS %d float\n" % n
    s += "".join("%.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v)
    s += "\nVERTICES %d %d\n" % (n, 2 * n) + "".join("1 %d\n" % i for i in range(n))
    nt = n // 3
    s += "\nPOLYGONS %d %d\n" % (nt, 4 * nt) + "".join("3 %d %d %d\n" % (3 * i, 3 * i + 1, 3 * i + 2) for i in range(nt))
    return s


def test_write_vtk_without_and_with_colours(tool, tmp_path):
    n = 9
    plain, col = tmp_path / "plain.vtk", tmp_path / "col.vtk"
    assert subprocess.run([tool, "vtk", str(plain), str(n), "0"], timeout=60).returncode == 0
    assert subprocess.run([tool, "vtk", str(col), str(n), "1"], timeout=60).returncode == 0
    assert plain.read_text() == _vtk_geometry(n)
    text = col.read_text()
    assert text.startswith(_vtk_geometry(n))
    tail = text[len(_vtk_geometry(n)):].split("\n")
    assert tail[:3] == ["", "POINT_DATA %d" % n, "COLOR_SCALARS rgb 3"]
    got = np.array([[float(x) for x in line.split()] for line in tail[3:3 + n]])
    i = np.arange(n)
    want = np.stack([(3 * i) & 255, (2 * i) & 255, i & 255], -1) / 255.0
    assert np.abs(got - want).max() < 1e-6


# ---- the restatement against closed forms ----------------------------------------------------------------------------------------
def test_restated_sampler_closed_forms():
    rng = np.random.default_rng(3)
    col = rng.integers(0, 256, (5, 6, 7, 4), dtype=np.uint8)
    col[..., 3] = rng.integers(1, 200, (5, 6, 7))
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    at = CR.sample(col, x.astype(np.float32), y.astype(np.float32), z.astype(np.float32))
    assert np.array_equal(at[..., :3], col[..., :3]) and (at[..., 3] == 1).all()  # at the voxels: the voxel's own colour
    mid = CR.sample(col, np.float32(2.5), np.float32(1), np.float32(3))  # half way along x: the mean of the two, rounded
    assert np.array_equal(mid[:3], np.rint((col[3, 1, 2, :3].astype(np.float32) + col[3, 1, 3, :3]) / 2).astype(np.uint8))
    col2 = col.copy()
    col2[3, 1, 3, 3] = 0  # a corner without colour is left out
    assert np.array_equal(CR.sample(col2, np.float32(2.25), np.float32(1), np.float32(3))[:3], col2[3, 1, 2, :3])
    col2[3, 1, 2, 3] = 0  # no corner with colour
    assert not CR.sample(col2, np.float32(2.25), np.float32(1), np.float32(3)).any()


def test_restated_integrate_closed_forms():
    tsdf = np.zeros((4, 5, 6, 2), np.float32)
    tsdf[..., 0], tsdf[..., 1] = 0.5, 1.0
    tsdf[0, 0, 0] = (0.0, 1.0)   # cleared-looking voxel: not observed
    tsdf[0, 0, 1] = (-1.0, 1.0)  # behind the surface at weight 1: not observed
    tsdf[0, 0, 2] = (1.0, 3.0)   # truncated: no colour
    tsdf[0, 0, 3] = (0.2, 0.0)   # weight 0: not observed
    img = np.zeros((40, 40, 4), np.uint8)
    img[...] = (10, 20, 30, 0)
    vs, R, t, intr = (0.01,) * 3, np.eye(3), np.array([-0.03, -0.025, 0.2], np.float32), (100.0, 100.0, 20.0, 20.0)
    col = CR.integrate_colour(img, tsdf, None, np.zeros((4, 5, 6, 4), np.uint8), vs, R, t, intr, 128)
    assert not col[0, 0, :4].any()
    assert (col[0, 0, 4:] == (10, 20, 30, 1)).all() and (col[1:] == (10, 20, 30, 1)).all()
    img[...] = (20, 41, 255, 7)
    col2 = CR.integrate_colour(img, tsdf, None, col, vs, R, t, intr, 2)
    assert (col2[1:] == (15, 30, 142, 2)).all()  # 30.5 -> 30 and 142.5 -> 142: rintf rounds half to even
    assert (CR.integrate_colour(img, tsdf, None, col2, vs, R, t, intr, 2)[1:, ..., 3] == 2).all()  # the cap holds
    psi = np.zeros((4, 5, 6, 4), np.float32)
    psi[..., 0] = 1000.0  # every voxel warped out of the image: nothing changes
    assert np.array_equal(CR.integrate_colour(img, tsdf, psi, col2, vs, R, t, intr, 2), col2)
