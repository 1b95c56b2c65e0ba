"""sobfu_amd::write_png_rgb (include/sobfu_amd/depth_io.hpp) on the CPU: the file tests/cpp/png_write_tool.cpp writes is decoded here with
zlib / struct alone -- signature, IHDR, every chunk CRC and every pixel byte."""
import struct
import subprocess
import zlib

import numpy as np
import pytest

from sobfu_amd import build_host


def decode_png(data):
    """-> (width, height, bit depth, colour type, rgb (h, w, 3) uint8) of a non-interlaced 8-bit RGB PNG; checks every CRC"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + body) & 0xFFFFFFFF, typ
        chunks.append((typ, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, filt, inter) == (0, 0, 0)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    assert len(raw) == h * (3 * w + 1)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert (rows[:, 0] == 0).all()  # filter type 0 on every row
    return w, h, depth, ctype, rows[:, 1:].reshape(h, w, 3)


@pytest.fixture(scope="module")
def tool():
    return build_host.build_png_tool()


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (480, 1280)])
def test_png_round_trip(tool, tmp_path, rows, cols):
    out = tmp_path / "x.png"
    subprocess.run([tool, str(out), str(rows), str(cols)], check=True, timeout=60)
    w, h, depth, ctype, rgb = decode_png(out.read_bytes())
    assert (w, h, depth, ctype) == (cols, rows, 8, 2)
    y, x, c = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(3), indexing="ij")
    assert np.array_equal(rgb, ((7 * y + 13 * x + 101 * c) & 255).astype(np.uint8))


def test_png_unwritable_path(tool, tmp_path):
    r = subprocess.run([tool, str(tmp_path / "no" / "such" / "dir.png"), "2", "2"], timeout=60)
    assert r.returncode == 1
