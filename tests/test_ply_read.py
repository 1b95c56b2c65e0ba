"""read_ply (sobfu_amd/mesh_io.py and, through tests/cpp/mesh_eval_tool, sobfu_amd::read_ply of include/sobfu_amd/evaluate.hpp): the
round trip with write_ply, ASCII and binary variants, property order, and every refusal.  Runs without a GPU."""
import subprocess

import numpy as np
import pytest

from sobfu_amd import mesh_io


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build, build_host

    build.build_hip()  # the tool links the library
    return build_host.build_mesh_eval_tool()


def _mesh(seed=0, V=37, F=51):
    rng = np.random.default_rng(seed)
    v = np.ones((V, 4), np.float32)
    v[:, :3] = rng.normal(size=(V, 3))
    n = np.ones((V, 4), np.float32)
    n[:, :3] = rng.normal(size=(V, 3))
    f = rng.integers(0, V, (F, 3)).astype(np.int32)
    c = rng.integers(0, 256, (V, 4)).astype(np.uint8)
    c[:, 3] = 0
    v[0, :3] = [np.float32(1e-42), -0.0, 3.4e38]  # a denormal, a negative zero, a huge value: bit patterns must survive
    return v, n, f, c


def _cpp(tool, path, tmp_path):
    """-> ("ok", vertices, normals | None, faces, colours | None) or ("refused", message)"""
    pre = str(tmp_path / "cpp_out")
    r = subprocess.run([tool, "read", str(path), pre], capture_output=True, text=True, timeout=60)
    if r.returncode == 1:
        assert r.stdout.startswith("refused: "), r.stdout
        return ("refused", r.stdout[len("refused: "):].strip())
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    tag, V, F, hn, hc = r.stdout.split()
    assert tag == "ok"
    v = np.fromfile(pre + ".v", np.float32).reshape(-1, 4)
    n = np.fromfile(pre + ".n", np.float32).reshape(-1, 4) if int(hn) else None
    f = np.fromfile(pre + ".f", np.int32).reshape(-1, 3)
    c = np.fromfile(pre + ".c", np.uint8).reshape(-1, 4) if int(hc) else None
    assert len(v) == int(V) and len(f) == int(F)
    return ("ok", v, n, f, c)


def _same(x, y):
    if x is None or y is None:
        return x is None and y is None
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _both(tool, path, tmp_path):
    """the Python reader's arrays, after checking that the C++ reader gives the same"""
    got = mesh_io.read_ply(path)
    cpp = _cpp(tool, path, tmp_path)
    assert cpp[0] == "ok"
    for a, b in zip(got, cpp[1:]):
        assert _same(a, b) or (len(got[0]) == 0 and b is None)  # no vertices: a vector cannot say "normals, but none"
    return got


@pytest.mark.parametrize("coloured", [False, True])
def test_round_trip_with_write_ply(tool, tmp_path, coloured):
    v, n, f, c = _mesh()
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    mesh_io.write_ply(a, v, n, f, c if coloured else None)
    gv, gn, gf, gc = _both(tool, a, tmp_path)
    assert _same(gv, v) and _same(gn, n) and _same(gf, f)
    assert (_same(gc, c) if coloured else gc is None)
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and np.all(gv[:, 3] == 1)
    mesh_io.write_ply(b, gv, gn, gf, gc)
    assert a.read_bytes() == b.read_bytes()  # read, then write, gives the same file


def test_empty_mesh_round_trips(tool, tmp_path):
    z = np.zeros((0, 4), np.float32)
    mesh_io.write_ply(tmp_path / "e.ply", z, z, np.zeros((0, 3), np.int32))
    gv, gn, gf, gc = _both(tool, tmp_path / "e.ply", tmp_path)
    assert gv.shape == (0, 4) and gf.shape == (0, 3) and gc is None


TYPES = {"float": "<f4", "double": "<f8", "uchar": "u1", "int": "<i4", "uint": "<u4", "short": "<i2", "ushort": "<u2", "char": "i1"}


def _write(path, v, n, f, c, ascii, order, extra=(("quality", "float"),), count_type="uchar", index_type="int", tail=True):
    """a PLY with the vertex properties in `order`, extra unknown properties, chosen list types and an unknown element after the faces"""
    cols = {"x": v[:, 0], "y": v[:, 1], "z": v[:, 2], "nx": n[:, 0], "ny": n[:, 1], "nz": n[:, 2], "red": c[:, 2], "green": c[:, 1], "blue": c[:, 0]}
    kinds = {k: ("uchar" if k in ("red", "green", "blue") else "float") for k in cols}
    for k, (name, kind) in enumerate(extra):
        cols[name], kinds[name] = (np.arange(len(v)) % 7 + k).astype(TYPES[kind]), kind
    head = "ply\nformat %s 1.0\ncomment made by the test\nelement vertex %d\n" % ("ascii" if ascii else "binary_little_endian", len(v))
    head += "".join("property %s %s\n" % (kinds[k], k) for k in order)
    head += "element face %d\nproperty list %s %s vertex_indices\n" % (len(f), count_type, index_type)
    if tail:
        head += "element tail 2\nproperty int a\nproperty double b\n"
    head += "end_header\n"
    with open(path, "wb") as fh:
        fh.write(head.encode())
        if ascii:
            for i in range(len(v)):
                fh.write((" ".join(repr(float(cols[k][i])) if kinds[k] in ("float", "double") else str(int(cols[k][i])) for k in order) + "\n").encode())
            for t in f:
                fh.write(("3 %d %d %d\n" % tuple(t)).encode())
            if tail:
                fh.write(b"1 2.5\n-3 4\n")
        else:
            rec = np.zeros(len(v), np.dtype([(k, TYPES[kinds[k]]) for k in order]))
            for k in order:
                rec[k] = cols[k]
            fh.write(rec.tobytes())
            fr = np.zeros(len(f), np.dtype([("n", TYPES[count_type]), ("i", TYPES[index_type], (3,))]))
            fr["n"], fr["i"] = 3, f
            fh.write(fr.tobytes())
            if tail:
                fh.write(np.array([(1, 2.5), (-3, 4.0)], np.dtype([("a", "<i4"), ("b", "<f8")])).tobytes())


ORDERS = [("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "quality"),
          ("quality", "blue", "nz", "y", "red", "x", "ny", "green", "z", "nx")]


@pytest.mark.parametrize("ascii", [False, True])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("count_type, index_type", [("uchar", "int"), ("int", "uint"), ("uchar", "ushort")])
def test_variants_give_the_same_arrays(tool, tmp_path, ascii, order, count_type, index_type):
    """ASCII and binary, shuffled properties with an unknown one among them, list types: float32 values survive repr() exactly"""
    v, n, f, c = _mesh(1)
    v[0, :3] = [0.1, -0.0, 3.4e38]
    path = tmp_path / "m.ply"
    _write(path, v, n, f, c, ascii, order, count_type=count_type, index_type=index_type)
    gv, gn, gf, gc = _both(tool, path, tmp_path)
    assert _same(gv, v) and _same(gn, n) and _same(gf, f) and _same(gc, c)


def test_positions_only(tool, tmp_path):
    v, n, f, c = _mesh(2)
    _write(tmp_path / "p.ply", v, n, f, c, True, ("z", "x", "y"), extra=(), tail=False)
    gv, gn, gf, gc = _both(tool, tmp_path / "p.ply", tmp_path)
    assert _same(gv, v) and gn is None and gc is None and _same(gf, f)


def _refused(tool, path, tmp_path, word):
    with pytest.raises(ValueError) as e:
        mesh_io.read_ply(path)
    assert word in str(e.value), str(e.value)
    cpp = _cpp(tool, path, tmp_path)
    assert cpp[0] == "refused" and word in cpp[1], cpp


@pytest.mark.parametrize("ascii", [False, True])
def test_refusals(tool, tmp_path, ascii):
    v, n, f, c = _mesh(3)
    good = tmp_path / "good.ply"
    _write(good, v, n, f, c, ascii, ORDERS[0], tail=False)
    raw = good.read_bytes()
    body = raw.index(b"end_header\n") + len(b"end_header\n")

    def variant(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        return p

    # a truncated body: the faces are cut short, then the vertices
    _refused(tool, variant("cut_faces.ply", raw[:len(raw) - (7 if not ascii else 40)]), tmp_path, "more than the file holds")
    _refused(tool, variant("cut_vertices.ply", raw[:body + 50]), tmp_path, "more than the file holds")
    # counts past the end of the file
    _refused(tool, variant("many_vertices.ply", raw.replace(b"element vertex 37", b"element vertex 4000000000")), tmp_path, "more than the file holds")
    _refused(tool, variant("many_faces.ply", raw.replace(b"element face 51", b"element face 3000000000")), tmp_path, "more than the file holds")
    # big-endian
    _refused(tool, variant("big.ply", raw.replace(b"format ascii" if ascii else b"format binary_little_endian", b"format binary_big_endian")), tmp_path,
             "big-endian")
    # an index out of range
    bad = f.copy()
    bad[17, 1] = len(v)
    _write(tmp_path / "range.ply", v, n, bad, c, ascii, ORDERS[0], tail=False)
    _refused(tool, tmp_path / "range.ply", tmp_path, "outside [0, 37)")
    bad[17, 1] = -1
    _write(tmp_path / "negative.ply", v, n, bad, c, ascii, ORDERS[0], tail=False)
    _refused(tool, tmp_path / "negative.ply", tmp_path, "outside [0, 37)")
    # not a PLY, no end of header
    _refused(tool, variant("not.ply", b"plx\n" + raw[4:]), tmp_path, "not a PLY")
    _refused(tool, variant("open.ply", raw[:body - 11]), tmp_path, "end_header")


@pytest.mark.parametrize("ascii", [False, True])
def test_quads_are_refused(tool, tmp_path, ascii):
    v, n, f, c = _mesh(4, V=8, F=2)
    head = ("ply\nformat %s 1.0\nelement vertex 8\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n"
            "property list uchar int vertex_indices\nend_header\n" % ("ascii" if ascii else "binary_little_endian")).encode()
    if ascii:
        data = head + b"".join(b"%d %d %d\n" % (i, i, i) for i in range(8)) + b"3 0 1 2\n4 4 5 6 7\n"
    else:
        data = head + v[:, :3].tobytes() + b"\x03" + np.array([0, 1, 2], "<i4").tobytes() + b"\x04" + np.array([4, 5, 6, 7], "<i4").tobytes()
    p = tmp_path / "quad.ply"
    p.write_bytes(data)
    _refused(tool, p, tmp_path, "only triangles")
    # a quad first: the binary sizes no longer add up, and the reason given is still the polygon
    if not ascii:
        data = head + v[:, :3].tobytes() + b"\x04" + np.array([4, 5, 6, 7], "<i4").tobytes()
        p.write_bytes(data)
        _refused(tool, p, tmp_path, "only triangles")


def test_cpp_round_trip_through_write_ply(tool, tmp_path):
    """sobfu_amd::write_ply's bytes (tests/cpp/ply_write_tool's mesh) read back by both readers"""
    from sobfu_amd import build_host

    wt = build_host.build_ply_tool()
    for coloured in (0, 1):
        out = tmp_path / ("w%d.ply" % coloured)
        subprocess.run([wt, str(out), "23", "31", str(coloured)], check=True, timeout=60)
        gv, gn, gf, gc = _both(tool, out, tmp_path)
        assert len(gv) == 23 and len(gf) == 31 and (gc is not None) == bool(coloured)
        again = tmp_path / "again.ply"
        mesh_io.write_ply(again, gv, gn, gf, gc)
        assert again.read_bytes() == out.read_bytes()
