"""Mesh files of the indexed marching-cubes path (ops.marching_cubes_indexed): binary little-endian PLY 1.0, byte for byte what
sobfu_amd::write_ply (include/sobfu_amd/sobfu.hpp) writes."""
from __future__ import annotations

import numpy as np


def _host(a, dtype):
    if a is None:
        return None
    if hasattr(a, "detach"):  # a torch tensor, on the GPU or not
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype)


def write_ply(path, vertices, normals, faces, colours=None):
    """vertices / normals (V, 4) float32 (x, y, z, w), faces (F, 3) int32, colours (V, 4) uint8 BGRA or None -> PLY with vertex
    (float x y z nx ny nz [uchar red green blue]) and face (list uchar int vertex_indices)"""
    v, n, f, c = _host(vertices, np.float32), _host(normals, np.float32), _host(faces, np.int32), _host(colours, np.uint8)
    V, Fn = len(v), len(f)
    if n.shape != (V, 4) or v.shape != (V, 4) or f.shape != (Fn, 3):
        raise ValueError(f"expected vertices / normals (V, 4) and faces (F, 3), got {v.shape} {n.shape} {f.shape}")
    coloured = c is not None and len(c) > 0
    if coloured and c.shape != (V, 4):
        raise ValueError(f"expected colours (V, 4), got {c.shape}")
    props = "".join(f"property float {p}\n" for p in ("x", "y", "z", "nx", "ny", "nz"))
    if coloured:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {V}\n{props}"
              f"element face {Fn}\nproperty list uchar int vertex_indices\nend_header\n")
    vt = [(p, "<f4") for p in ("x", "y", "z", "nx", "ny", "nz")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if coloured else [])
    rec = np.zeros(V, np.dtype(vt))
    for k, p in enumerate(("x", "y", "z")):
        rec[p] = v[:, k]
        rec["n" + p] = n[:, k]
    if coloured:
        rec["red"], rec["green"], rec["blue"] = c[:, 2], c[:, 1], c[:, 0]
    fr = np.zeros(Fn, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    fr["n"] = 3
    fr["i"] = f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(fr.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(buf, path):
    """-> (format, [(element name, count, [(property name, type) | (property name, count type, item type)])], body offset)"""
    if buf[:4] not in (b"ply\n", b"ply\r"):
        raise ValueError(f"{path}: not a PLY file")
    end = buf.find(b"end_header")
    nl = buf.find(b"\n", end)
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: the PLY header has no end_header line")
    fmt, elements = None, []
    for line in buf[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format" and len(w) == 3:
            if w[1] == "binary_big_endian":
                raise ValueError(f"{path}: big-endian PLY files are not supported")
            if w[1] not in ("ascii", "binary_little_endian") or w[2] != "1.0":
                raise ValueError(f"{path}: unknown PLY format {' '.join(w[1:])!r}")
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3 and w[2].isdigit():
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list" and w[2] in _PLY_TYPES and w[3] in _PLY_TYPES:
            elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
        else:
            raise ValueError(f"{path}: cannot read the PLY header line {line!r}")
    if fmt is None:
        raise ValueError(f"{path}: the PLY header has no format line")
    return fmt, elements, nl + 1


def read_ply(path):
    """A triangle mesh from a PLY 1.0 file, ASCII or binary little-endian -> vertices (V, 4) float32 with w = 1, normals (V, 4) float32
    with w = 1 or None, faces (F, 3) int32, colours (V, 4) uint8 BGRA (alpha 0, as the indexed marching cubes gives them) or None.
    Vertex properties may come in any order; unknown scalar properties are skipped.  Face lists: uchar / int counts, int / uint indices
    (any integer type).  ValueError for polygons other than triangles, big-endian files, element counts the file is too short for and
    vertex indices out of range.  read_ply then write_ply reproduces a file that write_ply wrote, byte for byte."""
    with open(path, "rb") as fh:
        buf = fh.read()
    fmt, elements, off = _ply_header(buf, path)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: no vertex element")
    ascii_tokens = buf[off:].split() if fmt == "ascii" else None
    tok = 0
    vert, faces = None, np.zeros((0, 3), np.int32)
    for name, count, props in elements:
        lists = [p for p in props if len(p) == 3]
        if lists and (name != "face" or len(props) != 1):
            if name in ("vertex", "face"):
                raise ValueError(f"{path}: element {name} has list properties this reader does not handle")
            raise ValueError(f"{path}: cannot skip element {name} with list properties")
        if not lists:  # fixed-size records
            dt = np.dtype([(p[0], "<" + p[1]) for p in props])
            if fmt == "ascii":
                k = count * len(props)
                if tok + k > len(ascii_tokens):
                    raise ValueError(f"{path}: element {name} declares {count} entries, more than the file holds")
                try:
                    vals = np.array(ascii_tokens[tok:tok + k], dtype=np.float64).reshape(count, len(props))
                except ValueError:
                    raise ValueError(f"{path}: element {name} holds something that is not a number") from None
                tok += k
                rec = np.zeros(count, dt)
                for j, p in enumerate(props):
                    rec[p[0]] = vals[:, j]
            else:
                if off + count * dt.itemsize > len(buf):
                    raise ValueError(f"{path}: element {name} declares {count} entries, more than the file holds")
                rec = np.frombuffer(buf, dt, count, off)
                off += count * dt.itemsize
            if name == "vertex":
                vert = rec
            continue
        if vert is None:
            raise ValueError(f"{path}: the face element comes before the vertex element")
        _, ct, it = lists[0]
        if ct[0] == "f" or it[0] == "f":
            raise ValueError(f"{path}: the face list must have integer counts and indices")
        if fmt == "ascii":
            if tok + 4 * count > len(ascii_tokens):
                raise ValueError(f"{path}: element face declares {count} entries, more than the file holds")
            try:
                vals = np.array(ascii_tokens[tok:tok + 4 * count], dtype=np.int64).reshape(count, 4)
            except ValueError:
                raise ValueError(f"{path}: the face element holds something that is not an integer") from None
            # a polygon with another count shifts the table: its count column no longer reads 3 everywhere
            tok += 4 * count
            n, idx = vals[:, 0], vals[:, 1:]
        else:
            dt = np.dtype([("n", "<" + ct), ("i", "<" + it, (3,))])
            if off + np.dtype("<" + ct).itemsize > len(buf) and count:
                raise ValueError(f"{path}: element face declares {count} entries, more than the file holds")
            first = int(np.frombuffer(buf, "<" + ct, 1, off)[0]) if count else 3
            if first != 3:
                raise ValueError(f"{path}: only triangles are supported, found a polygon of {first} vertices")
            if off + count * dt.itemsize > len(buf):
                raise ValueError(f"{path}: element face declares {count} entries, more than the file holds")
            rec = np.frombuffer(buf, dt, count, off)
            off += count * dt.itemsize
            n, idx = rec["n"].astype(np.int64), rec["i"].astype(np.int64)
        if count and not np.all(n == 3):
            bad = int(n[np.nonzero(n != 3)[0][0]])
            raise ValueError(f"{path}: only triangles are supported, found a polygon of {bad} vertices")
        V = len(vert) if vert is not None else 0
        if count and (idx.min() < 0 or idx.max() >= V):
            raise ValueError(f"{path}: a face refers to a vertex outside [0, {V})")
        faces = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    if vert is None:
        raise ValueError(f"{path}: the face element comes before the vertex element")
    have = set(vert.dtype.names or ())
    if not {"x", "y", "z"} <= have:
        raise ValueError(f"{path}: the vertex element has no x, y, z")
    V = len(vert)

    def cols(keys):
        out = np.ones((V, 4), np.float32)
        for k, key in enumerate(keys):
            out[:, k] = vert[key]
        return out

    vertices = cols(("x", "y", "z"))
    normals = cols(("nx", "ny", "nz")) if {"nx", "ny", "nz"} <= have else None
    colours = None
    if {"red", "green", "blue"} <= have:
        colours = np.zeros((V, 4), np.uint8)
        colours[:, 0], colours[:, 1], colours[:, 2] = vert["blue"], vert["green"], vert["red"]
    return vertices, normals, faces, colours
