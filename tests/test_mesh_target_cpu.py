"""The nine leading arguments of every mesh entry point of the C ABI -- (workspace, bytes, vertices, n_vertices, faces, n_triangles, origin,
h, dims): the triangle grid and its mesh -- are judged by one validator (sobfu_amd/csrc/sobfu_mesh.hpp).  Table-driven: every entry point
x every defect of that prefix, the other arguments valid, is refused with SOBFU_E_BADARG before any device call.  The addresses are
aligned and never dereferenced; no GPU is needed."""
import ctypes as C

import pytest

F3, I3, F9 = C.c_float * 3, C.c_int * 3, C.c_float * 9
P = [C.c_void_p(4096 * k) for k in range(1, 12)]  # 16-byte aligned addresses that are never dereferenced
BADARG = -1
DIMS = (2, 3, 4)
I9 = F9(1, 0, 0, 0, 1, 0, 0, 0, 1)


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    L = _lib.lib()
    L.sobfu_hip_mesh_grid_workspace_bytes.restype = C.c_size_t
    return L


def _prefix(lib, **kw):
    a = dict(ws=P[0], ws_bytes=lib.sobfu_hip_mesh_grid_workspace_bytes(I3(*DIMS), 0), v=P[1], nv=8, f=P[2], nt=4, origin=F3(0, 0, 0), h=0.5,
             dims=I3(*DIMS))
    a.update(kw)
    return a


def _lead(a):
    return (a["ws"], C.c_size_t(a["ws_bytes"]), a["v"], a["nv"], a["f"], a["nt"], a["origin"], C.c_float(a["h"]), a["dims"])


def _f(x):
    return C.c_float(x)


# name -> (call with the prefix, can the valid call be made without a device: nothing to do is a success)
ENTRY = {
    "grid_build": (lambda L, a: L.sobfu_hip_mesh_grid_build(a["v"], a["nv"], a["f"], a["nt"], a["origin"], _f(a["h"]), a["dims"], a["ws"],
                                                            C.c_size_t(a["ws_bytes"]), 0, C.byref(C.c_int(0)), None), False),
    "distance": (lambda L, a: L.sobfu_hip_mesh_distance(*_lead(a), P[3], 0, _f(0.0), 0, 0, P[4], P[5], None, P[6], None), True),
    "raycast": (lambda L, a: L.sobfu_hip_mesh_raycast(*_lead(a), P[3], P[4], 0, _f(0.0), _f(0.0), 0, P[5], P[6], None, None, None), True),
    "render": (lambda L, a: L.sobfu_hip_mesh_render(*_lead(a), None, None, I9, F3(0, 0, 0), _f(500.0), _f(500.0), _f(8.0), _f(6.0), 12, 16, _f(0.0),
                                                    _f(0.0), None, 0, None, 0, None, 0, None, 0, None, 0, None), True),
    "voxelise": (lambda L, a: L.sobfu_hip_mesh_voxelise(*_lead(a), P[3], 8, 8, 8, F3(0.1, 0.1, 0.1), _f(0.3), _f(0.1), 0, P[4], C.c_size_t(1 << 20),
                                                        P[5], None), False),
    "inside": (lambda L, a: L.sobfu_hip_mesh_inside(*_lead(a), P[3], 0, P[4], P[5], 0, None), True),
    "align_step": (lambda L, a: L.sobfu_hip_mesh_align_step(*_lead(a), P[3], 0, _f(0.0), 0, 0, P[4], P[5], C.c_size_t(1 << 20), P[6], None), True),
    "align_estimate": (lambda L, a: L.sobfu_hip_mesh_align_estimate(*_lead(a), P[3], 0, _f(0.0), 0, 0, 5, 6, _f(0.0), _f(0.0), P[5], C.c_size_t(1 << 20),
                                                                    P[4], P[6], None, None), True),
}

DEFECT = {
    "workspace NULL": lambda n: dict(ws=None),
    "workspace not a multiple of 16": lambda n: dict(ws=C.c_void_p(4096 + 8)),
    "workspace one byte short": lambda n: dict(ws_bytes=n - 1),
    "origin NaN": lambda n: dict(origin=F3(0, float("nan"), 0)),
    "h 0": lambda n: dict(h=0.0),
    "h +Inf": lambda n: dict(h=float("inf")),
    "a dim of 0": lambda n: dict(dims=I3(2, 0, 4)),
    "a dim of 129": lambda n: dict(dims=I3(2, 3, 129), ws_bytes=1 << 30),
    "n_vertices < 0": lambda n: dict(nv=-1),
    "n_triangles < 0": lambda n: dict(nt=-1),
    "triangles without vertices": lambda n: dict(v=None),
    "triangles without faces": lambda n: dict(f=None),
    "vertices at 4 mod 16": lambda n: dict(v=C.c_void_p(8192 + 4)),
    "faces at 2 mod 4": lambda n: dict(f=C.c_void_p(12288 + 2)),
}


@pytest.mark.parametrize("defect", sorted(DEFECT))
@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_a_defect_in_the_shared_prefix_is_refused(lib, entry, defect):
    call, _ = ENTRY[entry]
    n = lib.sobfu_hip_mesh_grid_workspace_bytes(I3(*DIMS), 0)
    assert n > 0
    assert call(lib, _prefix(lib, **DEFECT[defect](n))) == BADARG


@pytest.mark.parametrize("entry", sorted(e for e in ENTRY if ENTRY[e][1]))
def test_the_table_is_otherwise_valid(lib, entry):
    """with nothing to do (no points, no rays, no output image) the same call without the defect is a success: the refusals above are the
    defect's alone.  (The build and the voxeliser always launch; their other arguments are those of the GPU suites.)"""
    assert ENTRY[entry][0](lib, _prefix(lib)) == 0
