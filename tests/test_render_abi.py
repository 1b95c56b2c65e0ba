"""The rendering entry points of the C ABI on the CPU: exported, argument checks before any device call (SOBFU_E_BADARG = -1), and the
ABI version is unchanged (adding entries is backward compatible)."""
import ctypes as C

import pytest

F9, F3 = C.c_float * 9, C.c_float * 3
A = C.c_void_p(4096)  # a 16-byte aligned address that is never dereferenced: every case below is refused before any device call


@pytest.fixture(scope="module")
def lib():
    from sobfu_amd import build

    build.build_hip()
    from sobfu_amd import _lib

    return _lib.lib()


def _raycast(lib, **kw):
    a = dict(vol=A, X=8, Y=8, Z=8, vsx=0.01, vsy=0.01, vsz=0.01, trunc=0.05, R=F9(1, 0, 0, 0, 1, 0, 0, 0, 1), t=F3(0, 0, 0), fx=500.0,
             fy=500.0, cx=2.0, cy=2.0, rows=4, cols=4, step_factor=0.75, points=A, points_step=64, normals=A, normals_step=64)
    a.update(kw)
    f = C.c_float
    return lib.sobfu_hip_raycast(a["vol"], a["X"], a["Y"], a["Z"], f(a["vsx"]), f(a["vsy"]), f(a["vsz"]), f(a["trunc"]), a["R"], a["t"],
                                 f(a["fx"]), f(a["fy"]), f(a["cx"]), f(a["cy"]), a["rows"], a["cols"], f(a["step_factor"]), a["points"],
                                 a["points_step"], a["normals"], a["normals_step"], None)


def _image(lib, **kw):
    a = dict(points=A, points_step=64, normals=A, normals_step=64, rows=4, cols=4, image=A, image_step=16)
    a.update(kw)
    return lib.sobfu_hip_render_image(a["points"], a["points_step"], a["normals"], a["normals_step"], a["rows"], a["cols"], C.c_float(0),
                                      C.c_float(0), C.c_float(0), a["image"], a["image_step"], None)


def _normals(lib, **kw):
    a = dict(normals=A, normals_step=64, rows=4, cols=4, image=A, image_step=16)
    a.update(kw)
    return lib.sobfu_hip_render_normals(a["normals"], a["normals_step"], a["rows"], a["cols"], a["image"], a["image_step"], None)


def test_render_symbols_exported_and_version_unchanged(lib):
    from sobfu_amd import _lib

    for n in ("sobfu_hip_raycast", "sobfu_hip_render_image", "sobfu_hip_render_normals"):
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.sobfu_hip_abi_version() == 3


@pytest.mark.parametrize("kw", [
    dict(vol=None), dict(R=None), dict(t=None), dict(points=None), dict(normals=None),
    dict(X=1), dict(Y=1), dict(Z=1), dict(X=0), dict(rows=0), dict(cols=0), dict(rows=-1),
    dict(points_step=48), dict(normals_step=48),                               # a row of 4 float4 is 64 bytes
    dict(points=C.c_void_p(4104)), dict(normals=C.c_void_p(4100)),             # not 16-byte aligned
    dict(points_step=72), dict(normals_step=68),                               # rows after the first not 16-byte aligned
    dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=float("inf")), dict(trunc=float("nan")),
    dict(step_factor=0.0), dict(step_factor=-1.0), dict(step_factor=float("inf")), dict(step_factor=float("nan")),
    dict(vsx=0.0), dict(vsz=float("nan")), dict(fx=0.0),
])
def test_raycast_bad_arguments(lib, kw):
    assert _raycast(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(points=None), dict(normals=None), dict(image=None), dict(rows=0), dict(cols=0),
    dict(points_step=48), dict(normals_step=48), dict(image_step=12),
    dict(points=C.c_void_p(4104)), dict(normals=C.c_void_p(4104)), dict(image=C.c_void_p(4098)),
])
def test_render_image_bad_arguments(lib, kw):
    assert _image(lib, **kw) == -1


@pytest.mark.parametrize("kw", [
    dict(normals=None), dict(image=None), dict(rows=0), dict(cols=0), dict(normals_step=48), dict(image_step=12),
    dict(normals=C.c_void_p(4104)), dict(image=C.c_void_p(4098)),
])
def test_render_normals_bad_arguments(lib, kw):
    assert _normals(lib, **kw) == -1
