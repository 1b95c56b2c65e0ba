"""Builds the C++ host-shell test driver (tests/cpp/host_shell_tests.cpp over include/sobfu_amd/sobfu.hpp) with g++.

The shells are header-only host code; the driver links libsobfu_hip.so (C ABI) and libamdhip64.so."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "build", "host_shell_tests")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


APP = os.path.join(ROOT, "build", "sobfu_headless")


def _compile(src: str, out: str) -> None:
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           f"-I{ROCM}/include", f"-I{os.path.join(ROOT, 'include')}", src, "-o", out, f"-L{HERE}", "-lsobfu_hip",
                           f"-L{ROCM}/lib", "-lamdhip64", "-lz", f"-Wl,-rpath,{HERE}", f"-Wl,-rpath,{ROCM}/lib", "-Wl,-rpath,$ORIGIN/../sobfu_amd"])


def build_app(force: bool = False) -> str:
    """apps/sobfu_headless.cpp: the headless frame-loop app over the shells."""
    src = os.path.join(ROOT, "apps", "sobfu_headless.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"), os.path.join(ROOT, "include", "sobfu_amd", "depth_io.hpp"),
            os.path.join(HERE, "libsobfu_hip.so")]
    if force or not os.path.exists(APP) or any(os.path.getmtime(APP) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(APP), exist_ok=True)
        _compile(src, APP)
    return APP


IO_TOOL = os.path.join(ROOT, "build", "depth_io_tool")


def build_io_tool(force: bool = False) -> str:
    """tests/cpp/depth_io_tool.cpp: CPU-only driver of the depth readers / .npy writer (needs zlib only)."""
    src = os.path.join(ROOT, "tests", "cpp", "depth_io_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "depth_io.hpp")]
    if force or not os.path.exists(IO_TOOL) or any(os.path.getmtime(IO_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(IO_TOOL), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", f"-I{os.path.join(ROOT, 'include')}", src, "-o", IO_TOOL, "-lz"])
    return IO_TOOL


PNG_TOOL = os.path.join(ROOT, "build", "png_write_tool")


def build_png_tool(force: bool = False) -> str:
    """tests/cpp/png_write_tool.cpp: CPU-only driver of the PNG writer (needs zlib only)."""
    src = os.path.join(ROOT, "tests", "cpp", "png_write_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "depth_io.hpp")]
    if force or not os.path.exists(PNG_TOOL) or any(os.path.getmtime(PNG_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(PNG_TOOL), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", f"-I{os.path.join(ROOT, 'include')}", src, "-o", PNG_TOOL, "-lz"])
    return PNG_TOOL


COLOUR_TOOL = os.path.join(ROOT, "build", "colour_io_tool")


def build_colour_tool(force: bool = False) -> str:
    """tests/cpp/colour_io_tool.cpp: CPU-only driver of read_colour, the uint8 .npy writer and write_vtk (runs without a GPU)."""
    src = os.path.join(ROOT, "tests", "cpp", "colour_io_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "depth_io.hpp"), os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"),
            os.path.join(ROOT, "include", "sobfu_hip.h"), os.path.join(HERE, "libsobfu_hip.so")]
    if force or not os.path.exists(COLOUR_TOOL) or any(os.path.getmtime(COLOUR_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(COLOUR_TOOL), exist_ok=True)
        _compile(src, COLOUR_TOOL)
    return COLOUR_TOOL


PLY_TOOL = os.path.join(ROOT, "build", "ply_write_tool")


def build_ply_tool(force: bool = False) -> str:
    """tests/cpp/ply_write_tool.cpp: CPU-only driver of sobfu_amd::write_ply (runs without a GPU)."""
    src = os.path.join(ROOT, "tests", "cpp", "ply_write_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"), os.path.join(ROOT, "include", "sobfu_hip.h"),
            os.path.join(HERE, "libsobfu_hip.so")]
    if force or not os.path.exists(PLY_TOOL) or any(os.path.getmtime(PLY_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(PLY_TOOL), exist_ok=True)
        _compile(src, PLY_TOOL)
    return PLY_TOOL


VARIANT_TOOL = os.path.join(ROOT, "build", "variant_tool")


def build_variant_tool(force: bool = False) -> str:
    """tests/cpp/variant_tool.cpp: CPU-only driver of the fused passes' instantiation choice (sobfu_amd/csrc/sobfu_variant.hpp, no HIP)."""
    src = os.path.join(ROOT, "tests", "cpp", "variant_tool.cpp")
    deps = [src, os.path.join(HERE, "csrc", "sobfu_variant.hpp"), os.path.join(ROOT, "include", "sobfu_hip.h")]
    if force or not os.path.exists(VARIANT_TOOL) or any(os.path.getmtime(VARIANT_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(VARIANT_TOOL), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", f"-I{os.path.join(HERE, 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", src, "-o",
                               VARIANT_TOOL])
    return VARIANT_TOOL


ICP_TOOL = os.path.join(ROOT, "build", "icp_shell_tool")


def build_icp_tool(force: bool = False) -> str:
    """tests/cpp/icp_shell_tool.cpp: camera tracking through ProjectiveICP, Frame and the imgproc shells."""
    src = os.path.join(ROOT, "tests", "cpp", "icp_shell_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"), os.path.join(HERE, "libsobfu_hip.so")]
    if force or not os.path.exists(ICP_TOOL) or any(os.path.getmtime(ICP_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(ICP_TOOL), exist_ok=True)
        _compile(src, ICP_TOOL)
    return ICP_TOOL


MESH_WARP_TOOL = os.path.join(ROOT, "build", "mesh_warp_tool")


def build_mesh_warp_tool(force: bool = False) -> str:
    """tests/cpp/mesh_warp_tool.cpp: the canonical mesh carried to live through SobFusion's shells (warp_mesh, fit_to_live)."""
    src = os.path.join(ROOT, "tests", "cpp", "mesh_warp_tool.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"), os.path.join(ROOT, "include", "sobfu_amd", "depth_io.hpp"),
            os.path.join(HERE, "libsobfu_hip.so")]
    if force or not os.path.exists(MESH_WARP_TOOL) or any(os.path.getmtime(MESH_WARP_TOOL) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(MESH_WARP_TOOL), exist_ok=True)
        _compile(src, MESH_WARP_TOOL)
    return MESH_WARP_TOOL


def build_host(force: bool = False) -> str:
    build_app(force)
    build_io_tool(force)
    build_png_tool(force)
    build_colour_tool(force)
    build_ply_tool(force)
    build_variant_tool(force)
    build_icp_tool(force)
    build_mesh_warp_tool(force)
    src = os.path.join(ROOT, "tests", "cpp", "host_shell_tests.cpp")
    deps = [src, os.path.join(ROOT, "include", "sobfu_amd", "sobfu.hpp"), os.path.join(ROOT, "include", "sobfu_hip.h"),
            os.path.join(HERE, "libsobfu_hip.so")]
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    _compile(src, OUT)
    return OUT


if __name__ == "__main__":
    print(build_host(force=True))
