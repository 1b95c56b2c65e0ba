"""Builds the host-side C++ programs with g++: the headless app, the host-shell test driver (tests/cpp/host_shell_tests.cpp over
include/sobfu_amd/sobfu.hpp) and the small tools under tests/cpp that the CPU tests drive.

The shells are header-only host code; what uses them links libsobfu_hip.so (C ABI) and libamdhip64.so.  The stand-alone tools need
neither HIP nor the library."""
from __future__ import annotations

import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsobfu_hip.so")
SOBFU_HPP = os.path.join(INC, "sobfu_amd", "sobfu.hpp")
DEPTH_IO_HPP = os.path.join(INC, "sobfu_amd", "depth_io.hpp")
SOBFU_HIP_H = os.path.join(INC, "sobfu_hip.h")
EVALUATE_HPP = os.path.join(INC, "sobfu_amd", "evaluate.hpp")  # part of sobfu.hpp
WARP_STATS_HPP = os.path.join(INC, "sobfu_amd", "warp_stats.hpp")  # part of sobfu.hpp
TRAJECTORY_HPP = os.path.join(INC, "sobfu_amd", "trajectory.hpp")


def _test_src(name: str) -> str:
    return os.path.join(ROOT, "tests", "cpp", name)


def _build(out: str, src: str, deps, linked: bool, force: bool = False, flags=()) -> str:
    """g++ `src` into build/`out` when it is missing or older than `src` / `deps`.  linked: against libsobfu_hip.so and the HIP
    runtime (the library is then a dependency too; `flags` are added); else a stand-alone program with `flags`."""
    out = os.path.join(ROOT, "build", out)
    deps = [src, *deps] + ([LIB] if linked else [])
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if linked:
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                               f"-I{ROCM}/include", f"-I{INC}", src, "-o", out, f"-L{HERE}", "-lsobfu_hip",
                               f"-L{ROCM}/lib", "-lamdhip64", "-lz", f"-Wl,-rpath,{HERE}", f"-Wl,-rpath,{ROCM}/lib", "-Wl,-rpath,$ORIGIN/../sobfu_amd", *flags])
    else:
        subprocess.check_call(["g++", "-O2", "-Wall", f"-I{INC}", src, "-o", out, *flags])
    return out


def build_app(force: bool = False) -> str:
    """apps/sobfu_headless.cpp: the headless frame-loop app over the shells."""
    return _build("sobfu_headless", os.path.join(ROOT, "apps", "sobfu_headless.cpp"), [SOBFU_HPP, EVALUATE_HPP, WARP_STATS_HPP, DEPTH_IO_HPP, TRAJECTORY_HPP, SOBFU_HIP_H], True, force)


def build_io_tool(force: bool = False) -> str:
    """tests/cpp/depth_io_tool.cpp: CPU-only driver of the depth readers / .npy writer (needs zlib only)."""
    return _build("depth_io_tool", _test_src("depth_io_tool.cpp"), [DEPTH_IO_HPP], False, force, ["-std=c++14", "-lz"])


def build_png_tool(force: bool = False) -> str:
    """tests/cpp/png_write_tool.cpp: CPU-only driver of the PNG writer (needs zlib only)."""
    return _build("png_write_tool", _test_src("png_write_tool.cpp"), [DEPTH_IO_HPP], False, force, ["-std=c++14", "-lz"])


def build_colour_tool(force: bool = False) -> str:
    """tests/cpp/colour_io_tool.cpp: CPU-only driver of read_colour, the uint8 .npy writer and write_vtk (runs without a GPU)."""
    return _build("colour_io_tool", _test_src("colour_io_tool.cpp"), [DEPTH_IO_HPP, SOBFU_HPP, SOBFU_HIP_H], True, force)


def build_ply_tool(force: bool = False) -> str:
    """tests/cpp/ply_write_tool.cpp: CPU-only driver of sobfu_amd::write_ply (runs without a GPU)."""
    return _build("ply_write_tool", _test_src("ply_write_tool.cpp"), [SOBFU_HPP, SOBFU_HIP_H], True, force)


def build_variant_tool(force: bool = False) -> str:
    """tests/cpp/variant_tool.cpp: CPU-only driver of the fused passes' instantiation choice (sobfu_amd/csrc/sobfu_variant.hpp, no HIP)."""
    return _build("variant_tool", _test_src("variant_tool.cpp"), [os.path.join(CSRC, "sobfu_variant.hpp"), SOBFU_HIP_H], False, force,
                  ["-std=c++17", f"-I{CSRC}"])


def build_geometry_tool(force: bool = False, flags=()) -> str:
    """tests/cpp/geometry_tool.cpp: CPU-only driver of the launch and tile geometry (sobfu_amd/csrc/sobfu_geometry.hpp and
    sobfu_tile_layout.hpp, no HIP)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_geometry.hpp", "sobfu_tile_layout.hpp", "sobfu_variant.hpp")] + [SOBFU_HIP_H]
    return _build("geometry_tool", _test_src("geometry_tool.cpp"), deps, False, force, ["-std=c++17", f"-I{CSRC}", *flags])


def build_icp_tool(force: bool = False) -> str:
    """tests/cpp/icp_shell_tool.cpp: camera tracking through ProjectiveICP, Frame and the imgproc shells."""
    return _build("icp_shell_tool", _test_src("icp_shell_tool.cpp"), [SOBFU_HPP], True, force)


def build_mesh_warp_tool(force: bool = False) -> str:
    """tests/cpp/mesh_warp_tool.cpp: the canonical mesh carried to live through SobFusion's shells (warp_mesh, fit_to_live)."""
    return _build("mesh_warp_tool", _test_src("mesh_warp_tool.cpp"), [SOBFU_HPP, DEPTH_IO_HPP], True, force)


def build_mesh_eval_tool(force: bool = False) -> str:
    """tests/cpp/mesh_eval_tool.cpp: read_ply, the point-triangle rule on the CPU (-ffp-contract=off, as the kernels are built) and
    compare_meshes (include/sobfu_amd/evaluate.hpp, sobfu_amd/csrc/sobfu_mesh_distance.hpp)."""
    deps = [SOBFU_HPP, EVALUATE_HPP, SOBFU_HIP_H, os.path.join(CSRC, "sobfu_mesh_distance.hpp")]
    return _build("mesh_eval_tool", _test_src("mesh_eval_tool.cpp"), deps, True, force, [f"-I{CSRC}", "-ffp-contract=off"])


def build_mesh_ray_tool(force: bool = False, flags=()) -> str:
    """tests/cpp/mesh_ray_tool.cpp: CPU-only driver of the ray-triangle rule (sobfu_amd/csrc/sobfu_mesh_ray.hpp, no HIP; -ffp-contract=off,
    as the kernels are built)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_mesh_ray.hpp", "sobfu_mesh_distance.hpp")]
    return _build("mesh_ray_tool", _test_src("mesh_ray_tool.cpp"), deps, False, force, ["-std=c++14", f"-I{CSRC}", "-ffp-contract=off", *flags])


def build_mesh_parity_tool(force: bool = False, flags=()) -> str:
    """tests/cpp/mesh_parity_tool.cpp: CPU-only driver of the row-crossing rule (sobfu_amd/csrc/sobfu_mesh_parity.hpp, no HIP;
    -ffp-contract=off, as the kernels are built)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_mesh_parity.hpp", "sobfu_mesh_distance.hpp")]
    return _build("mesh_parity_tool", _test_src("mesh_parity_tool.cpp"), deps, False, force, ["-std=c++14", f"-I{CSRC}", "-ffp-contract=off", *flags])


def build_mesh_winding_tool(force: bool = False, flags=(), out: str = "mesh_winding_tool") -> str:
    """tests/cpp/mesh_winding_tool.cpp: CPU-only driver of the winding-number rule and the boundary chain
    (sobfu_amd/csrc/sobfu_mesh_winding.hpp, sobfu_mesh_boundary.hpp, no HIP; -ffp-contract=off, as the kernels are built).  out: the
    program's name under build/ (a second build with other flags keeps the first)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_mesh_winding.hpp", "sobfu_mesh_boundary.hpp", "sobfu_mesh_parity.hpp", "sobfu_mesh_distance.hpp")]
    return _build(out, _test_src("mesh_winding_tool.cpp"), deps, False, force, ["-std=c++14", f"-I{CSRC}", "-ffp-contract=off", *flags])


def build_mesh_sample_tool(force: bool = False, flags=(), out: str = "mesh_sample_tool") -> str:
    """tests/cpp/mesh_sample_tool.cpp: CPU-only driver of the mesh sampling rule (sobfu_amd/csrc/sobfu_mesh_sample.hpp, no HIP;
    -ffp-contract=off, as the kernels are built).  out: the program's name under build/ (a second build with other flags keeps the first)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_mesh_sample.hpp", "sobfu_mesh_distance.hpp", "sobfu_random.hpp")]
    return _build(out, _test_src("mesh_sample_tool.cpp"), deps, False, force, ["-std=c++17", f"-I{CSRC}", "-ffp-contract=off", *flags])


def build_warp_stats_tool(force: bool = False, flags=(), out: str = "warp_stats_tool") -> str:
    """tests/cpp/warp_stats_tool.cpp: CPU-only driver of the warp-field diagnostics' rules (sobfu_amd/csrc/sobfu_warp_stats.hpp, no HIP;
    -ffp-contract=off, as the kernels are built).  out: the program's name under build/ (a second build with other flags keeps the first)."""
    return _build(out, _test_src("warp_stats_tool.cpp"), [os.path.join(CSRC, "sobfu_warp_stats.hpp"), SOBFU_HIP_H], False, force,
                  ["-std=c++17", f"-I{CSRC}", "-ffp-contract=off", *flags])


def build_rigid_tool(force: bool = False) -> str:
    """tests/cpp/rigid_solve_tool.cpp: CPU-only driver of the shared rigid solve (sobfu_amd/csrc/sobfu_rigid.hpp, no HIP; -ffp-contract=off,
    as the kernels are built)."""
    return _build("rigid_solve_tool", _test_src("rigid_solve_tool.cpp"), [os.path.join(CSRC, "sobfu_rigid.hpp")], False, force,
                  ["-std=c++14", f"-I{CSRC}", "-ffp-contract=off"])


def build_depth_sensor_tool(force: bool = False) -> str:
    """tests/cpp/depth_sensor_tool.cpp: the depth sensor model through its C++ twin (sobfu_amd::SensorModel, sobfu_amd::depth_sensor)."""
    return _build("depth_sensor_tool", _test_src("depth_sensor_tool.cpp"), [SOBFU_HPP, EVALUATE_HPP, SOBFU_HIP_H], True, force)


def build_trajectory_tool(force: bool = False, flags=()) -> str:
    """tests/cpp/trajectory_tool.cpp: CPU-only driver of include/sobfu_amd/trajectory.hpp (TUM files, ATE, RPE; no HIP)."""
    return _build("trajectory_tool", _test_src("trajectory_tool.cpp"), [TRAJECTORY_HPP], False, force, ["-std=c++14", *flags])


def build_pass_a_plan_tool(force: bool = False) -> str:
    """tests/cpp/pass_a_plan_tool.cpp: CPU-only driver of the warping march's launch plan (sobfu_amd/csrc/sobfu_geometry.hpp, no HIP)."""
    deps = [os.path.join(CSRC, h) for h in ("sobfu_geometry.hpp", "sobfu_variant.hpp")] + [SOBFU_HIP_H]
    return _build("pass_a_plan_tool", _test_src("pass_a_plan_tool.cpp"), deps, False, force, ["-std=c++17", f"-I{CSRC}"])


def build_host(force: bool = False) -> str:
    for build in (build_pass_a_plan_tool, build_depth_sensor_tool, build_trajectory_tool, build_app, build_io_tool, build_png_tool, build_colour_tool, build_ply_tool, build_variant_tool, build_geometry_tool,
                  build_icp_tool, build_mesh_warp_tool, build_mesh_eval_tool, build_mesh_ray_tool, build_mesh_parity_tool, build_mesh_winding_tool, build_mesh_sample_tool, build_warp_stats_tool, build_rigid_tool):
        build(force)
    return _build("host_shell_tests", _test_src("host_shell_tests.cpp"), [SOBFU_HPP, EVALUATE_HPP, SOBFU_HIP_H], True, force)


if __name__ == "__main__":
    print(build_host(force=True))
