"""Time of one 640 x 480 screenshot view: raycast + shade (sobfu_hip_raycast + sobfu_hip_render_image) from the depth camera, in HIP events.

Volumes: phi_global after 2 synthetic frames of BASELINE config 3 (256^3, bench.py's translating sphere) and an init_sphere volume on config
5's 512^3 grid.  Per volume: warm-up, then the median over 9 windows of 20 views each.  Samples per ray (trilinear samples of the march,
hits and misses alike, rays outside the box count 0) come from the numpy restatement tests/render_reference.py on every 4th pixel in
each direction.  Prints one JSON line.  Kernel times: run under `rocprofv3 --kernel-trace --stats` separately.

    python tools/render_time.py [--windows 9] [--per-window 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sobfu_amd import fusion, ops, params, synthetic  # noqa: E402

import render_reference as RR  # noqa: E402


def time_view(vol, P, windows, per_window, rows=480, cols=640):
    pts = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty_like(pts)
    img = torch.empty((rows, cols, 4), dtype=torch.uint8, device="cuda")

    def view():
        ops.raycast(vol, P["vs"], P["trunc"], P["R"], P["t"], P["intr"], rows=rows, cols=cols, points=pts, normals=nrm)
        ops.render_image(pts, nrm, image=img)

    for _ in range(5):
        view()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_window):
            view()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / per_window)
    hits = int((nrm[..., 3] != 0).sum().item())
    # samples per ray from the restatement on a 1/4 x 1/4 grid of the same rays' camera
    fx, fy, cx, cy = P["intr"]
    _, _, samples = RR.raycast(vol.cpu().numpy(), P["vs"], P["trunc"], P["R"], P["t"], (fx / 4, fy / 4, cx / 4, cy / 4), rows // 4, cols // 4,
                               return_samples=True)
    med = float(np.median(ms))
    return {"ms_median": round(med, 4), "ms_min": round(float(min(ms)), 4), "ms_max": round(float(max(ms)), 4),
            "rays_per_s": round(rows * cols / (med * 1e-3)), "hit_pixels": hits, "samples_per_ray_mean": round(float(samples.mean()), 2),
            "samples_per_ray_max": int(samples.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--per-window", type=int, default=20)
    args = ap.parse_args()
    out = {"view": "640x480 raycast + shade", "windows": args.windows, "per_window": args.per_window}

    P = params.read_ini(os.path.join(ROOT, "params", "config3_boxing_256.ini"))
    size, tz, vx = float(P["size"][0]), float(P["t"][2]), float(P["vs"][0])
    fu = fusion.SobFusion(P)
    try:
        for n in range(2):  # bench.py's sequence: a sphere of radius 0.2 size translating 1.3 voxels per frame
            fu(torch.from_numpy(synthetic.render_sphere_depth((1.3 * vx * n, 0.0, tz + 0.5 * size), 0.2 * size, P["intr"])).cuda())
        torch.cuda.synchronize()
        out["phi_global_256"] = time_view(fu.phi_global, P, args.windows, args.per_window)
    finally:
        fu.close()
    del fu
    torch.cuda.empty_cache()

    P = params.read_ini(os.path.join(ROOT, "params", "config5_umbrella_512.ini"))
    size = P["size"].astype(np.float64)
    vol = ops.new_volume(P["dims"])
    ops.init_sphere(vol, P["vs"], P["trunc"], P["eta"], size / 2, 0.2 * float(size[0]))
    torch.cuda.synchronize()
    out["init_sphere_512"] = time_view(vol, P, args.windows, args.per_window)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
