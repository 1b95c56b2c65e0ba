"""Call times of sobfu_hip_warp_stats (profiles/warp_stats.md), one JSON line per run: `python tools/warp_stats_time.py DIM
[ITERS]`.  One process per grid; psi, psi_inv and the two masks come from a real solve: params/config3_boxing_256.ini's values at DIM^3, a
sphere moved 1.3 voxels between two synthetic frames, ITERS (default 32) solver iterations.  Device events around each launch, the median
of CALLS launches after WARM warm-up launches; the launches only enqueue (the result stays on the device), so the events time the two
memsets and the kernel.
  a  statistics only, no mask                        16 B / voxel of compulsory traffic
  b  with the phi_global mask                        24
  c  with psi_inv and both masks                     48 (plus the sampler's gathers around psi_inv(x), mostly from cache)
  d  c plus both volumes                             56
  yardstick  sobfu_hip_reg_energy_sobolev_from_psi on the same psi: the same stencil over the same 16 B / voxel, and a read-back of its
             block partials that the call waits for (host-synchronised, so timed with the host clock around a synchronise as well)
GB/s = compulsory bytes over the median time.  SOBFU_LAUNCHER_NT=0 / 1 forces the plain / nontemporal instantiation."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sobfu_amd import _lib, fusion, ops, params, synthetic  # noqa: E402

WARM, CALLS = 3, 15
EDGES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(dim, iters):
    P = params.read_ini(os.path.join(ROOT, "params", "config3_boxing_256.ini"), dims=(dim if dim != 256 else None))
    size, tz, vx = float(P["size"][0]), float(P["t"][2]), float(P["vs"][0])
    fu = fusion.SobFusion(P, max_iter=iters)
    for n in range(2):
        fu(torch.from_numpy(synthetic.render_sphere_depth((1.3 * vx * n, 0.0, tz + 0.5 * size), 0.2 * size, P["intr"])).cuda())
    stats = fu.warp_stats()
    n = dim ** 3
    L = _lib.lib()
    words = torch.empty(64, dtype=torch.int64, device="cuda")
    det, res = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    vs = (C.c_float * 3)(*[float(v) for v in P["vs"]])
    edges = (C.c_float * len(EDGES))(*EDGES)
    tol = C.c_float(0.1 * vx)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(inv, mask, mask_inv, vols):
        rc = L.sobfu_hip_warp_stats(ptr(fu.psi), ptr(inv), ptr(mask), ptr(mask_inv), dim, dim, dim, vs, C.c_float(1.0), edges, len(EDGES), tol, ptr(words),
                                    ptr(det) if vols else None, ptr(res) if vols else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    out = dict(dim=dim, iterations=iters, nt=os.environ.get("SOBFU_LAUNCHER_NT", "auto"), line=stats.line(1))
    for name, args, bytes_per_voxel in (("a", (None, None, None, False), 16), ("b", (None, fu.phi_global, None, False), 24),
                                        ("c", (fu.psi_inv, fu.phi_global, fu.phi_global_psi_inv, False), 48),
                                        ("d", (fu.psi_inv, fu.phi_global, fu.phi_global_psi_inv, True), 56)):
        med, lo, hi = timed(lambda: call(*args))
        out[name] = dict(us=1e3 * med, min_us=1e3 * lo, max_us=1e3 * hi, gbps=bytes_per_voxel * n / (1e6 * med))
    med, lo, hi = timed(lambda: ops.reg_energy_sobolev_from_psi(fu.psi))
    host = []
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.reg_energy_sobolev_from_psi(fu.psi)
        torch.cuda.synchronize()
        host.append(1e3 * (time.perf_counter() - t0))
    out["yardstick"] = dict(us=1e3 * med, min_us=1e3 * lo, max_us=1e3 * hi, host_us=1e3 * float(np.median(host)), gbps=16 * n / (1e6 * med))
    fu.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256, int(sys.argv[2]) if len(sys.argv) > 2 else 32)
