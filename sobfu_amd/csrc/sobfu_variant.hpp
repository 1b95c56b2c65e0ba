// Which instantiation of a fused pass a launch takes.  Host-only and free of HIP headers (tests/cpp/variant_tool.cpp compiles it with
// g++): one GridTraits per launch, pure choice functions that return a kernel's template arguments or a refusal, and the table of the
// instantiations that exist.  solver_kernels.hip launches the table row that equals the choice; a choice that is no row is refused.
#pragma once

#include <cstddef>
#include <cstdlib>

#include "sobfu_hip.h"

namespace sobfu_hip {

// The tuning environment, read at launch time -- once per launch and variable -- and by loop_warps_in_pass_a
// when a session begins, so that a change between two solves takes effect.
inline long env_cache_cells() {  // SOBFU_CACHE_CELLS: cells up to which the iteration's state (76 B per cell) stays in the 256 MiB Infinity Cache
    const char* e = getenv("SOBFU_CACHE_CELLS");
    return e ? atol(e) : 3300000L;  // ~250 MB / 76 B
}
inline int env_pipe_b() {  // SOBFU_PIPE_B=0/1 forces the pipelined march of pass B off / on; -1: unset
    const char* e = getenv("SOBFU_PIPE_B");
    return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
inline bool env_warp_a() {  // SOBFU_WARP_A=0 keeps the phi_n o psi stream in every loop
    const char* e = getenv("SOBFU_WARP_A");
    return !(e && atoi(e) == 0);
}

// What the choice needs to know of a launch's arrays: (X, Y, Z) the field arrays, (pX, pY, pZ) phi_n (the whole volume)
struct GridTraits {
    bool resident;  // the state stays in the Infinity Cache from one launch to the next: no streaming hints (they would push it out)
    bool idx32;     // tsdf-only phi_n below 4 GiB: 32-bit byte offsets for the corner gather
    bool arrays32;  // 12-byte arrays below 4 GiB: buffer addressing (the pipelined march, NTBUF, scope-carrying loads)
    bool plane32;   // in-plane byte offsets of 16-byte cells are 32-bit
    int pipe_b;     // SOBFU_PIPE_B: -1 unset (the pipelined march follows `resident`), else 0 / 1
};
inline GridTraits grid_traits(int X, int Y, int Z, int pX, int pY, int pZ, long cache_cells, int pipe_b = -1) {
    const size_t n = (size_t) X * Y * Z;
    GridTraits g;
    g.resident = (long) n <= cache_cells;
    g.idx32    = (size_t) pX * pY * pZ < ((size_t) 1 << 30);
    g.arrays32 = n * 12 < ((size_t) 1 << 32);
    g.plane32  = (size_t) X * Y * 16 < ((size_t) 1 << 32);
    g.pipe_b   = pipe_b;
    return g;
}

// ---- pass A: fused_potential_gradient_kernel<RPT, WY, COMPACT, NTL, WARP> and tile_potential_gradient_kernel<RPT, WY, COMPACT, NTL>
// (nt: NTL = kNT, else 0)
struct PassAVariant {
    bool compact, nt, warp;
    constexpr bool operator==(const PassAVariant& o) const { return compact == o.compact && nt == o.nt && warp == o.warp; }
};
inline constexpr PassAVariant kPassATable[] = {
    // compact  nt     warp
    {true,      true,  true},   // the warping march (loop_warps_in_pass_a)
    {true,      false, false},  // cache-resident grids
    {true,      true,  false},
    {false,     false, false},  // API format (launcher-level entry points)
};
inline constexpr PassAVariant kTilePassATable[] = {
    {true,  false, false},
    {true,  true,  false},
    {false, false, false},
};
// tile: the launch runs the tile kernel (it holds thin boxes, or it is a tile's planned pass A; kTilePassATable).  warp: pnp is
// phi_n (tsdf-only, extents X, Y, Z, sampled with 32-bit byte offsets) -- only the plain march of the compact format on a grid beyond
// the Infinity Cache samples it.  Streaming hints only for grids beyond the cache.
inline int choose_pass_a(const GridTraits& g, bool compact, bool warp, bool tile, PassAVariant* v) {
    if (warp && (tile || !compact || g.resident || !g.idx32)) return SOBFU_E_UNSUPPORTED;
    v->compact = compact;
    v->nt      = compact && !g.resident;
    v->warp    = warp;
    return 0;
}

// ---- pass B: fused_smooth_update_apply_kernel<RPT, WY, WRITE_UPDATES, COMPACT, DIRECT_OK, IDX32, HL, NTL, PIPE, NTBUF, APPLY>
// (lead: HL = SOBFU_HLEAD, else 0; nt: NTL = kNT, else 0)
struct PassBVariant {
    bool updates, compact, direct, idx32, lead, nt, pipe, ntbuf, apply;
    constexpr bool operator==(const PassBVariant& o) const {
        return updates == o.updates && compact == o.compact && direct == o.direct && idx32 == o.idx32 && lead == o.lead && nt == o.nt &&
               pipe == o.pipe && ntbuf == o.ntbuf && apply == o.apply;
    }
};
inline constexpr PassBVariant kPassBTable[] = {
    // updates compact direct idx32 lead nt  pipe  ntbuf apply
    {true , true , true , false, false, true , false, false, true },  // updates (reporting iterations, launcher-level entry points)
    {true , false, true , false, false, true , false, false, true },
    {false, true , true , true , false, false, true , false, true },  // the solver's own format: cache-resident, pipelined
    {false, true , true , true , false, false, false, false, true },  //   cache-resident
    {false, true , true , true , false, true , true , false, true },  //   pipelined
    {false, true , true , true , false, true , false, true , true },  //   plain march, buffer-addressed psi
    {false, true , true , true , false, true , false, false, true },  //   plain march, arrays of 4 GiB or more
    {false, true , true , false, false, true , false, false, true },  // compact, phi_n of 4 GiB or more
    {false, false, true , false, false, true , false, false, true },  // API format
    {true , true , false, false, false, true , false, false, true },  // the same without direct boxes ...
    {true , false, false, false, false, true , false, false, true },
    {false, true , false, true , true , true , false, true , false},  //   no phi_n o psi (the warping loop), halo lead
    {false, true , false, true , false, true , false, true , false},  //   no phi_n o psi
    {false, true , false, true , true , true , false, true , true },  //   halo lead, buffer-addressed psi
    {false, true , false, true , true , true , false, false, true },  //   halo lead
    {false, true , false, true , false, false, true , false, true },
    {false, true , false, true , false, false, false, false, true },
    {false, true , false, true , false, true , true , false, true },
    {false, true , false, true , false, true , false, true , true },
    {false, true , false, true , false, true , false, false, true },
    {false, true , false, false, false, true , false, false, true },
    {false, false, false, false, false, true , false, false, true },
};
// What a pass B launch asks for (from its PassBLaunch)
struct PassBAsk {
    bool compact, updates;
    bool sys_acquire;  // the launch reads cells other GPUs stored, at system scope: only the pipelined march does
    bool apply;        // false: no phi_n gather, no phi_n o psi store (the warping loop)
};
// How it marches: `pipe` before the geometry exists (it sets the chip's capacity and the even split), the rest from the finished box list
struct PassBMarch {
    bool pipe         = false;  // the software-pipelined march
    bool direct       = false;  // the list holds direct boxes
    bool long_marches = false;  // its longest march reaches SOBFU_HLEAD_MIN_ZC planes (and SOBFU_HLEAD > 0): the halo lead pays
};
// Stage 1: the pipelined march where the launch is latency-bound (cache-resident sizes; SOBFU_PIPE_B overrides) in the solver's own
// format (compact, 32-bit gather offsets, no `updates`, buffer addressing).  Connected tiles ALWAYS take it, whatever SOBFU_PIPE_B says:
// its loads carry the system scope for the halo cells other GPUs stored, and no launch falls back to one that reads them with ordinary loads.
inline int pass_b_march(const GridTraits& g, const PassBAsk& k, PassBMarch* m) {
    if (!g.plane32) return SOBFU_E_UNSUPPORTED;
    if (k.sys_acquire && !g.arrays32) return SOBFU_E_UNSUPPORTED;  // scope-carrying loads are buffer loads
    m->pipe = k.compact && g.idx32 && !k.updates && g.arrays32 && (k.sys_acquire || (g.pipe_b >= 0 ? g.pipe_b != 0 : g.resident));
    if (k.sys_acquire && !m->pipe) return SOBFU_E_UNSUPPORTED;
    return 0;
}
// Stage 2.  Streaming hints only for grids beyond the Infinity Cache; there the plain march's 12-byte psi load / store go through buffer
// instructions where the arrays allow it (NTBUF), and long marches request their halo SOBFU_HLEAD planes ahead (short ones -- small
// grids, multi-GPU tiles -- skip the extra prologue round trip).  !apply: the plain march with buffer-addressed psi only, any other
// launch would leave phi_n o psi stale.
inline int choose_pass_b(const GridTraits& g, const PassBAsk& k, const PassBMarch& m, PassBVariant* v) {
    if (!k.apply && (m.direct || !k.compact || !g.idx32 || k.updates || g.resident || m.pipe || !g.arrays32 || k.sys_acquire))
        return SOBFU_E_UNSUPPORTED;
    const bool own_format = k.compact && g.idx32 && !k.updates, plain_nt = !g.resident && !m.pipe;
    v->updates = k.updates;
    v->compact = k.compact;
    v->direct  = m.direct;
    v->idx32   = own_format;
    v->lead    = own_format && plain_nt && !m.direct && m.long_marches;
    v->nt      = !own_format || !g.resident;  // (the other formats take the template's default, kNT)
    v->pipe    = own_format && m.pipe;
    v->ntbuf   = own_format && plain_nt && g.arrays32;
    v->apply   = k.apply;
    return 0;
}

// Does the compact single-GPU loop of this grid run without the phi_n o psi stream?  Where both of its launches take that path: pass A
// warps phi_n itself over the whole grid (WARP), pass B neither warps nor stores F (APPLY = false) -- 68 instead of 76 B per cell and
// iteration.  That is a grid beyond the Infinity Cache whose pass B takes the plain march with buffer-addressed psi (NTBUF).
inline bool loop_warps_in_pass_a(const GridTraits& g) {
    const PassBAsk b{true, false, false, false};
    PassAVariant va;
    PassBVariant vb;
    PassBMarch m;
    return choose_pass_a(g, true, true, false, &va) == 0 && pass_b_march(g, b, &m) == 0 && choose_pass_b(g, b, m, &vb) == 0;
}
inline bool loop_warps_in_pass_a(int X, int Y, int Z) {  // the solver's choice at session_begin; SOBFU_WARP_A=0 turns the pair off
    return env_warp_a() && loop_warps_in_pass_a(grid_traits(X, Y, Z, X, Y, Z, env_cache_cells(), env_pipe_b()));
}

}  // namespace sobfu_hip
