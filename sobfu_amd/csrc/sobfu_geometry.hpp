// The geometry of a fused launch: which boxes of cells it produces, how many planes a workgroup marches, how many workgroups that
// makes and how they are numbered.  Host-only and free of HIP headers (tests/cpp/geometry_tool.cpp compiles it with g++): the plain
// structs that describe a launch and its planned form (the kernels read the latter: solver_iter_common.inl, solver_pass_a.inl), and
// the planners, pure functions of the boxes, the tuning environment and the chip's capacity.  solver_kernels.hip plans, chooses the
// variant (sobfu_variant.hpp) and launches.  A wrong plan changes no bits, it is only slower: tests/test_launch_geometry.py pins it.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "sobfu_variant.hpp"

#ifndef SOBFU_PAIR_B
#define SOBFU_PAIR_B 1  // cache-resident launches of the pipelined pass B: z-chunks march in alternating directions (Box::pair)
#endif
#ifndef SOBFU_HLEAD
#define SOBFU_HLEAD 3  // planes the halo requests of pass B run ahead on long marches (0: never; one plane ahead, straight from registers)
#endif
#ifndef SOBFU_HLEAD_MIN_ZC
#define SOBFU_HLEAD_MIN_ZC 24  // shortest march (planes) that uses the halo lead
#endif

namespace sobfu_hip {

// Tile configuration of the fused passes (see DESIGN.md "Kernel tuning").
constexpr int TX = 64;  // tile width in lanes: one wave per tile row (32-wide tiles measured slower: profiles/LABBOOK.md, round 5)
// tile of a workgroup: 64 lanes x 8 waves, one row per wave (rows-per-thread 2 / 4 and 4 / 16 waves were measured in rounds 1 - 2:
// profiles/LABBOOK.md; the kernels keep RPT / WY as template parameters, the launchers instantiate this one shape)
constexpr int kRPT = 1, kWY = 8;
// ... but the WARPING march of pass A, whose halo rows and columns cost a whole trilinear sample per wave: three halo tasks per 16 rows
// instead of three per 8 (1.19 x instead of 1.375 x wave-samples per row); 8 and 16 measured: profiles/r08_pass_a_tiles_sampler.md
#ifndef SOBFU_WARP_WY
#define SOBFU_WARP_WY 16
#endif
constexpr int kWarpWY = SOBFU_WARP_WY;
// the chip: workgroups of 8 waves that are resident at once when a CU holds `per_cu` of them (VGPRs / LDS / waves decide how many)
constexpr int kCUs = 256;
constexpr int wg_slots(int per_cu) { return kCUs * per_cu * 8 / kWY; }

// ---- what a launch is asked to produce ------------------------------------------------------------------------------------------
// A box of cells [x0, x1) x [y0, y1) x [z0, z1) of the (local) array a fused pass produces; direct: a THIN box, evaluated one
// lane per cell straight from the caches instead of by a z-march (the one-cell shells of a tile, halo messages).  Up to kMaxBoxes
// boxes per launch; empty boxes are skipped.
struct LaunchBox {
    int x0, x1, y0, y1, z0, z1;
    bool direct;
};
constexpr int kMaxBoxes = 6;  // of a launch descriptor and of the planned list the kernel gets
// A box of a tile's pass A.  dst != null: a PUSH box -- the cells of one halo message, whose results go to
// dst + 3 * ((x + ox) + px * ((y + oy) + py * (z + oz))): the neighbour's halo cells (peer-mapped) or a packed send buffer.
// A MARCHING push box may be larger than its message and serve the owned block too (which then leaves those cells out): only rows
// push_y0 <= y < push_y1 travel, and cells of planes local_z0 <= z < local_z1 are ALSO stored into this rank's own nabla_U.
struct TileLaunchBox {
    LaunchBox box;
    float* dst;
    int ox, oy, oz, px, py;
    int push_y0, push_y1, local_z0, local_z1;
};

// ---- the planned launch, as the kernels read it ---------------------------------------------------------------------------------
struct Box {
    int x0, x1, y0, y1, z0, z1;  // cells [x0, x1) x [y0, y1) x [z0, z1)
    int zc;                      // marching: planes per march (z-chunk); direct: wx, the lanes of a wave that run along x
    int kind;                    // 0 marching, 1 direct
    int wpg;                     // direct: waves of a workgroup that take cells (the others leave at once) -- see direct_wpg()
    int rem;                     // marching: the first `rem` z-chunks march zc + 1 planes (an even split of the planes over a chosen NUMBER of chunks)
    int pair;                    // marching, pass B: z-chunks march in alternating directions (even chunks top-down, odd ones bottom-up), so that
                                 // two neighbours start at -- or arrive at -- their common boundary TOGETHER: the 6 planes either side of it,
                                 // which both read, are fetched once where the two share an XCD (and its L2) instead of a march apart
};
struct BoxList {
    int n;
    int m0, m1;   // workgroups [m0, m1) belong to marching boxes, the rest to direct boxes
    Box b[kMaxBoxes];
    int first[kMaxBoxes + 1];  // first workgroup of box i; first[n] = workgroups in the launch
};
// where the cells of a PUSH box go (pass A of a multi-GPU tile: see tile_potential_gradient_kernel)
struct PushDst {
    float* base;             // null: the box is stored locally
    int ox, oy, oz, px, py;  // cell (x, y, z) -> base + 3 * ((x + ox) + px * ((y + oy) + py * (z + oz)))
    int y0, y1, lz0, lz1;    // marching push boxes: rows [y0, y1) travel; planes [lz0, lz1) are stored locally as well
};
constexpr int kMaxTileBoxes = 20;  // 18 messages + the owned block + one spare
struct TileBox {
    Box b;
    PushDst push;
};
struct TileBoxList {
    int n, n_push_wgs;  // workgroups [0, n_push_wgs) belong to push boxes
    TileBox b[kMaxTileBoxes];
    int first[kMaxTileBoxes + 1];
};

// ---- planning -------------------------------------------------------------------------------------------------------------------
// z-chunk length of a fused pass.  A launch has tiles * ceil(nz / zc) workgroups; `capacity` of them are resident at
// once on the chip (256 CUs x workgroups per CU allowed by VGPRs / LDS / waves).  Cost model: time ~ (1 + refill / zc)
// / utilisation, where utilisation = groups / (ceil(groups / capacity) * capacity) penalises a ragged last wave of
// workgroups (measured at 256^3, pass B: 768 groups = exactly 3 per CU: 166 us; 512 groups: 184 us; 1024: 195 us) and
// refill = planes re-read when a march starts (2 for pass A, 6 for pass B).  Small grids end up with many short
// marches, which is what the latency-bound regime wants (64^3: zc = 2 is 1.4x faster than zc = 8).
inline int env_zc(const char* env) {  // tuning override (SOBFU_ZC_A / SOBFU_ZC_B): planes per march, 0 = none
    const char* e = getenv(env);
    const int v   = e ? atoi(e) : 0;
    return v > 0 ? v : 0;
}
inline int pick_zc(int X, int Y, int nz, int ty, int capacity, int refill, const char* env) {
    if (const int v = env_zc(env)) return v < nz ? v : nz;
    const long tiles = (long) ((X + TX - 1) / TX) * ((Y + ty - 1) / ty);
    int best_zc = nz;
    double best = 1e30;
    for (int c = 1; c <= nz; ++c) {
        const int zc = (nz + c - 1) / c;
        if (zc < 2 && nz >= 2) break;
        const long groups = tiles * ((nz + zc - 1) / zc);
        const long waves  = (groups + capacity - 1) / capacity;
        const double util = (double) groups / (double) (waves * capacity);
        const double cost = (1.0 + (double) refill / zc) / util;
        if (cost < best - 1e-9) { best = cost; best_zc = zc; }
    }
    return best_zc;
}

// direct boxes: lanes of a wave that run along x, and the workgroups (of WY waves) the box needs
inline int direct_wx(int ex) {
    int wx = 1;
    while (wx < ex && wx < 64) wx *= 2;
    return wx;
}
// A wave of a box that is thin in x touches up to 64 / wx cache lines with EVERY load (its lanes sit in different rows), and the
// address unit of a CU takes them one line per cycle: eight such waves in one workgroup -- on one CU -- queue up behind each
// other (the one-column x shell of a 2 x 2 x 2 tile: 13.9 us as 32 full workgroups).  Such boxes get few working waves per
// workgroup, i.e. many small workgroups that the dispatcher spreads over all CUs.
// Only where the launch leaves the chip room (pass B of a tile: fewer workgroups than slots) -- in pass A, whose march fills every
// slot, a thousand one-wave workgroups in front of it cost more than they save (`spread` = false: full workgroups).
inline int direct_wpg(int wx, bool spread) { return spread ? std::max(1, std::min(kWY, wx / 4)) : kWY; }
inline int direct_groups(const LaunchBox& s, int wx, bool spread) {
    const int wyl = 64 / wx, wpg = direct_wpg(wx, spread);
    const long waves = (long) ((s.x1 - s.x0 + wx - 1) / wx) * ((s.y1 - s.y0 + wyl - 1) / wyl) * (s.z1 - s.z0);
    return (int) ((waves + wpg - 1) / wpg);
}
inline double box_cells(const LaunchBox& s) {
    return (s.x1 > s.x0 && s.y1 > s.y0 && s.z1 > s.z0) ? (double) (s.x1 - s.x0) * (s.y1 - s.y0) * (s.z1 - s.z0) : 0.0;
}
// geometry of one live box; returns its workgroups.  Marching boxes: zc_override > 0 fixes the planes per march; else, when the box's
// xy tiles fit the share of the chip it gets (`even`: launches that are one resident round -- multi-GPU tiles, cache-resident grids),
// the planes are split EVENLY over as many chunks as fill that share (chunk lengths differ by at most one plane: a launch of one
// round lasts as long as its longest march); else the cost model picks a chunk length (pick_zc).
inline int finish_box(Box& b, const LaunchBox& s, int ty, int share, int refill, int zc_override, const char* env, bool spread, bool even = false) {
    b.x0 = s.x0; b.x1 = s.x1; b.y0 = s.y0; b.y1 = s.y1; b.z0 = s.z0; b.z1 = s.z1;
    b.kind = s.direct ? 1 : 0;
    b.wpg = kWY;
    b.rem = 0;
    b.pair = 0;
    if (s.direct) {
        b.zc  = direct_wx(s.x1 - s.x0);
        b.wpg = direct_wpg(b.zc, spread);
        return direct_groups(s, b.zc, spread);
    }
    const int eu = s.x1 - s.x0, ev = s.y1 - s.y0, nz = s.z1 - s.z0;
    const int tiles = ((eu + TX - 1) / TX) * ((ev + ty - 1) / ty);
    int nch = 0;
    if (zc_override <= 0 && env_zc(env) == 0 && even && tiles <= share) nch = std::max(share / tiles, 1);
    if (nch > 0 && zc_override <= 0) {
        nch   = std::min(nch, std::max(nz / 2, 1));  // a march of one plane is all prologue
        b.zc  = nz / nch;
        b.rem = nz % nch;
        return tiles * nch;
    }
    b.zc = zc_override > 0 ? std::min(zc_override, nz) : pick_zc(eu, ev, nz, ty, share, refill, env);
    return tiles * ((nz + b.zc - 1) / b.zc);
}
// Fills the launch geometry of a box list: z-chunk per marching box (cost model above, the chip's capacity shared between the
// marching boxes; direct boxes are one short round trip and take no share) and the workgroup prefix -- marching boxes first.
// Returns the workgroups.
inline int finish_boxes(BoxList& L, const LaunchBox* boxes, int n, int ty, int capacity, int refill, const char* env, bool even = false) {
    L.n = 0;
    int live = 0;
    bool thin = false;
    for (int i = 0; i < n; ++i) {
        live += (box_cells(boxes[i]) > 0 && !boxes[i].direct) ? 1 : 0;
        thin = thin || (box_cells(boxes[i]) > 0 && boxes[i].direct);
    }
    // an even split fills the marching share exactly -- then the thin boxes' workgroups would start only when a march ends, and end the
    // launch: they keep a sixteenth of the slots (2 x 2 x 2 tile of 256^3: 15 chunks -> 480 + 288 workgroups, 43.0 us; 16 -> 512 + 288, 44.1)
    if (even && thin) capacity -= capacity / 16;
    int total = 0;
    L.m0 = L.m1 = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const bool direct_pass = pass == 1;  // marching boxes first
        if (!direct_pass) L.m0 = total;
        for (int i = 0; i < n && L.n < kMaxBoxes; ++i) {
            if (box_cells(boxes[i]) == 0 || boxes[i].direct != direct_pass) continue;
            // the chip's workgroup slots are shared equally between the marching boxes (the two plane ranges of an overlapped slab
            // schedule): a thin range is latency-critical, so it gets as many short marches as the big one gets long ones
            L.first[L.n] = total;
            total += finish_box(L.b[L.n], boxes[i], ty, std::max(capacity / std::max(live, 1), 1), refill, 0, env, true, even);
            ++L.n;
        }
        if (!direct_pass) L.m1 = total;
    }
    for (int k = L.n; k <= kMaxBoxes; ++k) L.first[k] = total;
    return total;
}

// Pass A of a multi-GPU tile (see tile_potential_gradient_kernel): the launch geometry of its box list.  The boxes with a
// destination (push boxes: direct, their result goes to `dst` only) are numbered first, then the others; returns the workgroups
// (< 0: too many boxes).  resident: the tile's state stays in the Infinity Cache (GridTraits)
inline int fill_tile_boxes(TileBoxList& L, const TileLaunchBox* boxes, int n, bool resident) {
    constexpr int TY = kRPT * kWY;
    L.n = 0;
    int live = 0, total = 0;
    for (int i = 0; i < n; ++i) live += (box_cells(boxes[i].box) > 0 && !boxes[i].box.direct && boxes[i].dst == nullptr) ? 1 : 0;
    for (int pass = 0; pass < 2; ++pass) {  // push boxes first
        for (int i = 0; i < n; ++i) {
            const TileLaunchBox& s = boxes[i];
            if ((s.dst != nullptr) != (pass == 0) || box_cells(s.box) == 0) continue;
            if (L.n >= kMaxTileBoxes) return -1;
            TileBox& t = L.b[L.n];
            L.first[L.n] = total;
            // z-chunks: a marching push box (a face with wide rows) marches up to 8 planes; the owned block of a cache-resident
            // tile is sized for TWO workgroups per CU -- the push boxes take slots too, and at that size 8-plane marches beat the 4-plane ones that
            // filling all four slots per CU would give (2 x 2 x 2 tile of 256^3: pass A 19.8 -> 19.1 us, 1 x 2 x 4: 18.9 -> 17.2)
            const int zc_box = (s.dst != nullptr && !s.box.direct) ? std::min(8, s.box.z1 - s.box.z0) : 0;
            total += finish_box(t.b, s.box, TY, std::max(wg_slots(resident ? 2 : 4) / std::max(live, 1), 1), 2, zc_box, "SOBFU_ZC_A", false);
            t.push.base = s.dst;
            t.push.ox = s.ox; t.push.oy = s.oy; t.push.oz = s.oz; t.push.px = s.px; t.push.py = s.py;
            t.push.y0 = s.push_y0; t.push.y1 = s.push_y1; t.push.lz0 = s.local_z0; t.push.lz1 = s.local_z1;
            ++L.n;
        }
        if (pass == 0) L.n_push_wgs = total;
    }
    for (int k = L.n; k <= kMaxTileBoxes; ++k) L.first[k] = total;
    return total;
}

// ---- the planners' entry points: the boxes of a launch descriptor -> the finished list; they return the workgroups -----------------
inline bool has_direct_box(const LaunchBox* boxes, int n) {
    bool direct = false;
    for (int i = 0; i < n; ++i) direct = direct || (boxes[i].direct && box_cells(boxes[i]) > 0);
    return direct;
}
// pass A, marching boxes only (fused_potential_gradient_kernel)
inline int plan_pass_a(BoxList& L, const LaunchBox* boxes, int n) {
    // <= 64 VGPR (the warping march included), 22 KB LDS: 4 workgroups of 8 waves per CU
    return finish_boxes(L, boxes, n, kRPT * kWY, wg_slots(4), 2, "SOBFU_ZC_A");
}
// the warping march of pass A (fused_potential_gradient_kernel<.., WARP>): tiles of 64 x kWarpWY cells, one row per wave
inline int plan_pass_a_warp(BoxList& L, const LaunchBox* boxes, int n) {
    // <= 64 VGPR: 8 waves per SIMD, 32 per CU -- 2 workgroups of 16 waves (39 KB LDS each)
    return finish_boxes(L, boxes, n, kRPT * kWarpWY, kCUs * 32 / kWarpWY, 2, "SOBFU_ZC_A");
}
// pass A of a launch that holds thin boxes: the tile kernel (no messages, no signalling, no gate) with a list of the call's own
// (< 0: too many boxes)
inline int plan_pass_a_thin(TileBoxList& L, const LaunchBox* boxes, int n, bool resident) {
    if (n > kMaxBoxes) return -1;
    TileLaunchBox tb[kMaxBoxes];
    for (int i = 0; i < n; ++i) tb[i] = TileLaunchBox{boxes[i], nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return fill_tile_boxes(L, tb, n, resident);
}
// pass B: m.pipe (pass_b_march) sets the chip's capacity and, with g.resident, the even split; the finished list completes m for stage 2
// of the choice (choose_pass_b) and sets Box::pair.  An empty launch (0 workgroups) leaves m as it was.
inline int plan_pass_b(BoxList& L, const LaunchBox* boxes, int n, const GridTraits& g, PassBMarch& m) {
    // workgroups a CU holds: <= 80 VGPR (launch bounds) and 32 - 48 KB LDS: 3 of 8 waves; the pipelined march (<= 128 VGPR): 2
    // cache-resident launches are ONE resident round of workgroups, which lasts as long as its longest march: the planes are
    // split evenly over as many z-chunks as fill the marching workgroups' share of the chip
    const int groups = finish_boxes(L, boxes, n, kRPT * kWY, wg_slots(m.pipe ? 2 : 3), 6, "SOBFU_ZC_B", g.resident && m.pipe);
    if (groups == 0) return 0;
    int zc_max = 0;
    for (int i = 0; i < L.n; ++i) {
        m.direct = m.direct || L.b[i].kind != 0;
        if (L.b[i].kind == 0) zc_max = std::max(zc_max, L.b[i].zc + (L.b[i].rem > 0 ? 1 : 0));  // the first `rem` chunks march one plane more
        if (L.b[i].kind == 0 && m.pipe && g.resident && SOBFU_PAIR_B) L.b[i].pair = 1;  // neighbouring z-chunks march towards / away from each other
    }
    m.long_marches = SOBFU_HLEAD > 0 && zc_max >= SOBFU_HLEAD_MIN_ZC;
    return groups;
}

}  // namespace sobfu_hip
