// The geometry of a multi-GPU tile: which cells a rank owns, which cells each of its up to 18 halo messages carries and where they
// land, how the messages are packed, which push box of pass A stands in for which part of the owned block, and the plane ranges of
// the slab schedules.  Host-only and free of HIP headers (tests/cpp/geometry_tool.cpp compiles it with g++); tiled_capi.hip keeps one
// TileLay per handle and reads everything through it.  sobfu_amd/tiled.py (TileLayout) states the same layout independently;
// tests/test_launch_geometry.py compares the two.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sobfu_geometry.hpp"

namespace sobfu_hip {

constexpr int kHalo = 4;

// The bits of SOBFU_TILED_DEBUG_SKIP (read once, when a handle is created): pieces of an iteration left out, for timing experiments
// only -- the results are wrong.  The first seven are read by the loop (tiled_capi.hip), the last three by push_boxes below.
enum DebugSkip : int {
    kSkipPushBoxes    = 1,    // pass A of the tile path launches the whole owned block alone, without its push boxes
    kSkipShells       = 2,    // pass B of the tile path without its thin x / y shells
    kSkipPassA        = 4,    // no pass A (tile path)
    kSkipPassB        = 8,    // no pass B (tile path)
    kSkipOwnedB       = 16,   // pass B without the owned block
    kSkipYShells      = 32,   // pass B without the y shells
    kSkipXShells      = 64,   // pass B without the x shells
    kSkipThinPush     = 128,  // no thin push boxes (x faces, edges, corners)
    kSkipMarchedPush  = 256,  // no marched push boxes (y / z faces)
    kMarchedHomeOnly  = 512,  // the marched push boxes store at home only
};

// The layout of ANY rank's tile (a rank also needs its neighbours': where their halo cells sit in their arrays).
// tile grid P, the rank's tile coordinates c; per axis: owned global range [g0, g1), halo cells lo / hi, local extent L,
// owned local range [o0, o1), global coordinate `base` of local cell 0
struct AxisLay {
    int g0, g1, lo, hi, L, o0, o1, base;
};
struct MsgGeom {
    int peer, dir[3];
    int sb[6], rb[6];  // cells sent / halo cells received (local cells of THIS rank)
    size_t cells;
    bool z_face() const { return dir[0] == 0 && dir[1] == 0 && dir[2] != 0; }
};
struct TileLay {
    int P[3], c[3];
    AxisLay a[3];
    std::vector<MsgGeom> msgs;
    bool ok = true;
    bool slab() const { return P[0] == 1 && P[1] == 1; }  // on the RCCL transport halos are whole planes and travel in place (no pack / unpack)
    size_t cells() const { return (size_t) a[0].L * a[1].L * a[2].L; }
};
inline TileLay make_layout(const int dims[3], const int P[3], int rank) {
    TileLay t;
    const int c[3] = {rank % P[0], (rank / P[0]) % P[1], rank / (P[0] * P[1])};  // x fastest
    for (int k = 0; k < 3; ++k) {
        t.P[k] = P[k];
        t.c[k] = c[k];
        const int base = dims[k] / P[k], rem = dims[k] % P[k];  // the cells of an axis are split as evenly as possible
        AxisLay& a = t.a[k];
        a.g0   = c[k] * base + std::min(c[k], rem);
        a.g1   = a.g0 + base + (c[k] < rem ? 1 : 0);
        a.lo   = c[k] > 0 ? kHalo : 0;
        a.hi   = c[k] < P[k] - 1 ? kHalo : 0;
        a.L    = (a.g1 - a.g0) + a.lo + a.hi;
        a.o0   = a.lo;
        a.o1   = a.lo + (a.g1 - a.g0);
        a.base = a.g0 - a.lo;
        if (P[k] > 1 && base < kHalo) t.ok = false;  // a tile must own at least a halo's worth of cells per split axis
    }
    // halo messages: every face neighbour (one non-zero offset) and edge neighbour (two); corners are never read.  Along an
    // axis with offset +1 the 4 owned cells next to that face are sent and the 4 halo cells beyond it received; along an
    // axis with offset 0 the owned range (the same on both sides, as the neighbour shares this coordinate).
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int dl[3] = {dx, dy, dz};
                const int nnz = (dx != 0) + (dy != 0) + (dz != 0);
                if (nnz < 1 || nnz > 2) continue;
                bool inside = true;
                for (int k = 0; k < 3; ++k) inside = inside && c[k] + dl[k] >= 0 && c[k] + dl[k] < P[k];
                if (!inside) continue;
                MsgGeom m;
                m.cells = 1;
                for (int k = 0; k < 3; ++k) {
                    const AxisLay& a = t.a[k];
                    m.dir[k] = dl[k];
                    if (dl[k] > 0) { m.sb[2 * k] = a.o1 - kHalo; m.sb[2 * k + 1] = a.o1; m.rb[2 * k] = a.o1; m.rb[2 * k + 1] = a.o1 + kHalo; }
                    else if (dl[k] < 0) { m.sb[2 * k] = a.o0; m.sb[2 * k + 1] = a.o0 + kHalo; m.rb[2 * k] = a.o0 - kHalo; m.rb[2 * k + 1] = a.o0; }
                    else { m.sb[2 * k] = m.rb[2 * k] = a.o0; m.sb[2 * k + 1] = m.rb[2 * k + 1] = a.o1; }
                    m.cells *= (size_t) (m.sb[2 * k + 1] - m.sb[2 * k]);
                }
                m.peer = (c[0] + dx) + P[0] * ((c[1] + dy) + P[1] * (c[2] + dz));
                t.msgs.push_back(m);
            }
    // the z FACES go last: on the packed (RCCL / callback) transports of a 3-D tile they travel IN PLACE as whole padded planes of the
    // array (see exchange_packed), so the messages that do use the packed buffers are a prefix of the list and of the buffers
    std::stable_partition(t.msgs.begin(), t.msgs.end(), [](const MsgGeom& m) { return !m.z_face(); });
    return t;
}

// ---- the messages of one exchange -----------------------------------------------------------------------------------------------
// One per face / edge neighbour, packed one after the other (same offsets on both sides).  Packed transports of a 3-D tile: the first
// n_packed messages travel through the buffers, the z faces behind them in place (zmsgs: offsets into the nabla_U array itself -- 4
// whole padded planes out of the owned rim, 4 into the halo).
struct TileMsgs {
    std::vector<sobfu_hip_tiled_msg> msgs, zmsgs;
    int n_packed   = 0;
    size_t floats  = 0;  // of a packed buffer that holds every message
};
inline TileMsgs make_messages(const TileLay& lay) {
    TileMsgs r;
    const bool slab = lay.slab();
    for (const MsgGeom& g : lay.msgs) {
        sobfu_hip_tiled_msg m;
        m.peer     = g.peer;
        m.send_off = m.recv_off = r.floats;
        m.count    = g.cells * 3;
        r.floats += m.count;
        r.msgs.push_back(m);
        if (g.z_face() && !slab) {  // the neighbour across a z face shares this tile's x / y layout: whole planes of the array match
            const size_t plane_f = (size_t) lay.a[0].L * lay.a[1].L * 3;
            r.zmsgs.push_back(sobfu_hip_tiled_msg{g.peer, plane_f * (size_t) g.sb[4], plane_f * (size_t) g.rb[4], plane_f * (size_t) kHalo});
        } else if (!g.z_face()) {
            r.n_packed += 1;  // (z faces are last in the list)
        }
    }
    if (slab) r.n_packed = (int) r.msgs.size();  // (slabs never take the packed path; keep the count meaningful)
    return r;
}
// where every cell of the packed receive buffer goes (x fastest inside a message box): the cell index in the local array
inline std::vector<uint32_t> scatter_table(const TileLay& lay, int n_packed) {
    std::vector<uint32_t> tab;
    for (int i = 0; i < n_packed; ++i) {
        const int* b = lay.msgs[i].rb;
        for (int z = b[4]; z < b[5]; ++z)
            for (int y = b[2]; y < b[3]; ++y)
                for (int x = b[0]; x < b[1]; ++x) tab.push_back((uint32_t) ((size_t) x + (size_t) lay.a[0].L * ((size_t) y + (size_t) lay.a[1].L * (size_t) z)));
    }
    return tab;
}
// the first n messages' send (or receive) boxes as launch_msg_copy takes them: 6 ints each
inline std::vector<int> flat_boxes(const TileLay& lay, int n, bool recv) {
    std::vector<int> v;
    for (int i = 0; i < n; ++i) v.insert(v.end(), recv ? lay.msgs[i].rb : lay.msgs[i].sb, (recv ? lay.msgs[i].rb : lay.msgs[i].sb) + 6);
    return v;
}

// ---- plane ranges of the z-slab schedules -----------------------------------------------------------------------------------------
// pass A: [a_lo, a_hi) are the planes away from an interior face (the boundary planes next to it go first, so that the exchange can
// start); pass B: [b_lo, b_hi) the planes whose +-3 taps are owned, [b_first, b_last) everything out to owned +-1
struct PlaneRanges {
    int a_lo, a_hi, b_lo, b_hi, b_first, b_last;
};
inline PlaneRanges plane_ranges(const TileLay& lay) {
    const AxisLay& z = lay.a[2];
    const int lo = z.o0, hi = z.o1, H = kHalo;
    PlaneRanges r;
    r.a_lo = z.lo ? std::min(lo + H, hi) : lo; r.a_hi = z.hi ? std::max(hi - H, r.a_lo) : hi;
    r.b_lo = z.lo ? std::min(lo + 3, hi) : lo; r.b_hi = z.hi ? std::max(hi - 3, r.b_lo) : hi;
    r.b_first = z.lo ? lo - 1 : lo; r.b_last = z.hi ? hi + 1 : hi;
    return r;
}

// ---- pass A's boxes ---------------------------------------------------------------------------------------------------------------
// One push box per message, then the owned block.  Destinations: the peers' halo cells when connected (dst0 / dst1: per message, for
// the two nabla_U halves; peers[i]: the layout of message i's peer), else the packed send buffer (sendbuf + the message's offset).
// Neither (dst0 == dst1 == null) on a 3-D tile: a packed transport, whose z faces leave in place.
struct PushBoxes {
    std::vector<TileLaunchBox> push[2];  // per nabla_U half
    LaunchBox own;                       // the owned block, shrunk by the faces that store at home
    LaunchBox whole;                     // the whole owned block (launches without messages)
};
inline PushBoxes push_boxes(const TileLay& lay, const TileMsgs& mm, float* sendbuf, float* const* dst0, float* const* dst1, const TileLay* peers,
                            int debug_skip) {
    // The y and z FACES are pushed by short marches whose cells the owned block would compute a second time.  Instead such a box
    // stands in for the owned block on its cells (it stores them at home too) and the owned block shrinks: by the 4 rim planes
    // along z, by a whole 8-row tile along y (the face box then marches 8 rows, of which the 4 rim rows travel).  Where face
    // boxes meet, the z box is the one that stores at home.  The x face (4 cells of a 64-lane row: lane per cell) and the edge
    // strips stay push-only: shrinking the owned block by 4 columns would not save it a single workgroup.  Measured (one box, A/B):
    // 1 x 1 x 8 slabs of 256^3 43.1 -> 41.6 us per iteration; 2 x 2 x 2 and 1 x 2 x 4 tiles unchanged (43.4 / 44.7).
    const AxisLay &ax = lay.a[0], &ay = lay.a[1], &az = lay.a[2];
    const int ny_nb = (ay.lo ? 1 : 0) + (ay.hi ? 1 : 0), nz_nb = (az.lo ? 1 : 0) + (az.hi ? 1 : 0);
    const bool wide = (ax.o1 - ax.o0) >= 64;  // rows wide enough for the faces to be MARCHED (thin rows: lane per cell, push-only)
    // packed (RCCL / callback) transports of a 3-D tile: the z faces leave IN PLACE, straight out of the owned block's rim planes -- no
    // push box evaluates them and the owned block keeps those planes
    const bool z_inplace = dst0 == nullptr && dst1 == nullptr && !lay.slab() && !mm.zmsgs.empty();
    const bool z_home = !z_inplace && wide && nz_nb > 0 && (az.o1 - az.o0) > kHalo * nz_nb;
    const bool y_home = wide && ny_nb > 0 && (ay.o1 - ay.o0) > 8 * ny_nb;
    const int iz0 = az.o0 + ((z_home && az.lo) ? kHalo : 0), iz1 = az.o1 - ((z_home && az.hi) ? kHalo : 0);  // planes the z boxes leave
    const int iy0 = ay.o0 + ((y_home && ay.lo) ? 8 : 0), iy1 = ay.o1 - ((y_home && ay.hi) ? 8 : 0);
    PushBoxes r;
    for (int h = 0; h < 2; ++h) {
        std::vector<TileLaunchBox>& v = r.push[h];
        for (size_t i = 0; i < lay.msgs.size(); ++i) {
            const MsgGeom& m = lay.msgs[i];
            TileLaunchBox b{};
            // wide rows (y / z faces): a short march costs a fifth of the loads of a lane-per-cell evaluation (1 x 1 x 8 slabs: pass A
            // 26.6 -> 18.4 us); thin in x: direct
            const bool march = (m.sb[1] - m.sb[0]) >= 64;
            b.box = LaunchBox{m.sb[0], m.sb[1], m.sb[2], m.sb[3], m.sb[4], m.sb[5], !march};
            b.push_y0 = m.sb[2]; b.push_y1 = m.sb[3];
            const bool face_z = march && m.dir[0] == 0 && m.dir[1] == 0 && m.dir[2] != 0, face_y = march && m.dir[0] == 0 && m.dir[2] == 0 && m.dir[1] != 0;
            if (face_z && z_home) { b.local_z0 = m.sb[4]; b.local_z1 = m.sb[5]; }
            if (face_y && y_home) {
                if (m.dir[1] > 0) b.box.y0 = ay.o1 - 8; else b.box.y1 = ay.o0 + 8;
                b.local_z0 = iz0; b.local_z1 = iz1;
            }
            if (z_inplace && m.dir[0] == 0 && m.dir[1] == 0 && m.dir[2] != 0) continue;
            if ((!march && (debug_skip & kSkipThinPush)) || (march && (debug_skip & kSkipMarchedPush))) continue;
            if (march && (debug_skip & kMarchedHomeOnly)) b.push_y1 = b.push_y0;
            float* const* dst = h ? dst1 : dst0;
            if (dst && dst[i]) {  // the matching message of the peer: direction -dir; its receive box is where these cells live there
                const TileLay& pl = peers[i];
                const MsgGeom* pm = nullptr;
                for (const MsgGeom& g : pl.msgs)
                    if (g.dir[0] == -m.dir[0] && g.dir[1] == -m.dir[1] && g.dir[2] == -m.dir[2]) pm = &g;
                b.dst = dst[i];
                b.ox = pm->rb[0] - m.sb[0]; b.oy = pm->rb[2] - m.sb[2]; b.oz = pm->rb[4] - m.sb[4];
                b.px = pl.a[0].L; b.py = pl.a[1].L;
            } else {
                b.dst = sendbuf + mm.msgs[i].send_off;
                b.ox = -m.sb[0]; b.oy = -m.sb[2]; b.oz = -m.sb[4];
                b.px = m.sb[1] - m.sb[0]; b.py = m.sb[3] - m.sb[2];
            }
            v.push_back(b);
        }
    }
    r.own   = LaunchBox{ax.o0, ax.o1, iy0, iy1, iz0, iz1, false};
    r.whole = LaunchBox{ax.o0, ax.o1, ay.o0, ay.o1, az.o0, az.o1, false};
    return r;
}

}  // namespace sobfu_hip
