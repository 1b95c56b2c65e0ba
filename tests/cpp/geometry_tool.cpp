// CPU-only driver of sobfu_amd/csrc/sobfu_geometry.hpp and sobfu_tile_layout.hpp (tests/test_launch_geometry.py): the geometry of a
// fused launch and of a multi-GPU tile.  The tuning environment is the process's own.  One case per input line, one answer line each:
//   A X Y Z n {x0 x1 y0 y1 z0 z1 direct} * n            pass A of a launch descriptor (thin boxes: the tile kernel's list)
//   B X Y Z resident pipe n {x0 x1 y0 y1 z0 z1 direct} * n   pass B; resident / pipe as launch_pass_b derives them
//   T X Y Z n {x0 x1 y0 y1 z0 z1 direct dst ox oy oz px py push_y0 push_y1 local_z0 local_z1} * n    a tile's planned pass A
//   L X Y Z Px Py Pz rank                               the rank's layout, its messages and their bookkeeping
//   P X Y Z Px Py Pz rank connected debug_skip          pass A's push boxes and the slab schedules' plane ranges
// Answers: "groups G m0 m1 first f.. | x0 x1 y0 y1 z0 z1 zc kind wpg rem pair | .." (B adds "direct long" in front of the boxes),
// for tile lists "groups G push N first f.. | <box> base ox oy oz px py y0 y1 lz0 lz1 | ..", or "refused".  Pointers are printed as
// integers; a connected P case takes fake destinations 4096 * (message + 1) (+ 2^30 for the second nabla_U half), the send buffer is 2^32.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "sobfu_tile_layout.hpp"

using namespace sobfu_hip;

static std::ostream& operator<<(std::ostream& o, const Box& b) {
    return o << b.x0 << ' ' << b.x1 << ' ' << b.y0 << ' ' << b.y1 << ' ' << b.z0 << ' ' << b.z1 << ' ' << b.zc << ' ' << b.kind << ' ' << b.wpg << ' '
             << b.rem << ' ' << b.pair;
}
static std::ostream& operator<<(std::ostream& o, const LaunchBox& b) {
    return o << b.x0 << ' ' << b.x1 << ' ' << b.y0 << ' ' << b.y1 << ' ' << b.z0 << ' ' << b.z1 << ' ' << (b.direct ? 1 : 0);
}
static void print(std::ostream& o, const BoxList& L, int groups, const PassBMarch* m) {
    o << "groups " << groups << ' ' << L.m0 << ' ' << L.m1 << " first";
    for (int k = 0; k <= kMaxBoxes; ++k) o << ' ' << L.first[k];
    if (m) o << " | " << m->direct << ' ' << m->long_marches;
    for (int i = 0; i < L.n; ++i) o << " | " << L.b[i];
}
static void print(std::ostream& o, const TileBoxList& L, int groups) {
    if (groups < 0) {
        o << "refused";
        return;
    }
    o << "groups " << groups << " push " << L.n_push_wgs << " first";
    for (int k = 0; k <= kMaxTileBoxes; ++k) o << ' ' << L.first[k];
    for (int i = 0; i < L.n; ++i) {
        const PushDst& p = L.b[i].push;
        o << " | " << L.b[i].b << ' ' << (unsigned long long) (uintptr_t) p.base << ' ' << p.ox << ' ' << p.oy << ' ' << p.oz << ' ' << p.px << ' ' << p.py
          << ' ' << p.y0 << ' ' << p.y1 << ' ' << p.lz0 << ' ' << p.lz1;
    }
}
static LaunchBox read_box(std::istream& in) {
    LaunchBox b{};
    int direct = 0;
    in >> b.x0 >> b.x1 >> b.y0 >> b.y1 >> b.z0 >> b.z1 >> direct;
    b.direct = direct != 0;
    return b;
}
static void print(std::ostream& o, const TileLaunchBox& b) {
    o << " | " << b.box << ' ' << (unsigned long long) (uintptr_t) b.dst << ' ' << b.ox << ' ' << b.oy << ' ' << b.oz << ' ' << b.px << ' ' << b.py << ' '
      << b.push_y0 << ' ' << b.push_y1 << ' ' << b.local_z0 << ' ' << b.local_z1;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream out;
        std::string k;
        if (!(in >> k)) continue;
        int X, Y, Z;
        in >> X >> Y >> Z;
        if (k == "A" || k == "B") {
            int resident = 0, pipe = 0, n = 0;
            if (k == "B") in >> resident >> pipe;
            in >> n;
            std::vector<LaunchBox> boxes;
            for (int i = 0; i < n; ++i) boxes.push_back(read_box(in));
            if (k == "A" && has_direct_box(boxes.data(), n)) {
                TileBoxList L{};
                print(out, L, plan_pass_a_thin(L, boxes.data(), n, grid_traits(X, Y, Z, X, Y, Z, env_cache_cells()).resident));
            } else if (k == "A") {
                BoxList L{};
                print(out, L, plan_pass_a(L, boxes.data(), n), nullptr);
            } else {
                GridTraits g = grid_traits(X, Y, Z, X, Y, Z, env_cache_cells());
                g.resident = resident != 0;
                PassBMarch m;
                m.pipe = pipe != 0;
                BoxList L{};
                const int groups = plan_pass_b(L, boxes.data(), n, g, m);
                print(out, L, groups, &m);
            }
        } else if (k == "T") {
            int n = 0;
            in >> n;
            std::vector<TileLaunchBox> boxes;
            for (int i = 0; i < n; ++i) {
                TileLaunchBox b{};
                b.box = read_box(in);
                unsigned long long dst = 0;
                in >> dst >> b.ox >> b.oy >> b.oz >> b.px >> b.py >> b.push_y0 >> b.push_y1 >> b.local_z0 >> b.local_z1;
                b.dst = (float*) (uintptr_t) dst;
                boxes.push_back(b);
            }
            TileBoxList L{};
            print(out, L, fill_tile_boxes(L, boxes.data(), n, grid_traits(X, Y, Z, X, Y, Z, env_cache_cells()).resident));
        } else if (k == "L" || k == "P") {
            int P[3], rank;
            in >> P[0] >> P[1] >> P[2] >> rank;
            const int dims[3] = {X, Y, Z};
            const TileLay lay = make_layout(dims, P, rank);
            if (!lay.ok) {
                std::cout << "refused\n";
                continue;
            }
            const TileMsgs mm = make_messages(lay);
            if (k == "L") {
                out << "P " << lay.P[0] << ' ' << lay.P[1] << ' ' << lay.P[2] << " c " << lay.c[0] << ' ' << lay.c[1] << ' ' << lay.c[2];
                for (const AxisLay& a : lay.a)
                    out << " | " << a.g0 << ' ' << a.g1 << ' ' << a.lo << ' ' << a.hi << ' ' << a.L << ' ' << a.o0 << ' ' << a.o1 << ' ' << a.base;
                out << " | msgs " << mm.msgs.size() << " packed " << mm.n_packed << " floats " << mm.floats;
                for (size_t i = 0; i < lay.msgs.size(); ++i) {
                    const MsgGeom& m = lay.msgs[i];
                    out << " | " << m.peer;
                    for (int v : m.sb) out << ' ' << v;
                    for (int v : m.rb) out << ' ' << v;
                    out << ' ' << mm.msgs[i].peer << ' ' << mm.msgs[i].send_off << ' ' << mm.msgs[i].recv_off << ' ' << mm.msgs[i].count;
                }
                out << " | inplace " << mm.zmsgs.size();
                for (const sobfu_hip_tiled_msg& m : mm.zmsgs) out << " | " << m.peer << ' ' << m.send_off << ' ' << m.recv_off << ' ' << m.count;
                // the scatter table: its length and an order-sensitive checksum, sum of (i + 1) * entry i modulo 2^64
                uint64_t h = 0;
                const std::vector<uint32_t> tab = lay.slab() ? std::vector<uint32_t>() : scatter_table(lay, mm.n_packed);
                for (size_t i = 0; i < tab.size(); ++i) h += (uint64_t) (i + 1) * tab[i];
                out << " | scatter " << tab.size() << ' ' << h;
            } else {
                int connected = 0, debug_skip = 0;
                in >> connected >> debug_skip;
                std::vector<float*> d0, d1;
                std::vector<TileLay> peers;
                for (size_t i = 0; i < lay.msgs.size(); ++i) {
                    d0.push_back((float*) (uintptr_t) (4096 * (i + 1)));
                    d1.push_back((float*) (uintptr_t) (4096 * (i + 1) + ((size_t) 1 << 30)));
                    peers.push_back(make_layout(dims, P, lay.msgs[i].peer));
                }
                float* sendbuf = (float*) (uintptr_t) ((size_t) 1 << 32);
                const PushBoxes pb = connected ? push_boxes(lay, mm, sendbuf, d0.data(), d1.data(), peers.data(), debug_skip)
                                               : push_boxes(lay, mm, sendbuf, nullptr, nullptr, nullptr, debug_skip);
                const PlaneRanges r = plane_ranges(lay);
                out << "planes " << r.a_lo << ' ' << r.a_hi << ' ' << r.b_lo << ' ' << r.b_hi << ' ' << r.b_first << ' ' << r.b_last;
                out << " | own " << pb.own << " | whole " << pb.whole;
                for (int h = 0; h < 2; ++h) {
                    out << " | half " << h << ' ' << pb.push[h].size();
                    for (const TileLaunchBox& b : pb.push[h]) print(out, b);
                }
            }
        } else {
            std::cerr << "unknown case: " << line << "\n";
            return 2;
        }
        std::cout << out.str() << "\n";
    }
    return 0;
}
