// CPU-only driver of sobfu_amd/csrc/sobfu_variant.hpp (tests/test_variant_choice.py): which instantiation of a fused pass a launch takes.
// The tuning environment is the process's own.  One case per input line:
//   A X Y Z compact warp tile                                  -> "A|T compact nt warp" (T: the tile kernel) or "refused <code>"
//   B X Y Z pX pY pZ compact updates direct long sys apply     -> "B updates compact direct idx32 lead nt pipe ntbuf apply" or "refused <code>"
//   W X Y Z                                                    -> "warp" or "stream" (loop_warps_in_pass_a)
// `variant_tool --table` prints the rows of the three tables in the same form.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "sobfu_variant.hpp"

using namespace sobfu_hip;

static std::string fmt(char kind, const PassAVariant& v) {
    char b[64];
    snprintf(b, sizeof b, "%c %d %d %d", kind, v.compact, v.nt, v.warp);
    return b;
}
static std::string fmt(const PassBVariant& v) {
    char b[64];
    snprintf(b, sizeof b, "B %d %d %d %d %d %d %d %d %d", v.updates, v.compact, v.direct, v.idx32, v.lead, v.nt, v.pipe, v.ntbuf, v.apply);
    return b;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--table") == 0) {
        for (const PassAVariant& v : kPassATable) std::cout << fmt('A', v) << "\n";
        for (const PassAVariant& v : kTilePassATable) std::cout << fmt('T', v) << "\n";
        for (const PassBVariant& v : kPassBTable) std::cout << fmt(v) << "\n";
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string k, out;
        if (!(in >> k)) continue;
        int rc = 0;
        if (k == "A") {
            int X, Y, Z, compact, warp, tile;
            in >> X >> Y >> Z >> compact >> warp >> tile;
            PassAVariant v{};
            rc = choose_pass_a(grid_traits(X, Y, Z, X, Y, Z, env_cache_cells()), compact, warp, tile, &v);
            out = fmt(tile ? 'T' : 'A', v);
        } else if (k == "B") {
            int X, Y, Z, pX, pY, pZ, compact, updates, direct, long_marches, sys, apply;
            in >> X >> Y >> Z >> pX >> pY >> pZ >> compact >> updates >> direct >> long_marches >> sys >> apply;
            const GridTraits g = grid_traits(X, Y, Z, pX, pY, pZ, env_cache_cells(), env_pipe_b());
            const PassBAsk ask{compact != 0, updates != 0, sys != 0, apply != 0};
            PassBMarch m;
            PassBVariant v{};
            rc = pass_b_march(g, ask, &m);
            m.direct       = direct != 0;
            m.long_marches = long_marches != 0;
            if (rc == 0) rc = choose_pass_b(g, ask, m, &v);
            out = fmt(v);
        } else if (k == "W") {
            int X, Y, Z;
            in >> X >> Y >> Z;
            out = loop_warps_in_pass_a(X, Y, Z) ? "warp" : "stream";
        } else {
            std::cerr << "unknown case: " << line << "\n";
            return 2;
        }
        std::cout << (rc != 0 ? "refused " + std::to_string(rc) : out) << "\n";
    }
    return 0;
}
