// The steps of X * Bm that xb_next (pls_amd/csrc/xb_route.hpp) plans for a call, without a GPU: tests/test_xb_route.py.
// stdin, one call per line:  N K C es ldx ldo x_vec out_vec num_cu xb4 ss denied
// stdout, one line per call: its steps under the fixed mask `denied` of refused routes, "; " between them, each
//   <kernel><selectors> [split y=<gridDim.y>] [+ finish] (columns) [gx gy lds kper ks sw ldp part_bytes bytes]
#include "../../pls_amd/csrc/xb_route.hpp"

#include <cstdio>
#include <iostream>
#include <string>

int main() {
    using namespace plsk;
    XbShape s{};
    long long N, ldx, ldo;
    int xv, ov, ss;
    unsigned denied;
    while (std::cin >> N >> s.K >> s.C >> s.es >> ldx >> ldo >> xv >> ov >> s.num_cu >> s.xb4 >> ss >> denied) {
        s.N = N; s.ldx = ldx; s.ldo = ldo; s.x_vec = xv != 0; s.out_vec = ov != 0; s.ss = ss != 0;
        std::string line;
        for (int c0 = 0; c0 < s.C;) {
            const XbStep st = xb_next(s, c0, denied);
            if (st.use < 1 || st.gx < 1 || st.gy < 1 || (denied & xb_bit(st.route))) {
                std::printf("bad step at column %d\n", c0);
                return 1;
            }
            static const char *const names[] = {"xb_kernel", "xb_wide", "xb_wide", "xb_split", "xb_mfma_lds", "xb_mfma4", "xb_mfma4w", "xb_mfma4w"};
            char buf[256];
            std::string t = names[st.route];
            std::snprintf(buf, sizeof buf, "<%d,%d%s%s>", st.vec, st.sel, st.route == XB_WIDE2 ? ",2" : "", st.ss ? ",ss" : "");
            t += buf;
            if (st.route == XB_MFMA4W_SPLIT) t += " split y=" + std::to_string(st.gy);
            if (st.route == XB_SPLIT || st.route == XB_MFMA4W_SPLIT) t += " + finish";
            std::snprintf(buf, sizeof buf, " (%d) [%u %u %zu %d %d %d %lld %zu %lld]", st.use, st.gx, st.gy, st.lds, st.kper, st.ks, st.sw,
                          (long long)st.ldp, st.part_bytes, (long long)st.bytes);
            line += (line.empty() ? "" : "; ") + t + buf;
            c0 += st.use;
        }
        std::printf("%s\n", line.c_str());
    }
    return 0;
}
