// xdiagmiss_geom_of (pls_amd/csrc/xdiagmiss_layout.hpp) on the CPU: the route and the tile rows every case of
// tests/test_xdiag_missing_ref.py claims, the on-chip budget of the tile, the K split and the workspace.  Includes only that
// header; tests/test_xdiagmiss_layout.py builds it with ASan + UBSan and feeds it the cases.
// stdin: one case per line "name N K A es route rt" (route 0 resident / 1 streaming; rt 0 on the streaming route), 256 CUs.
// stdout: per case and alignment "name aligned route rt S kper ws_bytes split_S tail_lo tail_hi" (the last three: the K ranges of
// miss_row_split at this shape and the fewest / most columns a lane owns in the last one), then "swept <n>" for the shapes of the
// sweep below and "split <n>" for the shapes on which miss_geom_of and xdiagmiss_geom_of are held to miss_row_split
// (miss_layout.hpp).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pls_amd/csrc/xdiagmiss_layout.hpp"

using plsk::i64;

static int failures = 0;
#define EXPECT(cond, ...)                    \
    do {                                     \
        if (!(cond)) {                       \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");      \
            ++failures;                      \
        }                                    \
    } while (0)

// the invariants of any geometry; touches both ends of every workspace field in a host image when the workspace is small
static void invariants(const char *name, i64 N, i64 K, i64 A, int es, int cu, bool aligned, bool force) {
    const plsk::XdmGeom g = plsk::xdiagmiss_geom_of(N, K, A, es, cu, aligned, force);
    EXPECT(g.vec == (aligned ? 16 / es : 1), "%s: vec %d", name, g.vec);
    EXPECT(g.ws_bytes > 0 && g.ws_bytes < ((i64)4 << 30), "%s: workspace of %lld bytes", name, (long long)g.ws_bytes);
    if (force) EXPECT(g.route == plsk::XDM_STREAM, "%s: forced to stream, route %d", name, g.route);
    if (g.route == plsk::XDM_RESIDENT) {
        EXPECT(g.rt >= plsk::XDM_RT_MIN && g.rt <= plsk::XDM_RT_MAX && (g.rt & (g.rt - 1)) == 0, "%s: tile rows %d", name, g.rt);
        EXPECT(g.rt >= g.vec && plsk::WG % g.rt == 0, "%s: tile rows %d against the workgroup", name, g.rt);
        EXPECT(g.lds_bytes == (i64)g.rt * K * 8 && g.lds_bytes <= plsk::XDM_TILE_BYTES, "%s: tile of %lld bytes", name, (long long)g.lds_bytes);
        // two workgroups, each with its tile and its hand-over, on one CU
        EXPECT(2 * (g.lds_bytes + plsk::XDM_HAND_BYTES) <= plsk::XDM_LDS_CU, "%s: two tiles of %lld bytes exceed a CU's LDS", name, (long long)g.lds_bytes);
        EXPECT(g.ntiles * g.rt >= N && (g.ntiles - 1) * g.rt < N, "%s: %lld tiles of %d rows for %lld rows", name, (long long)g.ntiles, g.rt, (long long)N);
        EXPECT(g.ntiles >= cu, "%s: %lld tiles leave CUs idle", name, (long long)g.ntiles);
        EXPECT(g.S == 1 && g.kper == K, "%s: the resident route does not split K", name);
    } else {
        const int RL = 1 << g.lrl, CL = plsk::WG >> g.lrl;
        EXPECT(RL * CL == plsk::WG, "%s: lanes", name);
        EXPECT(g.nrb * RL * g.vec >= N && (g.nrb - 1) * RL * g.vec < N, "%s: %lld row blocks", name, (long long)g.nrb);
        EXPECT(g.S >= 1 && g.S <= 65535 && g.kper >= 1, "%s: S %d kper %d", name, g.S, g.kper);
        EXPECT((i64)g.S * g.kper >= K && (i64)(g.S - 1) * g.kper < K, "%s: %d ranges of %d columns do not cover %lld exactly", name, g.S, g.kper, (long long)K);
        EXPECT(g.S == 1 || g.kper % CL == 0, "%s: a range of %d columns for %d column lanes", name, g.kper, CL);
    }
    // the fields in order, 16-byte aligned, inside the workspace
    const i64 offs[] = {g.o_sd, g.o_q0, g.o_qd, g.o_part, g.o_red, g.o_tv, g.ws_bytes};
    const i64 need[] = {N * A * 8, N * 8, N * A * 8, g.route == plsk::XDM_STREAM ? (i64)g.S * N * plsk::XDM_PART * 8 : 0,
                        (i64)plsk::XDM_RED_SLICES * (2 * A + 1) * 8, A * 8};
    EXPECT(offs[0] == 0, "%s: first field", name);
    for (int i = 0; i < 6; ++i) {
        EXPECT(offs[i] % 16 == 0, "%s: field %d at %lld", name, i, (long long)offs[i]);
        EXPECT(offs[i + 1] - offs[i] >= need[i] && offs[i + 1] - offs[i] < need[i] + 16, "%s: field %d has %lld bytes, needs %lld", name, i,
               (long long)(offs[i + 1] - offs[i]), (long long)need[i]);
    }
    if (g.ws_bytes <= (64 << 20)) {
        std::vector<unsigned char> ws((size_t)g.ws_bytes, 0);
        for (int i = 0; i < 6; ++i)
            if (need[i] > 0) {
                ws[(size_t)offs[i]] += 1;
                ws[(size_t)(offs[i] + need[i] - 1)] += 1;
            }
    }
}

int main() {
    const int cu = 256;
    char name[128];
    long long N, K, A;
    int es, route, rt;
    while (std::scanf("%127s %lld %lld %lld %d %d %d", name, &N, &K, &A, &es, &route, &rt) == 7) {
        for (int al = 0; al < 2; ++al) {
            const plsk::XdmGeom g = plsk::xdiagmiss_geom_of(N, K, A, es, cu, al != 0);
            EXPECT(g.route == route, "%s: claims route %d, the header says %d", name, route, g.route);
            EXPECT(g.route != plsk::XDM_RESIDENT || g.rt == rt, "%s: claims %d tile rows, the header says %d", name, rt, g.rt);
            invariants(name, N, K, A, es, cu, al != 0, false);
            invariants(name, N, K, A, es, cu, al != 0, true);
            // the columns a lane owns in the last K range of the row sweep at this shape (the split of the fit and, with K
            // split or not, of the streaming route): lane c has ceil((left - c) / CL) of the `left` columns
            const plsk::MissRowSplit s = plsk::miss_row_split(N, K, g.vec, cu);
            const long long CL = plsk::WG >> s.lrl, left = K - (long long)(s.S - 1) * s.kper;
            std::printf("%s %d %d %d %d %d %lld %d %lld %lld\n", name, al, g.route, g.route == plsk::XDM_RESIDENT ? g.rt : 0, g.S, g.kper,
                        (long long)g.ws_bytes, s.S, left / CL, (left + CL - 1) / CL);
        }
    }
    // a sweep of shapes around the thresholds and far from them, several CU counts
    long long swept = 0;
    const long long Ns[] = {1, 2, 3, 7, 8, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 8191, 8192, 16383, 16384, 100000, 1048576};
    const long long Ks[] = {1, 2, 7, 8, 63, 64, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4096, 50000, 200000};
    const int cus[] = {1, 64, 256, 304};
    for (long long n : Ns)
        for (long long k : Ks)
            for (int c : cus)
                for (int e = 4; e <= 8; e += 4)
                    for (int al = 0; al < 2; ++al) {
                        if (n * k > (1ll << 32)) continue;
                        const long long a = k < 10 ? k : 10;
                        std::snprintf(name, sizeof(name), "sweep-%lldx%lld-cu%d-es%d", n, k, c, e);
                        invariants(name, n, k, a, e, c, al != 0, false);
                        invariants(name, n, k, a, e, c, al != 0, true);
                        swept += 2;
                    }
    std::printf("swept %lld\n", swept);
    // the K split of a row sweep is written once: the fit's geometry (16 / es rows per lane) and the streaming route's (16 / es or
    // one row per lane) are miss_row_split's, the ranges cover K and a range is whole turns of the column lanes
    long long split = 0;
    std::vector<long long> rows;
    for (long long n = 1; n <= 70; ++n) rows.push_back(n);
    for (long long n = 255; n <= 260; ++n) rows.push_back(n);
    for (long long n = 511; n <= 514; ++n) rows.push_back(n);
    rows.push_back(5000);
    const long long cols[] = {1, 7, 8, 9, 63, 64, 65, 513, 20011, 200000};
    const int split_cus[] = {1, 64, 256};
    for (long long n : rows)
        for (long long k : cols)
            for (int e = 4; e <= 8; e += 4)
                for (int vec : {1, 16 / e})
                    for (int c : split_cus) {
                        const plsk::MissRowSplit s = plsk::miss_row_split(n, k, vec, c);
                        const int CL = plsk::WG >> s.lrl;
                        std::snprintf(name, sizeof(name), "split-%lldx%lld-es%d-vec%d-cu%d", n, k, e, vec, c);
                        EXPECT((i64)(s.S - 1) * s.kper < k && k <= (i64)s.S * s.kper, "%s: %d ranges of %d columns", name, s.S, s.kper);
                        EXPECT(s.kper % CL == 0, "%s: a range of %d columns for %d column lanes", name, s.kper, CL);
                        const plsk::XdmGeom x = plsk::xdiagmiss_geom_of(n, k, k < 3 ? k : 3, e, c, vec > 1, true);
                        EXPECT(x.vec == vec && x.lrl == s.lrl && x.nrb == s.nrb && x.S == s.S && x.kper == s.kper,
                               "%s: the streaming route has {%d, %lld, %d, %d}, the split {%d, %lld, %d, %d}", name, x.lrl, (long long)x.nrb,
                               x.S, x.kper, s.lrl, (long long)s.nrb, s.S, s.kper);
                        if (vec > 1) {
                            const plsk::MissGeom m = plsk::miss_geom_of(n, k, e, c);
                            EXPECT(m.lrl == s.lrl && m.nrb == s.nrb && m.S == s.S && m.kper == s.kper,
                                   "%s: the fit has {%d, %lld, %d, %d}, the split {%d, %lld, %d, %d}", name, m.lrl, (long long)m.nrb, m.S,
                                   m.kper, s.lrl, (long long)s.nrb, s.S, s.kper);
                        }
                        ++split;
                    }
    std::printf("split %lld\n", split);
    return failures ? 1 : 0;
}
