// vardiag_geom_of (pls_amd/csrc/vardiag_layout.hpp) on the CPU: every (row tile, column block) of the column sweep has exactly one
// owner, the partials of every range fill the planned buffer without a collision, the ranges cover 1..A, the tile fits a CU twice.
// Includes only that header; tests/test_vardiag_layout.py builds it with ASan + UBSan and feeds it the cases.
// stdin: one case per line "name N K A es", 256 CUs.
// stdout: per case and alignment "name aligned vec NT CB RS nranges AS part_bytes st_bytes msg_values one_launch", then "swept <n>"
// for the shapes of the sweep below.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pls_amd/csrc/vardiag_layout.hpp"

using plsk::vd_i64;

static int failures = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");        \
            ++failures;                        \
        }                                      \
    } while (0)

static void invariants(const char *name, vd_i64 N, vd_i64 K, vd_i64 A, int es, int cu, bool aligned) {
    const plsk::VdGeom g = plsk::vardiag_geom_of(N, K, A, es, cu, aligned);
    EXPECT(g.vec == (aligned ? 16 / es : 1), "%s: vec %d", name, g.vec);
    EXPECT(plsk::VD_TR % g.vec == 0 && plsk::VD_TR * plsk::VD_TC % (plsk::VD_THREADS * g.vec) == 0, "%s: a tile in whole vectors per thread", name);
    EXPECT(g.NT * plsk::VD_TR >= N && (g.NT - 1) * plsk::VD_TR < N, "%s: %lld row tiles for %lld rows", name, (long long)g.NT, (long long)N);
    EXPECT(g.CB * plsk::VD_TC >= K && (g.CB - 1) * plsk::VD_TC < K, "%s: %lld column blocks for %lld columns", name, (long long)g.CB, (long long)K);
    EXPECT(g.RS >= 1 && g.RS <= g.NT && g.RS <= 65535, "%s: %d row splits of %lld tiles", name, g.RS, (long long)g.NT);
    EXPECT(g.RS == g.NT || (vd_i64)g.RS * g.CB >= (vd_i64)plsk::VD_WG_PER_CU * cu, "%s: %d x %lld workgroups leave CUs idle", name, g.RS, (long long)g.CB);
    EXPECT(g.lds_bytes == plsk::VD_TILE_BYTES && plsk::VD_WG_PER_CU * g.lds_bytes <= plsk::VD_LDS_CU, "%s: LDS", name);
    EXPECT(plsk::VD_LDC % 2 == 1 && plsk::VD_LDC >= plsk::VD_TR, "%s: the padded column", name);
    // every row tile has one owner among the splits (the column blocks are the grid's other axis: one workgroup per pair)
    if (g.NT <= (1 << 22)) {
        std::vector<unsigned char> owner((size_t)g.NT, 0);
        for (int rs = 0; rs < g.RS; ++rs) {
            const vd_i64 lo = plsk::vd_tile_lo(g.NT, g.RS, rs), hi = plsk::vd_tile_lo(g.NT, g.RS, rs + 1);
            EXPECT(lo < hi, "%s: split %d owns no tile", name, rs);
            for (vd_i64 t = lo; t < hi; ++t) owner[(size_t)t] += 1;
        }
        for (vd_i64 t = 0; t < g.NT; ++t) EXPECT(owner[(size_t)t] == 1, "%s: tile %lld has %d owners", name, (long long)t, owner[(size_t)t]);
    }
    EXPECT(plsk::vd_tile_lo(g.NT, g.RS, 0) == 0 && plsk::vd_tile_lo(g.NT, g.RS, g.RS) == g.NT, "%s: the splits' ends", name);
    // the ranges cover 1..A in order; a range's kernel reads CR scores of a row inside its AS
    EXPECT(g.AS % 4 == 0 && g.AS >= A && g.AS < A + 4, "%s: AS %d", name, g.AS);
    int at = 0;
    vd_i64 most = 0;
    for (int j = 0; j < g.nranges; ++j) {
        const int lo = plsk::vd_range_lo(j), hi = plsk::vd_range_hi(j, (int)A), nc = hi - lo, cr = plsk::vd_cr(nc);
        EXPECT(lo == at && hi > lo && nc <= plsk::VD_RANGE, "%s: range %d is [%d, %d)", name, j, lo, hi);
        EXPECT(cr >= nc && cr < nc + 4 && cr <= plsk::VD_RANGE && lo + cr <= g.AS && lo % 8 == 0, "%s: range %d computes %d counts", name, j, cr);
        at = hi;
        // its partials: (rs, plane, k) -> one cell each, inside the buffer
        const vd_i64 L = nc + (lo == 0 ? 1 : 0);
        const vd_i64 p_rs = g.p_one_launch ? L * K : K, p_j = g.p_one_launch ? K : (vd_i64)g.RS * K;
        const vd_i64 cells = (vd_i64)g.RS * L * K;
        EXPECT((g.RS - 1) * p_rs + (L - 1) * p_j + (K - 1) == cells - 1, "%s: range %d: the last partial is not the buffer's last cell", name, j);
        EXPECT(g.p_one_launch ? L * K <= plsk::VD_INT_MAX : K <= plsk::VD_INT_MAX, "%s: a reduction longer than 2^31", name);
        if (cells <= (1 << 16)) {
            std::vector<unsigned char> hit((size_t)cells, 0);
            for (int rs = 0; rs < g.RS; ++rs)
                for (vd_i64 p = 0; p < L; ++p)
                    for (vd_i64 k = 0; k < K; ++k) hit[(size_t)(rs * p_rs + p * p_j + k)] += 1;
            for (vd_i64 i = 0; i < cells; ++i) EXPECT(hit[(size_t)i] == 1, "%s: range %d: partial cell %lld written %d times", name, j, (long long)i, hit[(size_t)i]);
        }
        most = cells > most ? cells : most;
    }
    EXPECT(at == A, "%s: the ranges end at %d of %lld", name, at, (long long)A);
    EXPECT(g.part_bytes == most * 8, "%s: %lld bytes of partials planned, the largest range needs %lld", name, (long long)g.part_bytes, (long long)(most * 8));
    EXPECT(g.st_bytes == g.NT * plsk::VD_TR * g.AS * 8, "%s: the row-contiguous scores", name);
    EXPECT(g.msg_values == A + K * (A + 1), "%s: the message", name);
    const plsk::VdGeom s = plsk::vardiag_geom_of(N, K, A, es, cu, aligned, false);
    EXPECT(s.msg_values == A && s.part_bytes == 0 && s.st_bytes == 0, "%s: without ssxk", name);
}

int main() {
    const int cu = 256;
    char name[128];
    long long N, K, A;
    int es;
    while (std::scanf("%127s %lld %lld %lld %d", name, &N, &K, &A, &es) == 5) {
        for (int al = 0; al < 2; ++al) {
            invariants(name, N, K, A, es, cu, al != 0);
            const plsk::VdGeom g = plsk::vardiag_geom_of(N, K, A, es, cu, al != 0);
            std::printf("%s %d %d %lld %lld %d %d %d %lld %lld %lld %d\n", name, al, g.vec, (long long)g.NT, (long long)g.CB, g.RS, g.nranges, g.AS,
                        (long long)g.part_bytes, (long long)g.st_bytes, (long long)g.msg_values, g.p_one_launch);
        }
    }
    long long swept = 0;
    const long long Ns[] = {1, 2, 127, 128, 129, 255, 256, 257, 1031, 4097, 40000, 65537, 1048576};
    const long long Ks[] = {1, 7, 63, 64, 65, 127, 128, 129, 513, 4000, 100000};
    const long long As[] = {1, 3, 4, 5, 23, 24, 25, 48, 50};
    const int cus[] = {1, 64, 256, 304};
    for (long long n : Ns)
        for (long long k : Ks)
            for (long long a : As)
                for (int c : cus)
                    for (int e = 4; e <= 8; e += 4)
                        for (int al = 0; al < 2; ++al) {
                            if (a > k || n * k > (1ll << 31)) continue;
                            std::snprintf(name, sizeof(name), "sweep-%lldx%lld-a%lld-cu%d-es%d", n, k, a, c, e);
                            invariants(name, n, k, a, e, c, al != 0);
                            ++swept;
                        }
    // a reduction that no longer fits one launch: a launch per plane
    invariants("planes", 1, 100000000, 24, 4, cu, true);
    EXPECT(plsk::vardiag_geom_of(1, 100000000, 24, 4, cu, true).p_one_launch == 0, "planes: one launch of 2.5e9 values");
    std::printf("swept %lld\n", swept);
    return failures ? 1 : 0;
}
