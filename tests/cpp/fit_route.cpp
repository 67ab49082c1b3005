// The plan fit_plan (pls_amd/csrc/fit_route.hpp) makes for a fit, without a GPU: tests/test_fit_route.py.
// stdin, one fit per line:
//   N K M A es ldx ldy ldt xmod ymod tmod num_cu method algo fuse work_layout defer fused_grid reducer pre xep denied
//   (xmod, ymod, tmod: the address of X, Y, T modulo 16; tmod < 0: no scores asked for)
// stdout, one line per fit: the plan as name=value fields.
#include "../../pls_amd/csrc/fit_route.hpp"

#include <cstdio>
#include <iostream>

int main() {
    using namespace plsk;
    FitShape s{};
    long long N, ldx, ldy, ldt, algo, fuse, layout, defer, grid;
    int xmod, ymod, tmod, reducer, pre, xep;
    unsigned denied;
    while (std::cin >> N >> s.K >> s.M >> s.A >> s.es >> ldx >> ldy >> ldt >> xmod >> ymod >> tmod >> s.num_cu >> s.method >> algo >> fuse >>
           layout >> defer >> grid >> reducer >> pre >> xep >> denied) {
        s.N = N; s.ldx = ldx; s.ldy = ldy; s.ldt = ldt;
        s.X = ((uintptr_t)1 << 32) + (uintptr_t)xmod;
        s.Y = ((uintptr_t)2 << 32) + (uintptr_t)ymod;
        s.Tm = tmod < 0 ? 0 : ((uintptr_t)3 << 32) + (uintptr_t)tmod;
        s.opt_algo = algo; s.opt_fuse = fuse; s.opt_work_layout = layout; s.opt_defer = defer; s.opt_fused_grid = grid;
        s.reducer = reducer != 0; s.pre = pre != 0; s.xep = xep != 0;
        const FitPlan p = fit_plan(s, denied);
        static const char *const names[] = {"KERNEL", "NIPALS", "GRAM", "TYPE2"};
        std::printf("algo=%s use_pre=%d fused_mode=%d wide_mode=%d semi_fit=%d wide_only=%d tiled_work=%d retile_fit=%d nip_copy=%d "
                    "tall_cg=%d wide_cg=%d mid_cg=%d defer=%d TR=%lld WR=%lld ldw=%lld tsw=%lld work=%zu part=%zu sspart=%zu red=%zu "
                    "prow=%lld ssmax=%lld xep_ok=%d\n",
                    names[p.algo], (int)p.use_pre, p.fused_mode, p.wide_mode, (int)p.semi_fit, (int)p.wide_only, (int)p.tiled_work,
                    (int)p.retile_fit, (int)p.nip_copy, p.tall_cg, p.wide_cg, p.mid_cg, p.defer, (long long)p.TR, (long long)p.WR,
                    (long long)p.ldw, (long long)p.tsw, p.work_bytes, p.part_bytes, p.sspart_bytes, p.red_bytes, (long long)p.prow,
                    (long long)p.ssmax, (int)p.xep_ok);
    }
    return 0;
}
