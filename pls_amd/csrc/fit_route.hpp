// fit_route.hpp -- which plan a fit takes once no single-launch route has taken it, with what tiles and workspaces: fit_plan, a
// pure function of the shape.  fit_device (plan_fit.hpp) executes it.  Plain C++17, no HIP and no handle: tests/cpp/fit_route.cpp
// builds it with the host compiler alone.  The layout predicates the launchers share with the plan live here too (common.hpp
// includes this file), with addresses as integers and the element size `es` (8 or 4) as a value.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pls_hip.h"  // PLS_HIP_ALGO_*, PLS_HIP_KERNEL_TYPE*
#include "xb_route.hpp"             // i64, WAVE, WG

namespace plsk {

// slices of every reduced vector (reduce_partials_kernel, slice_tail): enough workgroups take part in a reduction, and the
// consumers add the slices of a value in index order
constexpr int RED_SLICES = 8;
constexpr int SYRK_TB = 128;             // block tile of the SYRK (columns of X per panel: syrk_kernels.hpp)
constexpr i64 XCHG_CAP = 1 << 16;        // doubles per message piece of the device-side exchange (512 KB: exchange_kernels.hpp)
constexpr int XTY_KCMT = 32;             // accumulators per lane in xty_kernel

// ---- layout predicates (shared by the launchers) -------------------------------------------------------------------------------
// a base of `vec` elements' alignment and a leading dimension of whole vec-element vectors
inline bool vec_ok(uintptr_t p, i64 ld, int es, int vec) { return (p % ((size_t)es * vec) == 0) && (ld % vec == 0); }
// 16-byte aligned columns / element alignment; the span of the column groups behind one descriptor
inline bool cols_aligned(uintptr_t q, i64 ld, int es) { return (q % 16 == 0) && (ld % (16 / es) == 0); }
inline bool elem_aligned(uintptr_t q, int es) { return q % (size_t)es == 0; }
// EDGE level of a source matrix (ld in elements) read with tiles of RP row lanes: 0 plain, 1 per-wave descriptors
// (long columns), 2 unaligned columns; -1 = not addressable at all
inline int edge_level(uintptr_t q, i64 ld, int es, int cg_all, int cg_wave) {
    if (!elem_aligned(q, es)) return -1;
    const bool fits = (i64)cg_all * ld * (i64)es < (1ll << 31);
    if (cols_aligned(q, ld, es) && fits) return 0;
    if ((i64)cg_wave * ld * (i64)es >= (1ll << 31)) return -1;
    return cols_aligned(q, ld, es) ? 1 : 2;
}

// upper bound of partial rows any product of a fit can write (fused_grid: PLS_HIP_OPT_FUSED_GRID)
inline i64 max_partial_rows(int num_cu, i64 fused_grid, i64 N, int K) {
    const int nkg32 = (K + XTY_KCMT - 1) / XTY_KCMT;
    const i64 nch = (N + WG - 1) / WG;  // vec = 1 is the worst case
    const i64 G = std::min<i64>(std::max<i64>(1, (8 * num_cu) / nkg32), std::max<i64>(nch, 1));
    return std::max<i64>(G, std::max<i64>(8 * (i64)num_cu, fused_grid));
}

// Will launch_deflate_score accept every deflating pass of a fit (decided once per fit, like fused_pass_mode)?
// 0 = no, 1 = yes, 2 = yes through an EDGE instantiation (long or unaligned columns).
inline int deflate_score_mode(uintptr_t X, i64 ldx, int es, i64 N, int K, uintptr_t Tm) {
    const int V = 16 / es;
    const int CG = 512 / ((256 / es) / V);
    if (N < 1 || (size_t)K * 16 > 72 * 1024 || !elem_aligned(Tm, es) || (N + 16) * (i64)es >= (1ll << 31)) return 0;
    const int e = edge_level(X, ldx, es, CG, 4);
    return e < 0 ? 0 : (e == 0 ? 1 : 2);
}
// Can the caller's matrix be copied into short tiles (launch_retile / launch_retile_xty read it with the 256-byte-segment
// tile) and every pass then run on the copy?  The checks of deflate_score_mode without its LDS limit on K.
inline bool wide_source_ok(uintptr_t X, i64 ldx, int es, i64 N, uintptr_t Tm) {
    const int V = 16 / es;
    const int CG = 512 / ((256 / es) / V);
    if (N < 1 || !elem_aligned(Tm, es) || (N + 16) * (i64)es >= (1ll << 31)) return false;
    return edge_level(X, ldx, es, CG, 4) >= 0;
}

// Column groups of the tile that reads the caller's matrix.  32 (16 row lanes, 256-byte segments) from 257 columns on;
// NARROW matrices take taller tiles with fewer column groups, so that a lane still has 8-16 loads in flight: 8 groups x 64
// row lanes (128 fp64 rows, 1 KB segments) up to 128 columns, 16 x 32 up to 256.  With the 32-group tile a 64-column matrix
// has 2 loads per lane and streams at 0.64-0.68 of peak (config-3-sized: 581 / 1,097 components/s), a 32-column one at 0.38-0.46.
inline int tall_groups(int K) {
    return K <= 128 ? 8 : (K <= 256 ? 16 : 32);
}
// Will launch_fused_pass accept every pass of a fit on (X, ldx) with score columns Tm + a*ldt?  (Decided once
// per fit: the work buffer's layout depends on it.)  0 = no; 1 = yes; 2 = yes through an EDGE instantiation (columns
// that are not 16-byte aligned, or a leading dimension whose 32 column groups do not fit one descriptor -- up to
// 2^31 bytes per WAVE / RP = 4 columns there).  Any N >= 1: the last N % V rows are the tail kernel's.
inline int fused_pass_mode(uintptr_t X, i64 ldx, int es, i64 N, int K, uintptr_t Tm) {
    const int CG = tall_groups(K);
    if (K > 32 * 32 || N < 1 || !elem_aligned(Tm, es) || (N + 16) * (i64)es >= (1ll << 31)) return 0;
    const int e = edge_level(X, ldx, es, CG, CG / 8);  // (a wave holds 64 / (512 / CG) = CG / 8 column groups)
    return e < 0 ? 0 : (e == 0 ? 1 : 2);
}

// ---- the plan of a fit -----------------------------------------------------------------------------------------------------------
struct FitShape {
    i64 N;
    int K, M, A;
    int es;                 // sizeof(T): 8 or 4
    i64 ldx, ldy, ldt;
    uintptr_t X, Y, Tm;     // addresses (Tm: 0 = no scores asked for)
    int num_cu;
    int method;             // pls_hip_method
    i64 opt_algo, opt_fuse, opt_work_layout, opt_defer, opt_fused_grid;
    bool reducer;           // a reducer is installed
    bool pre;               // X^T X and X^T Y came with the upload
    bool xep;               // the device-side exchange is attached
};

enum FitAlgo { FIT_KERNEL, FIT_NIPALS, FIT_GRAM, FIT_TYPE2 };
constexpr unsigned FIT_NO_COPY = 1u;  // `denied`: the optional tiled copy of the KERNEL plan was refused its memory

struct FitPlan {
    FitAlgo algo;
    bool use_pre;           // GRAM / TYPE2 start from the upload's X^T X and X^T Y
    int fused_mode;         // fused_pass_mode of the caller's matrix (0: the tile-resident pass does not cover the fit)
    int wide_mode;          // deflate_score_mode, asked only where fused_mode is 0
    bool semi_fit;          // NIPALS on a wide matrix: deflation + score in one sweep, the loading in a second read
    bool wide_only;         // NIPALS, 4096 < K <= 8192: every component fused on the row-pack copy, which must succeed
    bool tiled_work;        // NIPALS: the working copy is row-tile-major
    bool retile_fit;        // KERNEL: X is copied once into tiles, every component reads the copy
    bool nip_copy;          // NIPALS on a wide matrix: the working copy is made in the X^T Y sweep
    int tall_cg;            // column groups of the tile that reads the caller's matrix ...
    int wide_cg;            // ... of the short tiles of the working copy (0: none) ...
    int mid_cg;             // ... of its half-height tiles for 512 < K <= 1024 (0: none)
    int defer;              // rank-1 updates pending per stored matrix (1: every pass stores)
    i64 TR, WR;             // rows per tile: of the caller's matrix, of the working copy
    i64 ldw, tsw;           // column stride and tile stride of the working copy
    size_t work_bytes;      // workspaces (work: 0 = none)
    size_t part_bytes, sspart_bytes, red_bytes;
    i64 prow, ssmax;        // capacity of `part` in partial rows, of `sspart` in partials
    bool xep_ok;            // the device-side exchange can carry a component's sums
};

inline FitPlan fit_plan(const FitShape &s, unsigned denied) {
    const i64 N = s.N;
    const int K = s.K, M = s.M, A = s.A, es = s.es;
    FitPlan p{};
    i64 algo = s.opt_algo;
    // GRAM plan for a KERNEL_TYPE1 request: the K-sized loop runs on XX = X^T X exactly as KERNEL_TYPE2
    // does (no pass over X per component), then the scores are formed in one pass, T = X R.
    // AUTO: pick between the read-only pass plan and the Gram plan from a bandwidth / matrix-core cost
    // model (measured rates on MI355X: ~6 TB/s streaming reads, ~59 TFLOP/s executed in the fp64 SYRK of
    // which the symmetric half is computed).  GRAM pays off for A >~ K/60.
    const bool have_pre = s.pre && K <= 32768;
    if (algo == PLS_HIP_ALGO_AUTO && have_pre) {
        algo = PLS_HIP_ALGO_GRAM;  // X^T X is already there: the component loop needs no pass over X at all
    } else if (algo == PLS_HIP_ALGO_AUTO) {
        // Both plans priced with what they launch (profiles/r4/auto_scan.txt): a pass over X per component + ~14 us of launches for
        // KERNEL; for GRAM the SYRK on the blocks it EXECUTES (whole 128-column blocks: a 32-column matrix costs what a 128-column
        // one does), the pass that forms T = X R, and per component the symv + update on K x K data, ~9 us + 18 ns per column.
        const double pass_s = (double)N * K * es / 6.0e12;
        const int nbk = (K + SYRK_TB - 1) / SYRK_TB;
        const double kp = (double)nbk * SYRK_TB;
        // tiles of 16 x 16 the SYRK executes: the blocks above the diagonal in full, 36 of 64 in a diagonal block (syrk_kernels.hpp)
        const double tile_frac = (32.0 * nbk * (nbk - 1) + 36.0 * nbk) / (64.0 * nbk * nbk);
        const double syrk_s = 2.0 * N * kp * kp * tile_frac / 60.0e12;
        const double kernel_s = (1 + A) * pass_s + A * 14e-6;
        const double gram_s = syrk_s + 1.3 * pass_s + A * (9e-6 + K * 1.8e-8) + 40e-6;
        // ranks of a sharded fit see different N: they must not disagree on the plan -> KERNEL there
        const bool gram_ok = K <= 2048 && N >= 4096 && !s.reducer;
        algo = (gram_ok && kernel_s > gram_s) ? PLS_HIP_ALGO_GRAM : PLS_HIP_ALGO_KERNEL;
    }
    const bool gram = (s.method == PLS_HIP_KERNEL_TYPE1) && (algo == PLS_HIP_ALGO_GRAM);
    const bool type2 = (s.method == PLS_HIP_KERNEL_TYPE2) || gram;
    const bool nipals = !type2 && (algo == PLS_HIP_ALGO_NIPALS);
    p.algo = gram ? FIT_GRAM : (type2 ? FIT_TYPE2 : (nipals ? FIT_NIPALS : FIT_KERNEL));
    p.use_pre = have_pre && type2;
    const i64 L0 = (i64)K * M;
    const i64 redn = (i64)RED_SLICES * std::max<i64>(L0, K + 1);
    p.prow = max_partial_rows(s.num_cu, s.opt_fused_grid, N, K);
    p.part_bytes = (size_t)p.prow * (size_t)std::max<i64>(L0, K) * 8;
    // t^T t partials: one per workgroup of whichever kernel forms the scores (narrow X*v: N/256; tile kernels: their grid)
    // (the split score kernel of short, wide matrices leaves one partial per 64 rows)
    p.ssmax = std::max<i64>(std::max<i64>(K >= 1024 ? (N + 63) / 64 : (N + WG - 1) / WG, 1), p.prow);
    p.sspart_bytes = (size_t)p.ssmax * 8;
    p.red_bytes = (size_t)redn * 8;
    // NIPALS keeps the deflated matrix in a library-owned buffer.  When the tile-resident pass covers the fit it
    // is stored row-tile-major (every R x K tile one contiguous block: fused_kernels.hpp), otherwise column-major
    // with ld = N for the one-product kernels.
    // the tile that reads the caller's matrix: 32 column groups x 16 row lanes, taller with fewer groups for narrow matrices
    p.tall_cg = tall_groups(K);
    p.TR = (512 / p.tall_cg) * (i64)(16 / es);
    // Any row count (the last N % V rows go to a tail kernel), any alignment of the columns and leading dimensions up to
    // 2^31 / 4 bytes (mode 2: the EDGE instantiations) -- the same one-sweep traffic for every matrix the reference
    // accepts (src/pls.cpp:419-421)
    p.fused_mode = (s.opt_fuse && N > 0) ? fused_pass_mode(s.X, s.ldx, es, N, K, s.Tm) : 0;
    const bool fused_fit = p.fused_mode != 0;
    p.wide_mode = (s.opt_fuse && !fused_fit && N > 0) ? deflate_score_mode(s.X, s.ldx, es, N, K, s.Tm) : 0;
    // wide matrices (no resident tile): deflation + score in one sweep, loading in a second read
    p.semi_fit = nipals && p.wide_mode != 0;
    // Beyond the semi-fused sweep's reach (its w and p_prev need 16 K bytes of LDS: K <= 4608) and up to 8192 columns the
    // copy's tiles are ONE row pack high (512 column groups x 16 columns per lane): the copy is made in the X^T Y sweep
    // (retile_xty) and every component runs fused on it -- instead of 4 N K s (NIPALS) / 2 N K s (KERNEL) per component
    // through the one-product kernels.
    // (read-only passes take 32 columns per lane there: the KERNEL plan up to 16384 columns)
    // (every precondition of launch_retile_xty for this shape is decided HERE, so that a fit which counts on the copy --
    // wide_only -- cannot find it refused later: the source layout (wide_source_ok), element-aligned responses, M <= 8
    // (wide_only below); the launcher's span limits hold for every row-pack tile -- 16 V K s + 512 bytes < 2^31 at K <= 16384
    // -- and the partial-row capacity is never below 2)
    // (beyond 8192 columns -- 32 columns per lane, a partial row of K doubles per workgroup -- only from 4096 rows on: on a shorter
    // matrix the partial rows weigh as much as the matrix and the one-product kernels win, 500 x 10,000: 0.47 against 0.83 ms per
    // fit, 1,500 x 10,000: 0.70 / 0.89, 3,000 x 12,000: 1.22 / 1.30; 6,000 x 10,000: 1.91 / 1.59 -- profiles/r4/short_wide_plan_choice.txt)
    const bool wide_src = s.opt_fuse && !fused_fit && N > 0 && K <= 512 * (nipals ? 16 : 32) && (K <= 512 * 16 || N >= 4096) &&
                          wide_source_ok(s.X, s.ldx, es, N, s.Tm) && elem_aligned(s.Y, es);
    // (more than 8 responses: X^T Y does not ride in the copy's sweep -- a plain copy before the first component and the X^T Y pass
    // of its own, as the KERNEL plan does; 25,000 x 8,192 with 12 responses: 12.3 -> 7.5 ms per 10-component fit)
    p.wide_only = nipals && wide_src && K > 256 * 16 && K <= 512 * 16 && A >= 3 && s.opt_work_layout != 0;
    p.tiled_work = nipals && (fused_fit || p.semi_fit || p.wide_only) && s.opt_work_layout != 0;
    // Row-tile-major tiles are contiguous whatever their height, so for 1024 < K <= 4096 the working copy uses
    // SHORTER tiles (8-32 rows) that do fit the registers of a CU: from the third component on the fully fused
    // pass runs again (2 N K s per component instead of the semi-fused 3 N K s).  Only the first deflation has
    // to read the caller's column-major X in 256-byte pieces (deflate_score, writing the short tiles).
    // KERNEL plan on such a matrix: X is copied ONCE into short tiles (read + write), after which every component
    // is one fused read-only pass instead of two one-product passes -- pays from the third component on.
    // ... and on a matrix whose columns are not 16-byte aligned (ld odd, a base pointer at 8 mod 16): the one-sweep pass can
    // read it (EDGE level 2) but every 256-byte segment then shares a line with its neighbours and the pass runs at 0.52
    // instead of 0.73 of peak; with the copy (formed in the same sweep as X^T Y: retile_xty_kernel) every component reads
    // aligned tiles.  Costs one write of X; pays from the fourth component on (copy_min below).
    const int FVX = 16 / es;
    // The same copy pays for ALIGNED matrices once there are enough components: a read-only pass over the tiled copy, one
    // contiguous 128 KB block per tile, runs at 0.85 of peak (0.63 ms at config 3) against 0.72 (0.74 ms) over the caller's
    // column-major matrix in 256-byte segments; the copy costs 0.86 ms more than the X^T Y pass it replaces
    // (copy_min_al below: 10 components).
    // Beyond 512 columns the direct pass (32 columns per lane, one workgroup per CU) already reads at 0.81 of peak and the
    // copy only pays from ~30 components on (one shard of config 5: 2.65 -> 2.52 ms per pass against 4.1 ms for the copy).
    constexpr int copy_min = 4, copy_min_al = 10;
    const bool copy_fit = fused_fit && M <= 8 &&
                          A >= (vec_ok(s.X, s.ldx, es, FVX) ? (K <= 32 * 16 ? copy_min_al : 3 * copy_min_al + 2) : copy_min);
    // (the copy is optional: without room for it -- FIT_NO_COPY -- the one-product kernels do the job)
    p.retile_fit = !(denied & FIT_NO_COPY) && !nipals && !type2 && A >= 3 && s.opt_work_layout != 0 &&
                   ((p.wide_mode != 0 && K <= 128 * 32) || (wide_src && K > 128 * 32) || copy_fit);
    // column groups of the short tiles of a wide matrix (1024 < K <= 4096): 16 columns per lane in 128 / 256 groups
    // (8-row fp32 / 4-row fp64 tiles at K <= 4096) -- the register shape of the headline kernel, two workgroups per CU
    // on read-only passes.  Config 4: read+write pass 0.766 -> 0.710 ms (0.70 -> 0.76 of peak), read-only pass
    // 0.364 -> 0.324 ms (0.74 -> 0.83) against 32 columns per lane in 64 / 128 groups (the round-1 shape, deleted in round 4).
    const int wide_groups = fused_fit ? (K <= 32 * 16 ? p.tall_cg : 64)  // (the copy of a matrix the resident tile covers)
                            : (K <= 128 * 16 ? 128 : (K <= 256 * 16 ? 256 : ((wide_src && (!nipals || p.wide_only)) ? 512 : 0)));
    p.wide_cg = ((p.semi_fit && p.tiled_work) || p.retile_fit || p.wide_only) ? wide_groups : 0;
    // 512 < K <= 1024: the resident tile of the caller's layout needs 32 columns per lane (one 8-wave workgroup per
    // CU, 5.7-5.85 TB/s); on the tiled copy the same K fits half-height tiles at 16 columns per lane (6.0 TB/s).
    // Component 0 reads X with the tall tile, the first deflation reads X tall and writes the short tiles (rdst),
    // every later pass runs on the short tiles.
    p.mid_cg = (nipals && fused_fit && p.tiled_work && K > 32 * 16 && A > 2) ? 64 : 0;
    // opt-in deferred write-back (defer_kernels.hpp): up to `defer` rank-1 updates pending per stored matrix
    p.defer = (nipals && p.fused_mode == 1 && p.tall_cg == 32 && N % FVX == 0 && cols_aligned(s.Tm, s.ldt, es) && p.tiled_work && K <= 32 * 16)
                  ? (int)s.opt_defer : 1;
    const int work_cg = p.wide_cg ? p.wide_cg : (p.mid_cg ? p.mid_cg : p.tall_cg);
    p.WR = (512 / work_cg) * (i64)(16 / es);  // rows per tile of the working copy
    const bool tiled = p.tiled_work || p.retile_fit;
    if ((nipals && A > 1 && N > 0) || p.retile_fit)
        p.work_bytes = tiled ? (size_t)((N + p.WR - 1) / p.WR) * p.WR * K * es : (size_t)((N + 3) & ~(i64)3) * K * es;
    // (a column-major working copy keeps 16-byte columns whatever N is)
    const i64 PV = 16 / (i64)es;
    p.ldw = tiled ? p.WR : (N + PV - 1) / PV * PV;
    p.tsw = tiled ? p.WR * (i64)K : p.TR;
    p.xep_ok = s.xep && s.reducer && (i64)K + 1 <= XCHG_CAP;
    // NIPALS on a wide matrix takes the same first sweep: its working copy is then complete before the first component,
    // which runs fused on it, as every later one does in place (instead of two one-product passes over X for component 0
    // and the semi-fused sweep + a loading pass for component 1: config 4 36.6 -> 36.0 ms per fit)
    p.nip_copy = nipals && (p.semi_fit || p.wide_only) && p.tiled_work && p.wide_cg != 0 && A >= 3;
    return p;
}

}  // namespace plsk
