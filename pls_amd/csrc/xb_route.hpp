// xb_route.hpp -- which kernel takes the next columns of out(N x C) = X * Bm, and with what geometry: xb_next, a pure function of
// the shape.  launch_xb (launch_products.hpp) executes its steps.  Plain C++17, no HIP and no handle: tests/cpp/xb_route.cpp
// builds it with the host compiler alone.  The geometry helpers and workgroup sizes the kernels share with the routes live here
// too (common.hpp includes this file).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pls_hip.h"  // PLS_HIP_FAM_XB

namespace plsk {

typedef int64_t i64;

constexpr int WAVE = 64;
constexpr int WG = 256;
constexpr int XB4_WG = 1024;  // workgroup of the 4 x 4 x 4 MFMA kernels (xb_mfma4.hpp, xb_mfma4w.hpp)

// ---- geometry of the 4 x 4 x 4 MFMA kernels (constexpr: host and device) ------------------------------------------------------
// xb_mfma4_kernel, column steps per batch: 4 (2 where the accumulators of fp32 storage's 4-row packs leave no room) -- 8 fit the
// registers up to 20 fp64 columns and are 4 % slower with the barrier (0.757 against 0.730 ms; 2: 0.723, 1: 0.791)
constexpr int xb4_u(int v, int ncg) { return v * ncg > 20 ? 2 : 4; }
constexpr int xb4_kp(int K, int u) { return (K + (4 * u > 32 ? 4 * u : 32) - 1) / (4 * u > 32 ? 4 * u : 32) * (4 * u > 32 ? 4 * u : 32); }  // rows of Bm in LDS
constexpr int xb4_stride(int ncg) { return (8 * ncg) % 64 == 0 ? 4 * ncg + 4 : 4 * ncg; }  // (k-rows on disjoint banks)
// xb_mfma4w_kernel, rows of Bm per window (a power of two: the staging's index arithmetic is shifts): as many as two buffers of
// [KC][ST] doubles fit in ~150 KB of LDS and 8 doubles per thread carry -- 1,024 for 8 columns, 512 up to 16, 256 beyond
// (fp32 storage, V = 4 rows per lane: twice the accumulators -- 128 rows from 16 columns on, so that nothing spills in the loop)
constexpr int xb4w_kcl2(int v, int ncg) { return ncg <= 2 ? 10 : ncg <= 3 ? 9 : v > 2 ? 7 : ncg <= 4 ? 9 : 8; }

// ---- the routes of X * Bm ------------------------------------------------------------------------------------------------------
enum XbRoute {         // one value per launch shape; `vec`, `sel` of the step are the template selectors <T, vec, sel>
    XB_KERNEL,         // xb_kernel<T, vec, MT, ss>: 1, 2 or 4 columns, Bm in registers
    XB_WIDE,           // xb_wide_kernel<T, vec, MT>: up to 32 columns, Bm through LDS
    XB_WIDE2,          // xb_wide_kernel<T, 2, MT, 2>: its two-pack form
    XB_SPLIT,          // xb_split_kernel<T, vec, MT> over (rows, columns of X) + xb_split_finish_kernel
    XB_MFMA_LDS,       // xb_mfma_lds_kernel<T, vec, NT>: up to 16 NT columns on the 16-wide MFMA
    XB_MFMA4,          // xb_mfma4_kernel<T, vec, NCG>: all of Bm resident in LDS
    XB_MFMA4W,         // xb_mfma4w_kernel<T, vec, NCG>: Bm in windows
    XB_MFMA4W_SPLIT,   // xb_mfma4w_kernel<T, vec, NCG> with the columns of X split over blockIdx.y + xb_split_finish_kernel
};
constexpr unsigned xb_bit(XbRoute r) { return 1u << r; }
// the routes that need a resource (dynamic LDS beyond the default, the partial buffer) and can therefore be denied ...
constexpr unsigned XB_OPTIONAL = xb_bit(XB_SPLIT) | xb_bit(XB_MFMA4) | xb_bit(XB_MFMA4W) | xb_bit(XB_MFMA4W_SPLIT);
// ... and those of them that take a whole call or none of it: a denial under way restarts the call at column 0
constexpr unsigned XB_WHOLE_CALL = xb_bit(XB_SPLIT) | xb_bit(XB_MFMA4W_SPLIT);

struct XbShape {
    i64 N;
    int K, C;
    i64 ldx, ldo;
    int es;               // sizeof(T): 8 or 4
    bool x_vec, out_vec;  // X / out: 16-byte base and a leading dimension of whole 16-byte vectors
    int num_cu;
    int xb4;              // PLS_HIP_XB4
    bool ss;              // the sum of squares of the (one) column is asked for
};

struct XbStep {
    XbRoute route;
    int use;             // columns c0 .. c0 + use - 1
    int vec, sel;        // template selectors: rows per lane; MT (columns per tile), NT or NCG (column groups)
    bool ss;             // xb_kernel<T, vec, 1, true>: writes gx partial sums of squares
    unsigned gx, gy;     // grid
    size_t lds;          // dynamic LDS bytes
    int kper, ks, sw;    // split routes: columns of X per blockIdx.y, and how many; xb_mfma4w_kernel: sub-windows per tile slot
    i64 ldp;             // partial buffer: leading dimension ...
    size_t part_bytes;   // ... and size (0: none)
    int fam;             // Scope: family and traffic
    i64 bytes;
};

// The step that handles columns c0 ... of the call `s`; `denied`: the xb_bit()s of the routes that were refused their resource.
inline XbStep xb_next(const XbShape &s, int c0, unsigned denied) {
    const i64 N = s.N, ldx = s.ldx, ldo = s.ldo, es = s.es;
    const int K = s.K, C = s.C, num_cu = s.num_cu, rem = C - c0, FV = 16 / s.es;
    const bool f32 = s.es == 4;
    auto open = [&](XbRoute r) { return !(denied & xb_bit(r)); };
    XbStep st{};
    auto done = [&](XbRoute r, int use, int vec, int sel, i64 gx) {
        st.route = r; st.use = use; st.vec = vec; st.sel = sel; st.gx = (unsigned)gx;
        if (!st.gy) st.gy = 1;
        st.fam = PLS_HIP_FAM_XB;
        st.bytes = N * K * es + N * use * es + (i64)K * use * 8;
        return st;
    };

    bool wide = s.x_vec && s.out_vec;
    // keep >= ~4 workgroups per CU in flight: narrow the per-lane access on short matrices
    if (wide && N / ((i64)FV * WG) < 4 * (i64)num_cu) wide = false;
    // the matrix-core kernel xb_mfma_lds_kernel takes the columns in one pass -- more than 8 with fp32 storage, more than 32 with
    // fp64 -- and has a workgroup for at least half the CUs
    const i64 rows_per_wg_many = (i64)(WG / WAVE) * 16 * FV;
    const bool many = C > (f32 ? 8 : 32) && s.x_vec && (N + rows_per_wg_many - 1) / rows_per_wg_many >= num_cu / 2;
    // 5..32 columns of a large matrix on the 4 x 4 x 4 MFMA kernels (xb_mfma4.hpp, xb_mfma4w.hpp): one sweep of X where the column-split
    // path below makes one per 4 columns (20,000 x 2,000, 20 columns: five sweeps, 0.13 of peak).  Not for a handful of columns
    // of a matrix with fewer than 128: its output is a third of the traffic and the VALU kernels are as fast.
    // Nor for a matrix with fewer 16 FV-row tiles than CUs (2,000 x 20,000: the MFMA column-split route spreads it).
    const i64 xb4_tiles = (N + 16 * FV - 1) / (16 * FV);
    const bool xb4_big = (i64)N * K * es >= ((i64)32 << 20);
    const bool xb4_ok = s.xb4 && C > 4 && s.x_vec && s.out_vec && 36 * std::max(ldx, ldo) * es < ((i64)1 << 31) && xb4_big &&
                        (K >= 128 || C > 8) && xb4_tiles >= (i64)num_cu;
    // the resident form (all of Bm in LDS, a wave per tile): at least two rounds of 16 tiles per workgroup
    auto resident_lds = [&](int ncg) { return (size_t)xb4_kp(K, xb4_u(FV, ncg)) * xb4_stride(ncg) * 8; };
    auto xb4_resident = [&](int use) {
        return s.xb4 != 3 &&  // (PLS_HIP_XB4=3: the windowed form everywhere, for measurements)
               resident_lds((use + 3) / 4) <= 152 * 1024 && N / (16 * FV) >= (i64)2 * (XB4_WG / WAVE) * num_cu;
    };
    // the column-split shape: one row per lane cannot give every CU a workgroup (fp32: two -- its 4-byte accesses stream worse);
    // measured per shape, tools/xb_split_sweep.py: beyond that the row-parallel kernel is as fast or faster
    const bool split_shape = K >= 1024 && (N + WG - 1) / WG <= (i64)(f32 ? 2 : 1) * num_cu;
    // the windowed form: not for fp64 storage with 8 columns or fewer (the VALU kernel holds them in one sweep at 0.72-0.74 of
    // peak, this one 0.68), not for fp32 beyond 20 (its 24-column form spills)
    // ... unless those 8 would go down the column-split path (two sweeps: 20,000 x 2,000, 8 columns 0.126 against 0.055 ms)
    auto xb4_windowed = [&](int cols) { return f32 ? cols <= 20 : (cols > 8 || split_shape); };  // cols: ALL that remain
    const bool xb4_first = xb4_ok && (xb4_resident(std::min(C, f32 ? 24 : 32)) || xb4_windowed(C));
    // 1..4 columns of a TALL matrix (fitted values of a few responses; no sum of squares asked for): the resident form with one
    // column group -- three quarters of its MFMAs are padding and free; what counts is the tile walk (config 3, one column:
    // 0.71 -> 0.67 ms; fp32 0.41 -> 0.34)
    const bool xb4_few = s.xb4 && C <= 4 && !s.ss && s.x_vec && s.out_vec && K >= 128 && 36 * std::max(ldx, ldo) * es < ((i64)1 << 31) &&
                         xb4_big && xb4_resident(4);
    // dynamic LDS of xb_mfma4w_kernel: two windows of Bm, or the partial sums of a round's tiles
    auto windowed_lds = [&](int ncg) { return std::max((size_t)2 * (1 << xb4w_kcl2(FV, ncg)) * xb4_stride(ncg) * 8, (size_t)16 * FV * 64 * 8); };

    // VERY short and wide (fewer 16 FV-row tiles than CUs: 2,000 x 20,000, a usual shape of the method), 5 columns or more: the
    // windowed MFMA kernel with the columns split over blockIdx.y as well, fp64 partial sums, xb_split_finish_kernel behind it --
    // one sweep of X for up to 32 columns where the VALU split below makes one per 4.  A whole-call route.
    if (open(XB_MFMA4W_SPLIT) && s.xb4 && C > 4 && N > 0 && K >= 1024 && xb4_tiles < (i64)num_cu && s.x_vec &&
        36 * ldx * es < ((i64)1 << 31) && xb4_big) {
        const int use = std::min(rem, f32 ? 20 : 32);
        const int ncg = std::max(2, (use + 3) / 4), kc = 1 << xb4w_kcl2(FV, ncg);
        st.sw = 16;  // one tile per workgroup: its 16 waves share the columns of every window
        const int kspl = (int)std::min<i64>((2 * (i64)num_cu + xb4_tiles - 1) / xb4_tiles, std::max(1, K / (2 * kc)));
        st.kper = ((K + kspl - 1) / kspl + kc - 1) / kc * kc;
        st.ks = (K + st.kper - 1) / st.kper;
        st.gy = (unsigned)st.ks;
        st.lds = windowed_lds(ncg);
        st.ldp = (N + 63) / 64 * 64;
        st.part_bytes = (size_t)st.ks * (4 * ncg) * st.ldp * 8;
        return done(XB_MFMA4W_SPLIT, use, FV, ncg, xb4_tiles);
    }
    // One score column (or a few) of a short, wide matrix: the rows alone give fewer workgroups than there are CUs -- split the
    // columns as well (xb_split_kernel); ~3 workgroups per CU, at least 128 columns each.  A whole-call route.
    // (not when the matrix-core kernel takes the columns in one pass (`many`): 32 columns on 131,072 x 4,096 fp32 were eight
    // sweeps of this path, 2.6 instead of 0.75 ms -- profiles/r4/products_scan.txt; nor when the 4 x 4 x 4 kernels do)
    if (open(XB_SPLIT) && N > 0 && split_shape && !many && !xb4_first && !xb4_few) {
        const bool v2 = s.x_vec && (N + (i64)FV * WG - 1) / ((i64)FV * WG) >= 8;
        const i64 per = (i64)WG * (v2 ? FV : 1), rg = (N + per - 1) / per;
        int KS = (int)std::min<i64>(K / 128, (3 * (i64)num_cu + rg - 1) / rg);
        const int kper = (K + KS - 1) / KS;
        KS = (K + kper - 1) / kper;
        if (KS >= 2) {
            const int mt = C > 2 ? 4 : (C > 1 ? 2 : 1);  // columns per sweep of X, fixed for the call
            st.kper = kper;
            st.ks = KS;
            st.gy = (unsigned)KS;
            st.ldp = (N + 63) / 64 * 64;
            st.part_bytes = (size_t)KS * mt * st.ldp * 8;
            return done(XB_SPLIT, std::min(mt, rem), v2 ? FV : 1, mt, rg);
        }
    }
    if (!f32 && rem > 32 && s.x_vec) {
        // fp64 storage beyond the 32 columns a pass of the LDS-staged VALU kernel holds: up to 64 per pass on the matrix
        // cores with Bm in LDS (1,048,576 x 512, 64 columns: one pass instead of two of 1.27 ms)
        const int use = std::min(rem, 64);
        return done(XB_MFMA_LDS, use, FV, use > 48 ? 4 : 3, (N + rows_per_wg_many - 1) / rows_per_wg_many);
    }
    if (open(XB_MFMA4) && ((rem > 4 && xb4_ok) || xb4_few)) {
        // 5..32 columns (fp32 storage: ..24) with all of Bm in LDS: the 4 x 4 x 4 MFMA form, columns padded to 4 (xb_mfma4.hpp)
        const int use = std::min(rem, f32 ? 24 : 32);
        if (xb4_resident(use)) {
            const int ncg = (use + 3) / 4, waves = XB4_WG / WAVE;
            st.lds = resident_lds(ncg);
            return done(XB_MFMA4, use, FV, ncg, std::min<i64>(num_cu, (xb4_tiles + waves - 1) / waves));
        }
    }
    if (open(XB_MFMA4W) && rem > 4 && xb4_ok && xb4_windowed(rem)) {
        // the same product where Bm does not fit in LDS or the matrix has too few row tiles for a wave each: Bm in windows,
        // the waves of a workgroup = tile slots x sub-windows (xb_mfma4w.hpp)
        const int use = std::min(rem, f32 ? 20 : 32), ncg = (use + 3) / 4;
        const i64 grid = std::min<i64>(num_cu, xb4_tiles), tpw = (xb4_tiles + grid - 1) / grid;
        int tw = 16;
        for (int cand : {8, 4, 2})
            if ((tpw + cand - 1) / cand * cand < (tpw + tw - 1) / tw * tw) tw = cand;
        st.sw = 16 / tw;
        st.lds = windowed_lds(ncg);
        return done(XB_MFMA4W, use, FV, ncg, grid);
    }
    if (f32 && rem > 8 && s.x_vec) {
        // fp32 storage, many columns: up to 32 per pass on the matrix cores (xb_mfma_lds_kernel) -- the LDS-staged
        // VALU kernel below holds only 8 columns of fp64 accumulators per pass at 4 rows per lane.  (For fp64
        // storage, where it takes 32 columns per pass, it is the faster one: 0.86 vs 1.04 ms at 20 columns.)
        const int use = std::min(rem, 32);
        return done(XB_MFMA_LDS, use, FV, use > 16 ? 2 : 1, (N + rows_per_wg_many - 1) / rows_per_wg_many);
    }
    if (rem > 4) {
        // many columns: Bm through LDS, up to `cap` columns per pass over X; the tile is the column
        // count rounded up to a multiple of 4 (every extra column costs VEC fp64 FMAs per element)
        const int cap = wide ? (FV == 2 ? 32 : 8) : 32;  // fp32 x 4 rows per lane: 8 columns = 32 fp64 accumulators
        const int use = std::min(rem, cap), mtc = (use + 3) & ~3;
        // fp64, 13..20 columns on a large matrix: two row packs per lane (one LDS read of a B value feeds 4 FMAs)
        const bool two = wide && FV == 2 && mtc >= 16 && mtc <= 20 && N >= (i64)num_cu * 4 * WG * FV * 2;
        const i64 per = (i64)WG * (wide ? FV : 1) * (two ? 2 : 1);
        return done(two ? XB_WIDE2 : XB_WIDE, use, wide ? FV : 1, mtc, (N + per - 1) / per);
    }
    const int mt = rem > 2 ? 4 : rem > 1 ? 2 : 1;
    const i64 per = (i64)WG * (wide ? FV : 1);
    st.ss = s.ss && mt == 1;
    return done(XB_KERNEL, std::min(mt, rem), wide ? FV : 1, mt, (N + per - 1) / per);
}

}  // namespace plsk
