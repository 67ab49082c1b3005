// xdiagmiss_layout.hpp -- the route, the tile shape, the K split and the workspace of pls_hip_x_diagnostics_missing:
// xdiagmiss_geom_of, a pure function of (N, K, A, element size, CU count, alignment).  plan_xdiag_missing.hpp only executes what
// it returns.  Plain C++17, no HIP and no handle: tests/cpp/xdiagmiss_layout.cpp builds it with the host compiler alone.
//
// Row-resident route (tall X): a workgroup of WG lanes owns a tile of `rt` rows (a power of two, XDM_RT_MIN .. XDM_RT_MAX) and
// holds all K cells of each as fp64 in LDS, rt x K x 8 bytes <= XDM_TILE_BYTES, across all A components.  The tile is half of what
// a CU could give one workgroup: two workgroups share a CU, one loads while the other computes.  Thresholds:
//   K <= XDM_TILE_BYTES / (8 XDM_RT_MIN) = 1024                 (a row of 8-row tiles fits)
//   N >= XDM_RT_MIN num_cu                                      (8-row tiles alone give every CU one)
//   rt = min(pow2 floor of XDM_TILE_BYTES / (8 K), pow2 floor of N / num_cu, XDM_RT_MAX): the rows shrink before CUs go idle
// Streaming route (everything else): one read-only sweep per component, the row sweep of the fit with `vec` rows per lane; its
// K split is miss_row_split of miss_layout.hpp, and the ranges of a row are added in index order by a finish kernel.
#pragma once
#include "miss_layout.hpp"  // miss_row_split; i64, WG

namespace plsk {

enum XdmRoute { XDM_RESIDENT = 0, XDM_STREAM = 1 };

constexpr i64 XDM_LDS_CU = 160 << 10;     // LDS of a CU
constexpr i64 XDM_TILE_BYTES = 64 << 10;  // the resident tile of one workgroup
constexpr int XDM_RT_MIN = 8, XDM_RT_MAX = 64;
constexpr int XDM_HAND = 3;                                   // values a column lane hands over per component: num, den, q
constexpr i64 XDM_HAND_BYTES = 2 * (i64)WG * XDM_HAND * 8 + (i64)WG * 4;  // static LDS of the resident kernel: two parities of the hand-over, the cell counts
constexpr int XDM_PART = 4;                                   // values per row and K range of the streaming route: num, den, q, count
constexpr int XDM_RED_SLICES = 8;                             // == RED_SLICES (fit_route.hpp; held by a static_assert in the plan)

struct XdmGeom {
    int route;
    int vec;  // rows per lane of a load from X: 16 / es when the alignment allows it, else 1
    // resident
    int rt;         // rows of a tile
    i64 ntiles;     // workgroups
    i64 lds_bytes;  // dynamic LDS of a workgroup: rt x K x 8
    // streaming
    int lrl;      // log2 of the row lanes of a workgroup
    i64 nrb;      // row blocks
    int S, kper;  // K ranges and the columns of one
    // workspace, byte offsets into one buffer (every field on a 16-byte boundary); the worst case over what may be asked for
    i64 o_sd, o_q0, o_qd, o_part, o_red, o_tv, ws_bytes;
};

inline int xdm_pow2_floor(i64 v, int cap) {
    int p = 1;
    while (2 * (i64)p <= v && 2 * p <= cap) p *= 2;
    return p;
}

// aligned: pointer and leading dimension of X allow 16-byte loads.  force_stream: PLS_HIP_XDIAGMISS_ROUTE=stream.
inline XdmGeom xdiagmiss_geom_of(i64 N, i64 K, i64 A, int es, int num_cu, bool aligned, bool force_stream = false) {
    XdmGeom g{};
    g.vec = aligned ? 16 / es : 1;
    const bool resident = !force_stream && K * 8 * XDM_RT_MIN <= XDM_TILE_BYTES && N >= (i64)XDM_RT_MIN * num_cu;
    g.route = resident ? XDM_RESIDENT : XDM_STREAM;
    if (resident) {
        g.rt = std::min(xdm_pow2_floor(XDM_TILE_BYTES / (8 * K), XDM_RT_MAX), xdm_pow2_floor(N / num_cu, XDM_RT_MAX));
        g.ntiles = (N + g.rt - 1) / g.rt;
        g.lds_bytes = (i64)g.rt * K * 8;
        g.S = 1;
        g.kper = (int)K;
    } else {
        const MissRowSplit s = miss_row_split(N, K, g.vec, num_cu);
        g.lrl = s.lrl;
        g.nrb = s.nrb;
        g.S = s.S;
        g.kper = s.kper;
    }
    i64 at = 0;
    auto take = [&](i64 bytes) { const i64 o = at; at += (bytes + 15) & ~(i64)15; return o; };
    g.o_sd = take(N * A * 8);                                          // the fp64 scores (ld N)
    g.o_q0 = take(N * 8);                                              // q_0
    g.o_qd = take(N * A * 8);                                          // q_1 .. q_A when ssx is asked for without Qres (ld N)
    g.o_part = take(resident ? 0 : (i64)g.S * N * XDM_PART * 8);       // the K ranges' partials of one sweep
    g.o_red = take((i64)XDM_RED_SLICES * (2 * A + 1) * 8);             // the slices of [ssx | sst]
    g.o_tv = take(A * 8);                                              // tvar of this call's own scores
    g.ws_bytes = at;
    return g;
}

}  // namespace plsk
