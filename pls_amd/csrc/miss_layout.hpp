// miss_layout.hpp -- the sweep geometry of the missing-value plans and the workspace slab of a fold of
// pls_hip_cv_folds_missing: miss_row_split, the K split of every row sweep of the family (the diagnostics' streaming route
// included), miss_geom_of, a pure function of (N, K, element size, CU count), and MissCvLayout, the byte offsets
// of a fold's fields and the fold's byte count.  The same MissCvLayout sizes the round (plan_missing_cv.hpp) and is handed to
// the kernels that carve the slab (missing_cv_kernels.hpp).  Plain C++17, no HIP and no handle: tests/cpp/missing_cv_layout.cpp
// builds it with the host compiler alone.
#pragma once
#include "xb_route.hpp"  // i64, WG

namespace plsk {

constexpr int MISS_KC = 8;        // columns per workgroup of the column sweep: 2 x 8 fp64 accumulators per lane
constexpr int MISS_RF_ROWS = 16;  // rows per workgroup of the kernels that add the K ranges of a row sweep (miss_ranges_sum)

// geometry of the three sweeps of one call; the work copy has 16-byte columns (ldw a multiple of 16 / element size)
struct MissGeom {
    i64 ldw;
    int G;        // row groups (partial rows) of the column sweep
    i64 nkg;      // its column groups
    int lrl;      // row sweep: log2 of the row lanes of a workgroup
    i64 nrb;      //            row blocks
    int S, kper;  //            K ranges (1: no partials) and the columns of one
    int GY;       // workgroups of the row-chunked kernels of the Y side
    i64 nbK, nbN;  // blocks of the K- and N-parallel kernels
};

// The split of a row sweep (miss_row_walk of missing_kernels.hpp): a lane owns `vec` rows, a workgroup is RL = 1 << lrl row
// lanes x CL = WG / RL column lanes, and K is cut into S ranges of kper columns (a multiple of CL) where the nrb row blocks
// alone do not fill the chip.  The one copy of the rule: miss_geom_of and xdiagmiss_geom_of (xdiagmiss_layout.hpp) call it.
struct MissRowSplit {
    int lrl;      // log2 of the row lanes of a workgroup
    i64 nrb;      // row blocks
    int S, kper;  // K ranges (1: no partials) and the columns of one
};

inline MissRowSplit miss_row_split(i64 N, i64 K, int vec, int num_cu) {
    MissRowSplit s;
    const i64 nv = (N + vec - 1) / vec;
    s.lrl = 0;
    while ((1 << s.lrl) < WG && ((i64)1 << s.lrl) < nv) ++s.lrl;
    const int RL = 1 << s.lrl, CL = WG >> s.lrl;
    s.nrb = (nv + RL - 1) / RL;
    const i64 smax = std::max<i64>(1, K / (8 * CL));  // at least 8 columns per lane of a range
    const i64 S = std::min<i64>(std::min<i64>(std::max<i64>(1, (4 * (i64)num_cu) / s.nrb), smax), 65535);
    i64 kper = (K + S - 1) / S;
    kper += (-kper) & (CL - 1);
    s.kper = (int)std::min<i64>(kper, ((i64)1 << 31) - 1);
    s.S = (int)((K + s.kper - 1) / s.kper);
    return s;
}

inline MissGeom miss_geom_of(i64 N, i64 K, int es, int num_cu) {
    const int FV = 16 / es;
    MissGeom g;
    g.ldw = N + ((-N) & (FV - 1));
    g.nkg = (K + MISS_KC - 1) / MISS_KC;
    // the worst case of the row chunks (a caller's matrix that is not 16-byte aligned is walked one row per lane)
    const i64 nch = (N + WG - 1) / WG;
    // 5 workgroups per CU are resident at the 89 VGPRs of the deflating sweep: all of them in one round, no tail
    g.G = (int)std::min<i64>(std::min<i64>(std::max<i64>(1, (5 * (i64)num_cu) / g.nkg), nch), 65535);
    const MissRowSplit s = miss_row_split(N, K, FV, num_cu);
    g.lrl = s.lrl;
    g.nrb = s.nrb;
    g.S = s.S;
    g.kper = s.kper;
    g.GY = (int)std::min<i64>(nch, 2 * (i64)num_cu);
    g.nbK = (K + WG - 1) / WG;
    g.nbN = nch;
    return g;
}

// ---- the slab of a fold of pls_hip_cv_folds_missing ---------------------------------------------------------------------------
// A round of nround folds is nround slabs of `bytes` bytes, fold f of the round at base + f * bytes; every field begins on a
// 16-byte boundary of its slab and `bytes` is a multiple of 16, so that the work copy of every fold is aligned alike.
enum MissCvField {
    MCV_WORK = 0,  // the work copy of X: ldw x K elements of the storage type
    MCV_YA,        // the work copy of Y: N x M
    MCV_MASK,      // m: 1 on the training rows of the fold, 0 on its held-out rows (N)
    MCV_U,         // u~ = m o u (N)
    MCV_T,         // t, every row (N)
    MCV_TM,        // t~ = m o t (N)
    MCV_TPREV,     // t~ of the iteration before (N)
    MCV_W,         // w of the component (K)
    MCV_P,         // p of the component (K)
    MCV_Q,         // q of every component (M x A)
    MCV_COLPART,   // partial rows of the column sweep: G x K x {num, den}
    MCV_SSPART,    // block sums of squares of w (nbK)
    MCV_TPART,     // partials of the K-split row sweep: S x N x {num, den}; S = 1: empty
    MCV_YPART,     // partial rows of Y~^T t~, t~^T t~, |t~ - t~_prev|^2: GY x (M + 2)
    MCV_YSS,       // partial sums of squares of the columns of Y_a over the training rows: GY x M
    MCV_QQ,        // q^T q (2 doubles)
    MCV_WORDS,     // two ints: the column of Y_a that starts u, the convergence word (16 bytes)
    MCV_FIELDS
};

struct MissCvLayout {
    i64 off[MCV_FIELDS + 1];  // byte offset of field i in a fold's slab; off[MCV_FIELDS] = bytes
    i64 bytes;                // of one fold
};

inline MissCvLayout miss_cv_layout(i64 N, i64 K, i64 M, i64 A, int es, int num_cu) {
    const MissGeom g = miss_geom_of(N, K, es, num_cu);
    const i64 size[MCV_FIELDS] = {g.ldw * K * es, N * M * 8, N * 8, N * 8, N * 8, N * 8, N * 8, K * 8, K * 8, M * A * 8,
                                  (i64)g.G * K * 16, g.nbK * 8, g.S > 1 ? (i64)g.S * N * 16 : 0, (i64)g.GY * (M + 2) * 8,
                                  (i64)g.GY * M * 8, 16, 16};
    MissCvLayout l;
    i64 at = 0;
    for (int i = 0; i < MCV_FIELDS; ++i) {
        l.off[i] = at;
        at += (size[i] + 15) & ~(i64)15;
    }
    l.off[MCV_FIELDS] = l.bytes = at;
    return l;
}

}  // namespace plsk
