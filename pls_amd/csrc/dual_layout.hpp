// dual_layout.hpp -- ItemLayout: the one description of the workspace slab of a round of the sample-space plans, and the four
// slabs there are.  Plain C++17: no HIP, no handle (tests/cpp/dual_round.cpp compiles it alone).
//
// A round of nround items keeps every field of all its items together: [field 0 of item 0 .. nround-1 | field 1 of ... | ...],
// so that a kernel with a workgroup per item indexes every field by blockIdx.x alone.  The slab's size (what sizes the round
// and the allocation) and the address of every field (what the kernels are given) both come from the same list of sizes.
#pragma once

#include <cstdint>
#include <initializer_list>

namespace plsk {

typedef int64_t i64;

struct ItemLayout {
    static constexpr int MAX_FIELDS = 12;
    i64 off[MAX_FIELDS + 1] = {0};  // doubles of one item before field i; off[n]: doubles of one item
    int n = 0;
    bool ok = true;  // false: more than MAX_FIELDS fields were asked for (DualRounds::open refuses the layout)
    i64 ints = 0;  // a trailing field of `ints` 4-byte integers per item, behind the doubles (pos of cv_folds_dual)

    ItemLayout() = default;
    ItemLayout(std::initializer_list<i64> doubles) { append(doubles); }
    // the same fields, then `more`: the slab of a caller that adds state to another caller's items
    ItemLayout extended(std::initializer_list<i64> more) const {
        ItemLayout l = *this;
        l.append(more);
        return l;
    }
    ItemLayout with_ints(i64 count) const {
        ItemLayout l = *this;
        l.ints = count;
        return l;
    }
    i64 bytes_per_item() const { return off[n] * 8 + ints * 4; }
    double *field(double *base, i64 nround, int i) const { return base + nround * off[i]; }
    int *int_field(double *base, i64 nround) const { return reinterpret_cast<int *>(base + nround * off[n]); }

  private:
    void append(std::initializer_list<i64> doubles) {
        for (i64 d : doubles) {
            if (n == MAX_FIELDS) {
                ok = false;
                return;
            }
            off[n + 1] = off[n] + d;
            ++n;
        }
    }
};

// Every slab begins [Y_a | Z]: the working copy of the responses and the product Z = G [.] of the round (N x M each).
enum { DUAL_YA = 0, DUAL_Z = 1 };

// A fold (plan_dual_cv.hpp): Y_a and Z, the scores (N x A), tt (A), g and c (N + A), the predictions (ts x M); pos (N ints)
enum { CV_T = 2, CV_TT, CV_SCR, CV_PRED };
inline ItemLayout cv_fold_doubles(i64 N, i64 M, i64 A, i64 ts) { return ItemLayout{N * M, N * M, N * A, A, N + A, ts * M}; }
inline ItemLayout cv_dual_layout(i64 N, i64 M, i64 A, i64 ts) { return cv_fold_doubles(N, M, A, ts).with_ints(N); }

// A (problem, fold) pair (plan_dual_cvbatch.hpp): a fold's doubles (pos exists once per fold, elsewhere), then the held-out
// responses and the residuals by test position (ts x M each), the partial PRESS (M x A) and ssy (M)
enum { CVB_YTE = CV_PRED + 1, CVB_ESCR, CVB_PRESS, CVB_SSY };
inline ItemLayout cvbatch_layout(i64 N, i64 M, i64 A, i64 ts) {
    return cv_fold_doubles(N, M, A, ts).extended({ts * M, ts * M, M * A, M});
}

// A problem of a batch (plan_dual_batch.hpp): Y_a and Z (D reuses Z), T and U (N x A; S overwrites U), C (A x A), Q (M x A),
// tt (A), g and c (N + A)
enum { BAT_T = 2, BAT_U, BAT_C, BAT_Q, BAT_TT, BAT_SCR };
inline ItemLayout batch_dual_layout(i64 N, i64 M, i64 A) { return ItemLayout{N * M, N * M, N * A, N * A, A * A, M * A, A, N + A}; }

// A replicate (plan_resample.hpp): a problem's state, then s (N) and the product's input s o Y~_a (N x M)
enum { RS_S = BAT_SCR + 1, RS_YIN };
inline ItemLayout resample_layout(i64 N, i64 M, i64 A) { return batch_dual_layout(N, M, A).extended({N, N * M}); }

}  // namespace plsk
