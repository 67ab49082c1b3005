// dual_round.hpp -- DualRounds: the round driver every multi-item caller of the sample-space plan shares (cv_folds_dual,
// fit_batch_dual, fit_resampled_dual, cv_press_batch_dual).  G = X X^T once, then the items in rounds; per component a round
// costs one product Z = G [the product's input of every item] and one step launch of the caller, a workgroup per item.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
//   open()  G (the only pass over X the driver makes), the round's size from what is left of the device memory, the slab
//   run()   the round loop: init(i0, nb), per component the product and step(i0, nb, a), then after(i0, nb)
// Between the two the caller names its fields (field(), dual_layout.hpp) and launches what it needs once per call.
#pragma once

#include "dual_layout.hpp"

namespace {

struct DualRounds {
    plsk::ItemLayout lay;
    i64 items = 0, nround = 0;  // items of the call, per round
    double *base = nullptr;
    // One product kernel for the whole call, so that the bits of an item do not depend on the round it falls into: the
    // single-wave rows of dual_gy_kernel up to 32 columns per round (the 128-wide tile of the matrix-core kernel would be
    // mostly padding), xtg_kernel with X := G beyond (G is symmetric)
    bool gy = false;

    double *field(int i) const { return lay.field(base, nround, i); }
    int *int_field() const { return lay.int_field(base, nround); }

    // G = X X^T and the slab of a round in `slab`.  The caller has ensured whatever else the call keeps on the device: the
    // round is sized by what is left, as many items as 4 GB and half of the free device memory hold of per-item layout +
    // extra_bytes, at most value_cap and env_cap.  PLS_HIP_ERR_ALLOC with sz.refusal: not even one item fits.
    struct Sizing {
        i64 items = 0;        // of the whole call
        i64 extra_bytes = 0;  // workspace of the caller's own per item, beside the slab
        i64 value_cap = 0;    // most items a round may have (index ranges)
        i64 env_cap = 0;      // the caller's PLS_HIP_*_ROUND (> 0: the test knob)
        const char *refusal = "";
    };
    template <typename T>
    int open(pls_hip_context *c, const T *X, i64 ldx, int N, int K, int M, const plsk::ItemLayout &layout, const Sizing &sz, DevBuf &slab) {
        if (!layout.ok) return fail(c, PLS_HIP_ERR_INVALID, "internal: a round's layout has more fields than ItemLayout holds");
        // G and the partial blocks of its sweep first: the round is sized by what they leave
        CHK(ensure(c, c->dG, (size_t)N * N * 8));
        CHK(dual_gram<T>(c, X, ldx, N, K));
        lay = layout;
        items = sz.items;
        nround = round_size(lay.bytes_per_item() + sz.extra_bytes, sz.value_cap, sz.env_cap, items);
        if (nround < 1) return fail(c, PLS_HIP_ERR_ALLOC, sz.refusal);
        CHK(ensure(c, slab, (size_t)(nround * lay.bytes_per_item())));
        base = (double *)slab.p;
        gy = nround * M <= 32;
        return PLS_HIP_OK;
    }

    // The rounds.  `feed`: the field the product reads (Y_a, or s o Y~_a of the weighted mode); Z is field DUAL_Z.  The
    // callables return a status; `after` returns PLS_HIP_OK early for what a round has no use for.
    template <typename Init, typename Step, typename After>
    int run(pls_hip_context *c, int N, int M, int A, int feed, const char *round_text, Init &&init, Step &&step,
            After &&after) const {
        const double *G = (const double *)c->dG.p, *in = field(feed);
        double *Z = field(plsk::DUAL_Z);
        for (i64 i0 = 0; i0 < items; i0 += nround) {
            Range r_round(round_text, (int)(i0 / nround));
            const i64 nb = std::min(nround, items - i0);
            const int C = (int)(nb * M);
            CHK(init(i0, nb));
            for (int a = 0; a < A; ++a) {
                if (gy) CHK(launch_dual_gy(c, G, in, N, C, Z));
                else CHK(launch_sym_product(c, G, N, in, (i64)N, C, Z, (i64)N));
                CHK(step(i0, nb, a));
            }
            CHK(after(i0, nb));
        }
        return PLS_HIP_OK;
    }
};

}  // namespace
