// plan_batch.hpp -- pls_hip_fit_batch: many response sets against one X.  The sample-space route of plan_dual_batch.hpp under
// PLS_HIP_ALGO_DUAL; otherwise the batched route (X^T X once, the wide X^T [Y_0 | Y_1 | ...]
// on the matrix cores, two launches per component for all problems of a round) and the per-problem route (one KERNEL_TYPE2 fit each).
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

constexpr i64 BATCH_MSG_CAP = (i64)1 << 20;    // values per slice of a message of whole problems on a sharded handle
constexpr int BATCH_CB = 32;                   // column block of the fallback product (launch_xty)

// the batched route's shapes: the bounds of cv_folds_kernel (everything M-sized in one workgroup's LDS, X^T X resident)
bool batch_covers(const pls_hip_context *c, i64 K, i64 M, i64 A) {
    return !c->env.batch_refit && A <= 4096 && K <= 16384 && (M == 1 || M <= plsk::MMAX);
}

// XX (K x K) summed over the ranks into c->xx: from the upload that formed this member's part, or from X
template <typename T>
int batch_xx(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K) {
    const i64 KK = (i64)K * K;
    CHK(ensure(c, c->xx, (size_t)KK * 8));
    if (c->pre_xx) {
        CHK(ensure(c, c->red2, (size_t)plsk::RED_SLICES * KK * 8));
        hipLaunchKernelGGL(plsk::fill_slices_kernel, dim3((unsigned)((KK + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream,
                           c->pre_xx, (int)KK, (double *)c->red2.p);
        LAUNCH_CHECK(c);
        return compute_xx_finish(c, K, (double *)c->xx.p);
    }
    return compute_xx<T>(c, X, ldx, N, K, (double *)c->xx.p);
}

// red (RED_SLICES slices of K x C, slice stride K * C) = this rank's X^T G, G = C columns (ld ldg)
template <typename T>
int batch_xtg(pls_hip_context *c, const T *X, i64 ldx, const T *G, i64 ldg, i64 N, int K, i64 C, double *red) {
    constexpr int V = plsk::SyrkCfg<T>::V, RB = plsk::SyrkCfg<T>::RB;
    const i64 KC = (i64)K * C;
    const bool mfma = ((uintptr_t)X % 16) == 0 && ((uintptr_t)G % 16) == 0 && ldx % V == 0 && ldg % V == 0;
    if (mfma) {
        const int nbk = (K + plsk::SYRK_TB - 1) / plsk::SYRK_TB, nbc = (int)((C + plsk::SYRK_TB - 1) / plsk::SYRK_TB);
        const i64 nblocks = (i64)nbk * nbc, slots = 2 * (i64)c->num_cu, nslabs = (N + RB - 1) / RB;
        i64 S = plsk::row_splits(nblocks, slots, 8);
        S = std::max<i64>(1, std::min<i64>(std::min<i64>(S, nslabs), 64));
        while (S > 1 && S * KC * 8 > ((i64)1 << 30)) --S;
        if (ensure(c, c->part, (size_t)S * KC * 8) == PLS_HIP_OK &&
            plsk::raise_dynamic_lds((const void *)plsk::xtg_kernel<T, false>, (int)plsk::SyrkCfg<T>::LDS_BYTES)) {
            {
                Scope s(c, PLS_HIP_FAM_XTY, (i64)N * K * sizeof(T) * nbc + (i64)N * C * sizeof(T) * nbk + S * KC * 8);
                hipLaunchKernelGGL((plsk::xtg_kernel<T, false>), dim3((unsigned)nblocks, (unsigned)S), dim3(256), plsk::SyrkCfg<T>::LDS_BYTES,
                                   c->stream, X, ldx, G, ldg, N, K, (int)C, nbc, 1, (double *)c->part.p, (i64)K, KC);
                LAUNCH_CHECK(c);
            }
            return launch_reduce(c, (const double *)c->part.p, (int)S, (int)KC, nullptr, 0, red);
        }
        c->err.clear();
    }
    // layouts the matrix-core kernel declines (odd ld, pointers aligned to 8 bytes only): the column-reduction kernel in blocks of
    // 32 columns, into the same slices -- as compute_xx_local falls back
    CHK(ensure(c, c->part, (size_t)max_partial_rows(c, N, K) * (size_t)K * BATCH_CB * 8));
    for (i64 c0 = 0; c0 < C; c0 += BATCH_CB) {
        const int cb = (int)std::min<i64>(BATCH_CB, C - c0);
        int nb = 0;
        CHK(launch_xty<T>(c, X, ldx, G + c0 * ldg, ldg, N, K, cb, (double *)c->part.p, &nb));
        CHK(launch_reduce(c, (const double *)c->part.p, nb, K * cb, nullptr, 0, red + c0 * K, KC));
    }
    return PLS_HIP_OK;
}

// problems per round of the batched route: as many as 4 GB and half of the free device memory hold (0: not even one)
i64 batch_round_size(pls_hip_context *c, i64 K, i64 M, i64 A, i64 nprob) {
    const plsk::BatchLayout L((int)K, (int)M, (int)A);
    const i64 KP = K + (K & 1);
    // workspace, V and r columns, the sliced product and the message, and the row-split partial blocks of the product
    const i64 per = (L.total + 2 * KP + plsk::RED_SLICES * (2 * K + 1) * M + M) * 8 + 16 * K * M * 8;
    // K * C and a message slice stay below 2^31 values
    return round_size(per, ((i64)1 << 30) / std::max<i64>(1, (K + 1) * M), c->env.batch_round, nprob);
}

// The batched route on device pointers; any of R, Q, tt, B, ssy may be null.  PLS_HIP_ERR_ALLOC: workspace does not fit.
template <typename T>
int fit_batch_device(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, i64 N, int K, int M, int A, i64 nprob,
                     double *R, double *Q, double *tt, double *B, double *ssy) {
    const plsk::BatchLayout L(K, M, A);
    const i64 nround = batch_round_size(c, K, M, A, nprob);
    if (nround < 1) return fail(c, PLS_HIP_ERR_ALLOC, "fit_batch: the workspace of one problem does not fit");
    const i64 KP = K + (K & 1), per = (i64)(K + 1) * M;
    const i64 Cmax = nround * M;
    const i64 piece = c->reducer ? std::max<i64>(1, BATCH_MSG_CAP / per) : nround;  // whole problems per message
    CHK(ensure(c, c->bws, (size_t)nround * L.total * 8));
    CHK(ensure(c, c->bv, (size_t)2 * KP * nround * 8));
    CHK(ensure(c, c->bred, (size_t)plsk::RED_SLICES * K * Cmax * 8));
    CHK(ensure(c, c->bmsg, (size_t)plsk::RED_SLICES * per * std::min(piece, nround) * 8));
    CHK(ensure(c, c->bssy, (size_t)Cmax * 8));
    CHK(batch_xx<T>(c, X, ldx, N, K));
    const double *XX = (const double *)c->xx.p;
    double *ws = (double *)c->bws.p, *Vm = (double *)c->bv.p, *Rc = Vm + KP * nround;
    double *red = (double *)c->bred.p, *msg = (double *)c->bmsg.p, *sv = (double *)c->bssy.p;
    const size_t cs_bytes = (size_t)A * 8;
    for (i64 b0 = 0; b0 < nprob; b0 += nround) {
        const i64 nb = std::min(nround, nprob - b0), C = nb * M, KC = (i64)K * C;
        const T *G = Ys + b0 * M * ldy;
        if (N > 0) {
            CHK(batch_xtg<T>(c, X, ldx, G, ldy, N, K, C, red));
            hipLaunchKernelGGL((plsk::batch_ssy_kernel<T>), dim3((unsigned)C), dim3(plsk::WG), 0, c->stream, G, ldy, N, sv);
            LAUNCH_CHECK(c);
        }
        for (i64 p0 = 0; p0 < nb; p0 += piece) {
            const i64 np = std::min(piece, nb - p0), Lm = per * np;
            if (N > 0) {
                const unsigned g = (unsigned)std::min<i64>((Lm + plsk::WG - 1) / plsk::WG, 8192);
                hipLaunchKernelGGL(plsk::batch_pack_kernel, dim3(g), dim3(plsk::WG), 0, c->stream, (const double *)red, KC,
                                   (const double *)sv, K, M, p0 * M, Lm, msg);
                LAUNCH_CHECK(c);
            } else {
                HIPCHK(c, hipMemsetAsync(msg, 0, (size_t)plsk::RED_SLICES * Lm * 8, c->stream));  // an empty shard
            }
            CHK(do_allreduce(c, msg, (i64)plsk::RED_SLICES * Lm));
            hipLaunchKernelGGL(plsk::batch_step_kernel, dim3((unsigned)np), dim3(plsk::UPD_THREADS), cs_bytes, c->stream,
                               (const double *)msg, Lm, (const double *)Vm, Rc, KP, ws, (int)p0, K, M, A, -1, (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
        for (int a = 0; a < A; ++a) {
            CHK(launch_sym_product(c, XX, K, Rc, KP, (int)nb, Vm, KP));  // V = XX [r_0 r_1 ...]
            Scope s(c, PLS_HIP_FAM_SMALL, nb * ((i64)K * M * 3 + (i64)K * (2 * (a + 2)) + 2 * K) * 8);
            hipLaunchKernelGGL(plsk::batch_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), cs_bytes, c->stream,
                               (const double *)nullptr, (i64)0, (const double *)Vm, Rc, KP, ws, 0, K, M, A, a, (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
        if (R || Q || tt || B || ssy) {
            hipLaunchKernelGGL(plsk::batch_finish_kernel, dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, (const double *)ws, K, M, A,
                               b0, R, Q, tt, B, ssy);
            LAUNCH_CHECK(c);
        }
    }
    return PLS_HIP_OK;
}

// The per-problem route: one KERNEL_TYPE2 fit per problem under the handle's plan (its own collectives on a sharded handle),
// tt from the X^T X that fit left in the workspace, ssy from a column sweep (one message of RED_SLICES * M on a sharded handle).
template <typename T>
int fit_batch_refit(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, i64 N, int K, int M, int A, i64 nprob,
                    double *R, double *Q, double *tt, double *B, double *ssy) {
    const i64 KA = (i64)K * A, MA = (i64)M * A;
    CHK(ensure(c, c->bws, (size_t)(3 * KA + MA + M) * 8));
    CHK(ensure(c, c->bmsg, (size_t)plsk::RED_SLICES * M * 8));
    double *Wf = (double *)c->bws.p, *Pf = Wf + KA, *Rf = Pf + KA, *Qf = Rf + KA, *sv = Qf + MA;
    double *msg = (double *)c->bmsg.p;
    const double *saved_xx = c->pre_xx, *saved_xy = c->pre_xy;  // (X^T Y of an upload belongs to another Y)
    c->pre_xx = c->pre_xy = nullptr;
    int rc = PLS_HIP_OK;
    for (i64 b = 0; b < nprob && rc == PLS_HIP_OK; ++b) {
        const T *Yb = Ys + b * M * ldy;
        rc = fit_device<T>(c, X, ldx, Yb, ldy, N, K, M, A, PLS_HIP_KERNEL_TYPE2, Wf, Pf, Qf, Rf, (T *)nullptr, 0,
                           B ? B + b * K * M : nullptr);
        if (rc != PLS_HIP_OK) break;
        if (R && hipMemcpyAsync(R + b * KA, Rf, (size_t)KA * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) rc = PLS_HIP_ERR_DEVICE;
        if (Q && hipMemcpyAsync(Q + b * MA, Qf, (size_t)MA * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) rc = PLS_HIP_ERR_DEVICE;
        if (rc != PLS_HIP_OK) { c->err = "fit_batch: copy of a problem's results failed"; break; }
        if (tt) {
            hipLaunchKernelGGL(plsk::batch_tt_kernel, dim3((unsigned)A), dim3(plsk::WG), 0, c->stream, (const double *)c->xx.p,
                               (const double *)Rf, K, tt + b * A);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_batch: launch failed"); break; }
        }
        if (ssy) {
            if (N > 0) hipLaunchKernelGGL((plsk::batch_ssy_kernel<T>), dim3((unsigned)M), dim3(plsk::WG), 0, c->stream, Yb, ldy, N, sv);
            else if (hipMemsetAsync(sv, 0, (size_t)M * 8, c->stream) != hipSuccess) rc = PLS_HIP_ERR_DEVICE;
            hipLaunchKernelGGL(plsk::fill_slices_kernel, dim3((unsigned)((M + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream,
                               (const double *)sv, M, msg);
            if (rc != PLS_HIP_OK || hipGetLastError() != hipSuccess) { rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_batch: launch failed"); break; }
            rc = do_allreduce(c, msg, (i64)plsk::RED_SLICES * M);
            if (rc != PLS_HIP_OK) break;
            hipLaunchKernelGGL(plsk::sum_slices_kernel, dim3((unsigned)((M + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream,
                               (const double *)msg, M, ssy + b * M);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_batch: launch failed"); break; }
        }
    }
    c->pre_xx = saved_xx;
    c->pre_xy = saved_xy;
    return rc;
}

// pls_hip_fit_batch behind its argument checks
int fit_batch_impl(pls_hip_context *h, const void *X, i64 ldx, const void *Ys, i64 ldy, i64 N, i64 K, i64 M, i64 A, i64 nprob,
                   int dtype, int mem, double *R, double *Q, double *tt, double *B, double *ssy) {
    const size_t es = esize(dtype);
    const i64 C = nprob * M;
    const void *dX = X, *dY = Ys;
    i64 dldx = ldx, dldy = ldy;
    double *dR = R, *dQ = Q, *dtt = tt, *dB = B, *dssy = ssy;
    const i64 ldn = ld_quad(N);
    HostCall hc(h, mem);
    CHK(hc.out(dR, R, h->boR, K * A, nprob));
    CHK(hc.out(dQ, Q, h->boQ, M * A, nprob));
    CHK(hc.out(dtt, tt, h->bott, A, nprob));
    CHK(hc.out(dB, B, h->boB, K * M, nprob));
    CHK(hc.out(dssy, ssy, h->bossy, M, nprob));
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Ys, ldy, h->bY, N, C, es, ldn));
    int rc = PLS_HIP_ERR_ALLOC;
    if (batch_dual_covers(h, N, M)) {  // the sample-space plan, an explicit opt-in: every problem from one X X^T
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return fit_batch_dual<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, (int)N, K, (int)M, (int)A, nprob, dR, dQ, dtt, dB, dssy);
        });
        if (rc == PLS_HIP_ERR_ALLOC) h->err.clear();  // its workspace does not fit: the routes below
    }
    const bool dual = rc != PLS_HIP_ERR_ALLOC;  // (the sample-space route took the call)
    const bool batched = !dual && batch_covers(h, K, M, A);
    if (batched)
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return fit_batch_device<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, nprob, dR, dQ, dtt, dB, dssy);
        });
    // declined, or (single rank: the ranks of a sharded handle must not differ in their route) no room for the batched workspace
    if (!dual && (!batched || (rc == PLS_HIP_ERR_ALLOC && !h->reducer))) {
        h->err.clear();
        if (M > plsk::LM_MAX || K > 32768)
            return fail(h, PLS_HIP_ERR_UNSUPPORTED, "fit_batch: the per-problem route is pls_hip_fit's: M <= 1024, K <= 32768");
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return fit_batch_refit<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, nprob, dR, dQ, dtt, dB, dssy);
        });
    }
    if (rc != PLS_HIP_OK) return rc;
    return hc.finish(true);
}

}  // namespace
