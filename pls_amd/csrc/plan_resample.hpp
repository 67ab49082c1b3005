// plan_resample.hpp -- pls_hip_fit_resampled: the same (X, Y) fitted under nrep sets of non-negative row weights (bootstrap,
// jack-knife, a case-weighted fit), the coefficients of every replicate and their summaries about the unit-weight fit.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// Sample-space route (fit_resampled_dual, under PLS_HIP_ALGO_DUAL): G = X X^T once, the replicates in rounds (DualRounds, dual_round.hpp); per component a
// round costs one product Z = G [s o Y~_a of every replicate] and one launch of resample_step_kernel, a workgroup per
// replicate (resample_kernels.hpp has the algebra).  B of a round is one product X^T [s o D(0) | s o D(1) | ...].  The
// unit-weight fit behind B0 and the summaries is replicate "-1": it leads the first round and takes every kernel a replicate
// takes, so a replicate of unit weights has B_b - B0 == 0 exactly.
// General route (fit_resampled_refit): one KERNEL_TYPE1 fit per replicate on row-scaled fp64 work copies of X and Y.
#pragma once

namespace {

// the calls the sample-space route takes (the conditions of batch_dual_covers); every other call takes the general route
bool resample_dual_covers(const pls_hip_context *c, i64 N, i64 M) {
    return N >= 1 && dual_rounds_cover(c, N, M) && !c->env.resample_refit;
}

// s1, s2 and (B0 not asked for) the unit-weight coefficients: c->rsacc, 3 K M doubles
int resample_accumulators(pls_hip_context *c, i64 KM, bool summary, double *B0, double *&s1, double *&s2, double *&B0d) {
    CHK(ensure(c, c->rsacc, (size_t)(3 * KM * 8)));
    s1 = (double *)c->rsacc.p;
    s2 = s1 + KM;
    B0d = B0 ? B0 : s2 + KM;
    if (summary) HIPCHK(c, hipMemsetAsync(s1, 0, (size_t)(2 * KM * 8), c->stream));
    return PLS_HIP_OK;
}

// s1, s2 += the nb replicates at Br (stride K M), in index order
int resample_accumulate(pls_hip_context *c, const double *Br, const double *B0d, i64 KM, i64 nb, double *s1, double *s2) {
    Scope s(c, PLS_HIP_FAM_SMALL, (nb + 5) * KM * 8);
    hipLaunchKernelGGL(plsk::resample_accum_kernel, dim3((unsigned)((KM + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream, Br,
                       B0d, KM, nb, s1, s2);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

int resample_finish(pls_hip_context *c, const double *B0d, const double *s1, const double *s2, i64 KM, i64 nrep, double *Bmean,
                    double *Bm2) {
    Scope s(c, PLS_HIP_FAM_SMALL, 5 * KM * 8);
    hipLaunchKernelGGL(plsk::resample_final_kernel, dim3((unsigned)((KM + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream,
                       B0d, s1, s2, KM, (double)nrep, Bmean, Bm2);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// X, Y, Wt device pointers; any of Q, tt, B, B0, Bmean, Bm2 (device memory) may be null.  PLS_HIP_ERR_ALLOC: the workspace
// does not fit.
template <typename T>
int fit_resampled_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, int N, i64 K, int M, int A, const double *Wt,
                       i64 ldw, i64 nrep, double *Q, double *tt, double *B, double *B0, double *Bmean, double *Bm2) {
    const i64 NM = (i64)N * M, NA = (i64)N * A, KM = K * M, MA = (i64)M * A, es = (i64)sizeof(T);
    const bool summary = Bmean || Bm2, need0 = B0 || summary;
    const i64 off = need0 ? 1 : 0, items = nrep + off;  // item i is replicate i - off; replicate -1: the unit-weight fit
    if (A > ((i64)1 << 20)) return fail(c, PLS_HIP_ERR_ALLOC, "fit_resampled: the workspace of one replicate does not fit");
    CHK(ensure(c, c->dY, (size_t)NM * 8));  // before G: the round is sized by what is left
    Range r_call("pls_hip_fit_resampled (sample space)");
    DualRounds r;
    // (the only pass over X unless B, B0, Bmean or Bm2 is asked for.)  A summary without B: the round's block of B is
    // workspace, K M doubles per replicate beside the slab
    DualRounds::Sizing sz;
    sz.items = items;
    sz.extra_bytes = summary && !B ? KM * 8 : 0;
    sz.value_cap = ((i64)1 << 30) / ((i64)N * std::max(M, A));
    sz.env_cap = c->env.resample_round;
    sz.refusal = "fit_resampled: the workspace of one replicate does not fit";
    CHK(r.open<T>(c, X, ldx, N, (int)K, M, plsk::resample_layout(N, M, A), sz, c->rsw));
    if (summary && !B) CHK(ensure(c, c->rsB, (size_t)(r.nround * KM * 8)));
    double *s1 = nullptr, *s2 = nullptr, *B0d = nullptr;
    if (need0) CHK(resample_accumulators(c, KM, summary, B0, s1, s2, B0d));
    double *Y64 = (double *)c->dY.p;
    double *Ya = r.field(plsk::DUAL_YA), *Z = r.field(plsk::DUAL_Z), *T64 = r.field(plsk::BAT_T), *U = r.field(plsk::BAT_U);
    double *C = r.field(plsk::BAT_C), *Qw = r.field(plsk::BAT_Q), *ttw = r.field(plsk::BAT_TT), *scr = r.field(plsk::BAT_SCR);
    double *sv = r.field(plsk::RS_S), *Yin = r.field(plsk::RS_YIN);
    // one back-projection kernel for the whole call, as the product has one (dual_round.hpp): the bits of a replicate do not
    // depend on the round it falls into
    const bool blocks = r.nround * M > plsk::XTV_NC;
    {
        Scope s(c, PLS_HIP_FAM_SMALL, NM * (es + 8));
        hipLaunchKernelGGL((plsk::dual_convert_kernel<T, double>), dim3((unsigned)((NM + 255) / 256)), dim3(256), 0, c->stream, Y, ldy,
                           Y64, (i64)N, N, M);
        LAUNCH_CHECK(c);
    }
    auto init = [&](i64 i0, i64 nb) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (3 * NM + 2 * (i64)N) * 8);
        hipLaunchKernelGGL(plsk::resample_init_kernel, dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, Wt, ldw, i0 - off,
                           (const double *)Y64, N, M, sv, Ya, Yin);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto step = [&](i64, i64 nb, int a) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (4 * M + a + 5) * 8);
        hipLaunchKernelGGL(plsk::resample_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                           T64, U, Qw, C, ttw, scr, (const double *)sv, Yin, N, M, A, a, (int)c->opt_power_iters);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto after = [&](i64 i0, i64 nb) -> int {
        const i64 rep0 = i0 - off;
        const i64 lead = rep0 < 0 ? 1 : 0, nr = nb - lead, r0 = rep0 + lead;  // the unit-weight fit leads the first round
        if (Q && nr > 0) HIPCHK(c, hipMemcpyAsync(Q + r0 * MA, Qw + lead * MA, (size_t)(nr * MA * 8), hipMemcpyDeviceToDevice, c->stream));
        if (tt && nr > 0) HIPCHK(c, hipMemcpyAsync(tt + r0 * A, ttw + lead * A, (size_t)(nr * A * 8), hipMemcpyDeviceToDevice, c->stream));
        const bool back = nr > 0 && (B || summary);  // the replicates' coefficients are wanted
        if (!lead && !back) return PLS_HIP_OK;
        {
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (2 * NA + (i64)A * A + MA + NM + N) * 8);
            hipLaunchKernelGGL(plsk::resample_sd_kernel, dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, U, (const double *)C,
                               (const double *)Qw, (const double *)sv, N, M, A, Z);
            LAUNCH_CHECK(c);
        }
        Range r_b("X^T [s o D]");
        if (lead) CHK(batch_dual_xtv<T>(c, X, ldx, N, K, Z, M, B0d, blocks));
        if (!back) return PLS_HIP_OK;
        double *Br = B ? B + r0 * KM : (double *)c->rsB.p;
        CHK(batch_dual_xtv<T>(c, X, ldx, N, K, Z + lead * NM, (int)(nr * M), Br, blocks));
        if (summary) CHK(resample_accumulate(c, Br, B0d, KM, nr, s1, s2));
        return PLS_HIP_OK;
    };
    CHK(r.run(c, N, M, A, plsk::RS_YIN, "round of replicates", init, step, after));
    if (summary) CHK(resample_finish(c, B0d, s1, s2, KM, nrep, Bmean, Bm2));
    return PLS_HIP_OK;
}

// The general route: per replicate diag(s) X and diag(s) Y in fp64 work copies, one KERNEL_TYPE1 fit of them under the handle's
// plan (T discarded after tt), the accumulation as above.  PLS_HIP_ERR_ALLOC: a work copy does not fit.
template <typename T>
int fit_resampled_refit(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M, int A, const double *Wt,
                        i64 ldw, i64 nrep, double *Q, double *tt, double *B, double *B0, double *Bmean, double *Bm2) {
    const i64 KA = (i64)K * A, MA = (i64)M * A, KM = (i64)K * M, ldn = N + (N & 1);  // even ld keeps 16-B columns
    const bool summary = Bmean || Bm2, need0 = B0 || summary;
    if ((N * ((i64)K + M) + plsk::WG - 1) / plsk::WG > ((i64)1 << 31) - 1)
        return fail(c, PLS_HIP_ERR_UNSUPPORTED, "fit_resampled: N (K + M) < 2^39 on the general route");
    CHK(ensure(c, c->rsX, (size_t)(ldn * K * 8)));
    CHK(ensure(c, c->rsY, (size_t)(ldn * M * 8)));
    CHK(ensure(c, c->rsw, (size_t)((3 * KA + MA + ldn * A + KM) * 8)));
    double *Xs = (double *)c->rsX.p, *Ys = (double *)c->rsY.p;
    double *Wf = (double *)c->rsw.p, *Pf = Wf + KA, *Rf = Pf + KA, *Qf = Rf + KA, *Tf = Qf + MA, *Bf = Tf + ldn * A;
    double *s1 = nullptr, *s2 = nullptr, *B0d = nullptr;
    if (need0) CHK(resample_accumulators(c, KM, summary, B0, s1, s2, B0d));
    const double *saved_xx = c->pre_xx, *saved_xy = c->pre_xy;  // (products of an upload belong to the unscaled rows)
    c->pre_xx = c->pre_xy = nullptr;
    // An ALGO_DUAL handle that comes here refits under KERNEL: this route is the cross-check of the sample-space one and must
    // not share its algebra -- the Gram matrix of the scaled rows squares the condition number exactly as X X^T does.
    const i64 saved_algo = c->opt_algo;
    if (saved_algo == PLS_HIP_ALGO_DUAL) c->opt_algo = PLS_HIP_ALGO_KERNEL;
    int rc = PLS_HIP_OK;
    Range r_call("pls_hip_fit_resampled (refits)");
    for (i64 b = need0 ? -1 : 0; b < nrep && rc == PLS_HIP_OK; ++b) {
        hipLaunchKernelGGL((plsk::row_scale_kernel<T>), dim3((unsigned)((N * ((i64)K + M) + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                           c->stream, X, ldx, Y, ldy, b < 0 ? (const double *)nullptr : Wt + b * ldw, N, (i64)K, (i64)M, ldn, Xs, Ys);
        if (hipGetLastError() != hipSuccess) { rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_resampled: launch failed"); break; }
        double *Bb = b < 0 ? B0d : B ? B + b * KM : summary ? Bf : nullptr;
        rc = fit_device<double>(c, Xs, ldn, Ys, ldn, N, K, M, A, PLS_HIP_KERNEL_TYPE1, Wf, Pf, Qf, Rf, Tf, ldn, Bb);
        if (rc != PLS_HIP_OK || b < 0) continue;
        if (Q && hipMemcpyAsync(Q + b * MA, Qf, (size_t)MA * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
            rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_resampled: copy of a replicate's results failed");
            break;
        }
        if (tt) {  // t~_a^T t~_a from the fit's scores
            hipLaunchKernelGGL((plsk::batch_ssy_kernel<double>), dim3((unsigned)A), dim3(plsk::WG), 0, c->stream, (const double *)Tf, ldn,
                               N, tt + b * A);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, PLS_HIP_ERR_DEVICE, "fit_resampled: launch failed"); break; }
        }
        if (summary) rc = resample_accumulate(c, Bb, B0d, KM, 1, s1, s2);
    }
    c->pre_xx = saved_xx;
    c->pre_xy = saved_xy;
    c->opt_algo = saved_algo;
    if (rc != PLS_HIP_OK) return rc;
    if (summary) CHK(resample_finish(c, B0d, s1, s2, KM, nrep, Bmean, Bm2));
    return PLS_HIP_OK;
}

// pls_hip_fit_resampled behind its argument checks
int fit_resampled_impl(pls_hip_context *h, const void *X, i64 ldx, const void *Y, i64 ldy, i64 N, i64 K, i64 M, i64 A,
                       const double *Wt, i64 ldw, i64 nrep, int dtype, int mem, double *Q, double *tt, double *B, double *B0,
                       double *Bmean, double *Bm2) {
    const size_t es = esize(dtype);
    const i64 KM = K * M;
    const void *dX = X, *dY = Y;
    const double *dW = Wt;
    i64 dldx = ldx, dldy = ldy, dldw = ldw;
    double *dQ = Q, *dtt = tt, *dB = B, *dB0 = B0, *dBmean = Bmean, *dBm2 = Bm2;
    const i64 ldn = ld_quad(N);
    const size_t summary = (size_t)3 * KM * 8;  // rsoS = [B0 | Bmean | Bm2]
    HostCall hc(h, mem);
    CHK(hc.out(dQ, Q, h->boQ, M * A, nrep));
    CHK(hc.out(dtt, tt, h->bott, A, nrep));
    CHK(hc.out(dB, B, h->boB, KM, nrep));
    CHK(hc.out(dB0, B0, h->rsoS, KM, 1, 8, summary, 0));
    CHK(hc.out(dBmean, Bmean, h->rsoS, KM, 1, 8, summary, (size_t)KM * 8));
    CHK(hc.out(dBm2, Bm2, h->rsoS, KM, 1, 8, summary, (size_t)2 * KM * 8));
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(hc.in(dW, dldw, Wt, ldw, h->rsW, N, nrep, 8, ld_exact(N)));
    int rc = PLS_HIP_ERR_ALLOC;
    if (resample_dual_covers(h, N, M)) {  // the sample-space plan, an explicit opt-in: every replicate from one X X^T
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return fit_resampled_dual<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, (int)N, K, (int)M, (int)A, dW, dldw, nrep, dQ, dtt,
                                         dB, dB0, dBmean, dBm2);
        });
        if (rc == PLS_HIP_ERR_ALLOC) h->err.clear();  // its workspace does not fit: the general route
    }
    if (rc == PLS_HIP_ERR_ALLOC)
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return fit_resampled_refit<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, dW, dldw, nrep, dQ, dtt,
                                          dB, dB0, dBmean, dBm2);
        });
    if (rc != PLS_HIP_OK) return rc;
    return hc.finish(true);
}

}  // namespace
