// plan_dual_cvbatch.hpp -- pls_hip_cv_press_batch: the cross-validation folds of many response sets on one X, PRESS and ssy of
// every problem reduced on the device (the Q^2 permutation test).
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// Sample-space route (cv_press_batch_dual, under PLS_HIP_ALGO_DUAL): G = X X^T once -- the only pass over X whatever A, nprob
// and num_folds are -- then the nprob num_folds (problem, fold) pairs in rounds; per component a round costs one product
// Z = G [Y_a of every item] and one launch of dual_cvb_step_kernel, a workgroup per item; a reduce kernel after the round
// (dual_cvbatch_kernels.hpp has the algebra).  Nothing nobs x A-sized per problem exists unless E is asked for.
// General route (cv_press_batch_refit): per problem pls_hip_cv_folds on (X, Y_b), the PRESS kernels of pls_hip_validation on its
// E, a small kernel for ssy.  The library's own cross-check (PLS_HIP_CVBATCH_REFIT=1).
#pragma once

namespace {

// the calls the sample-space route takes: those of cv_dual_covers; every other call takes the general route
bool cvbatch_dual_covers(const pls_hip_context *c, i64 N, i64 M) { return cv_dual_covers(c, N, M) && !c->env.cvbatch_refit; }

// doubles of one item's state: Y_a and Z (N x M), the scores (N x A), tt (A), g and c (N + A), the predictions, the held-out
// responses and the residuals by test position (ts x M each), the partial PRESS (M x A) and ssy (M)
i64 cvbatch_item_doubles(i64 N, i64 M, i64 A, i64 ts) { return 2 * N * M + N * A + A + N + A + 3 * ts * M + M * A + M; }

// X, Ys device pointers, test_idx host memory; any of PRESS, ssy, E (device memory) may be null.  PLS_HIP_ERR_ALLOC: the
// workspace does not fit.
template <typename T>
int cv_press_batch_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, int N, int K, int M, int A, i64 nprob,
                        const int64_t *test_idx, int ts, i64 num_folds, double *PRESS, double *ssy, double *E) {
    const i64 nobs = num_folds * ts, NN = (i64)N * N, NM = (i64)N * M, NA = (i64)N * A, MA = (i64)M * A, tsM = (i64)ts * M;
    const i64 items = nprob * num_folds, es = (i64)sizeof(T);
    if (A > ((i64)1 << 20)) return fail(c, PLS_HIP_ERR_ALLOC, "cv_press_batch: the workspace of one item does not fit");
    // G and the partial blocks of its sweep first, then the folds' tables: the round is sized by what they leave
    CHK(ensure(c, c->dG, (size_t)NN * 8));
    CHK(ensure(c, c->cvbidx, (size_t)nobs * 8));
    CHK(ensure(c, c->cvbpos, (size_t)num_folds * N * 4));
    Range r_call("pls_hip_cv_press_batch (sample space)");
    CHK(dual_gram<T>(c, X, ldx, N, K));  // the only pass over X
    // N * C of the product stays below 2^30 values
    const i64 nround = round_size(cvbatch_item_doubles(N, M, A, ts) * 8, ((i64)1 << 30) / NM, c->env.dualcvb_round, items);
    if (nround < 1) return fail(c, PLS_HIP_ERR_ALLOC, "cv_press_batch: the workspace of one item does not fit");
    CHK(ensure(c, c->dcvb, (size_t)(nround * cvbatch_item_doubles(N, M, A, ts) * 8)));
    const double *G = (const double *)c->dG.p;
    const i64 *idx = (const i64 *)c->cvbidx.p;
    int *pos = (int *)c->cvbpos.p;
    double *Ya = (double *)c->dcvb.p, *Z = Ya + nround * NM, *T64 = Z + nround * NM, *ttv = T64 + nround * NA;
    double *scr = ttv + nround * A, *pred = scr + nround * (N + A), *yte = pred + nround * tsM, *escr = yte + nround * tsM;
    double *pressp = escr + nround * tsM, *ssyp = pressp + nround * MA;
    // one product kernel for the whole call, as the folds choose theirs (plan_dual_cv.hpp)
    const bool gy = nround * M <= 32;
    const int nblk = (int)((MA + M + plsk::WG - 1) / plsk::WG);
    HIPCHK(c, hipMemcpyAsync(c->cvbidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, PLS_HIP_FAM_SMALL, nobs * 8 + num_folds * N * 4);
        hipLaunchKernelGGL(plsk::dual_cvb_pos_kernel, dim3((unsigned)num_folds), dim3(plsk::WG), 0, c->stream, idx, N, ts, pos);
        LAUNCH_CHECK(c);
    }
    for (i64 i0 = 0; i0 < items; i0 += nround) {
        Range r_round("round of items", (int)(i0 / nround));
        const i64 nb = std::min(nround, items - i0);
        const int C = (int)(nb * M);
        {
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (NM * (es + 8) + (i64)N * 4 + tsM * (es + 16)));
            hipLaunchKernelGGL((plsk::dual_cvb_init_kernel<T>), dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, Ys, ldy, idx,
                               (const int *)pos, N, M, ts, num_folds, i0, Ya, pred, yte, ssyp);
            LAUNCH_CHECK(c);
        }
        for (int a = 0; a < A; ++a) {
            if (gy) CHK(launch_dual_gy(c, G, Ya, N, C, Z));
            else CHK(launch_sym_product(c, G, N, Ya, (i64)N, C, Z, (i64)N));
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
            hipLaunchKernelGGL(plsk::dual_cvb_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                               T64, ttv, scr, (const int *)pos, pred, (const double *)yte, escr, pressp, E, N, M, A, a, ts, i0,
                               num_folds, nobs, (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
        if (!PRESS && !ssy) continue;
        const i64 np = (i0 + nb - 1) / num_folds - i0 / num_folds + 1;  // problems with an item in the round
        Scope s(c, PLS_HIP_FAM_SMALL, (nb + 2 * np) * (MA + M) * 8);
        hipLaunchKernelGGL(plsk::dual_cvb_reduce_kernel, dim3((unsigned)(np * nblk)), dim3(plsk::WG), 0, c->stream, (const double *)pressp,
                           (const double *)ssyp, i0, nb, num_folds, (int)MA, M, nblk, PRESS, ssy);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

// The general route: per problem the existing cross-validation (whatever route pls_hip_cv_folds takes on this handle and
// shape) into the caller's slice of E or into a workspace, the PRESS kernels of pls_hip_validation on it; ssy of every
// problem in one launch.  Statuses of pls_hip_cv_folds are passed on.
template <typename T>
int cv_press_batch_refit(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, i64 N, i64 K, i64 M, i64 A, i64 nprob,
                         const int64_t *test_idx, i64 ts, i64 num_folds, int dtype, double *PRESS, double *ssy, double *E) {
    const i64 nobs = num_folds * ts, MA = M * A;
    if (PRESS && (nobs > ((i64)1 << 31) - 1 || M * A > (1 << 24) || ((nobs + plsk::VAL_CH - 1) / plsk::VAL_CH) * M * A > ((i64)1 << 31) - 1))
        return fail(c, PLS_HIP_ERR_UNSUPPORTED, "cv_press_batch: nobs < 2^31, M A <= 2^24, M A ceil(nobs / 4096) < 2^31 on the general route");
    Range r_call("pls_hip_cv_press_batch (per problem)");
    if (ssy) {
        CHK(ensure(c, c->cvbidx, (size_t)nobs * 8));
        HIPCHK(c, hipMemcpyAsync(c->cvbidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, c->stream));
        Scope s(c, PLS_HIP_FAM_SMALL, nprob * M * nobs * (i64)sizeof(T));
        hipLaunchKernelGGL((plsk::cvb_ssy_kernel<T>), dim3((unsigned)(nprob * M)), dim3(plsk::WG), 0, c->stream, Ys, ldy,
                           (const i64 *)c->cvbidx.p, N, nobs, ssy);
        LAUNCH_CHECK(c);
    }
    if (!PRESS && !E) {
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the index list is the caller's host memory)
        return PLS_HIP_OK;
    }
    if (!E) CHK(ensure(c, c->cve, (size_t)(M * nobs * A * 8)));
    for (i64 b = 0; b < nprob; ++b) {
        double *Eb = E ? E + b * M * nobs * A : (double *)c->cve.p;
        CHK(pls_hip_cv_folds(c, X, ldx, Ys + b * M * ldy, ldy, N, K, M, A, test_idx, ts, num_folds, dtype, PLS_HIP_MEM_DEVICE, Eb));
        if (PRESS) CHK(validation_impl(c, Eb, nobs, (int)A, (int)M, PLS_HIP_MEM_DEVICE, PRESS + b * MA, nullptr, nullptr, nullptr));
    }
    return PLS_HIP_OK;
}

// pls_hip_cv_press_batch behind its argument checks
int cv_press_batch_impl(pls_hip_context *h, const void *X, i64 ldx, const void *Ys, i64 ldy, i64 N, i64 K, i64 M, i64 A, i64 nprob,
                        const int64_t *test_idx, i64 ts, i64 num_folds, int dtype, int mem, double *PRESS, double *ssy, double *E) {
    const size_t es = esize(dtype);
    const i64 nobs = num_folds * ts, MA = M * A, C = nprob * M, ne = M * nobs * A;
    const void *dX = X, *dY = Ys;
    i64 dldx = ldx, dldy = ldy;
    double *dP = PRESS, *dS = ssy, *dE = E;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + ((-N) & 3);  // 16-byte columns for either type
        CHK(ensure(h, h->hX, (size_t)ldn * K * es));
        CHK(ensure(h, h->bY, (size_t)ldn * C * es));
        if (PRESS || ssy) CHK(ensure(h, h->cvbo, (size_t)(nprob * (MA + M) * 8)));
        if (E) CHK(ensure(h, h->cvboE, (size_t)(nprob * ne * 8)));
        CHK(h2d(h, h->hX.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->bY.p, ldn, Ys, ldy, N, C, es));
        dX = h->hX.p; dY = h->bY.p;
        dldx = dldy = ldn;
        dP = PRESS ? (double *)h->cvbo.p : nullptr;
        dS = ssy ? (double *)h->cvbo.p + nprob * MA : nullptr;
        dE = E ? (double *)h->cvboE.p : nullptr;
    }
    int rc = PLS_HIP_ERR_ALLOC;
    if (cvbatch_dual_covers(h, N, M)) {  // the sample-space plan, an explicit opt-in: every problem and fold from one X X^T
        if (dtype == PLS_HIP_F64)
            rc = cv_press_batch_dual<double>(h, (const double *)dX, dldx, (const double *)dY, dldy, (int)N, (int)K, (int)M, (int)A, nprob,
                                             test_idx, (int)ts, num_folds, dP, dS, dE);
        else
            rc = cv_press_batch_dual<float>(h, (const float *)dX, dldx, (const float *)dY, dldy, (int)N, (int)K, (int)M, (int)A, nprob,
                                            test_idx, (int)ts, num_folds, dP, dS, dE);
        if (rc == PLS_HIP_ERR_ALLOC) h->err.clear();  // its workspace does not fit: the general route
    }
    if (rc == PLS_HIP_ERR_ALLOC) {
        if (dtype == PLS_HIP_F64)
            rc = cv_press_batch_refit<double>(h, (const double *)dX, dldx, (const double *)dY, dldy, N, K, M, A, nprob, test_idx, ts,
                                              num_folds, dtype, dP, dS, dE);
        else
            rc = cv_press_batch_refit<float>(h, (const float *)dX, dldx, (const float *)dY, dldy, N, K, M, A, nprob, test_idx, ts,
                                             num_folds, dtype, dP, dS, dE);
    }
    if (rc != PLS_HIP_OK) return rc;
    if (mem == PLS_HIP_MEM_HOST) {
        if (PRESS) CHK(d2h(h, PRESS, MA, dP, MA, MA, nprob, 8));
        if (ssy) CHK(d2h(h, ssy, M, dS, M, M, nprob, 8));
        if (E) CHK(d2h(h, E, nobs, dE, nobs, nobs, nprob * MA, 8));
    }
    // the index list is host memory of the caller, and the call returns after the work has completed
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PLS_HIP_OK;
}

}  // namespace
