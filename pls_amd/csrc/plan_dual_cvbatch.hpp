// plan_dual_cvbatch.hpp -- pls_hip_cv_press_batch: the cross-validation folds of many response sets on one X, PRESS and ssy of
// every problem reduced on the device (the Q^2 permutation test).
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// Sample-space route (cv_press_batch_dual, under PLS_HIP_ALGO_DUAL): G = X X^T once -- the only pass over X whatever A, nprob
// and num_folds are -- then the nprob num_folds (problem, fold) pairs in rounds (DualRounds, dual_round.hpp); per component a round costs one product
// Z = G [Y_a of every item] and one launch of dual_cvb_step_kernel, a workgroup per item; a reduce kernel after the round
// (dual_cvbatch_kernels.hpp has the algebra).  Nothing nobs x A-sized per problem exists unless E is asked for.
// General route (cv_press_batch_refit): per problem pls_hip_cv_folds on (X, Y_b), the PRESS kernels of pls_hip_validation on its
// E, a small kernel for ssy.  The library's own cross-check (PLS_HIP_CVBATCH_REFIT=1).
#pragma once

namespace {

// the calls the sample-space route takes: those of cv_dual_covers; every other call takes the general route
bool cvbatch_dual_covers(const pls_hip_context *c, i64 N, i64 M) { return cv_dual_covers(c, N, M) && !c->env.cvbatch_refit; }

// X, Ys device pointers, test_idx host memory; any of PRESS, ssy, E (device memory) may be null.  PLS_HIP_ERR_ALLOC: the
// workspace does not fit.
template <typename T>
int cv_press_batch_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, int N, int K, int M, int A, i64 nprob,
                        const int64_t *test_idx, int ts, i64 num_folds, double *PRESS, double *ssy, double *E) {
    const i64 nobs = num_folds * ts, NM = (i64)N * M, MA = (i64)M * A, tsM = (i64)ts * M;
    const i64 items = nprob * num_folds, es = (i64)sizeof(T);
    if (A > ((i64)1 << 20)) return fail(c, PLS_HIP_ERR_ALLOC, "cv_press_batch: the workspace of one item does not fit");
    // the folds' tables before G: the round is sized by what is left
    CHK(ensure(c, c->cvbidx, (size_t)nobs * 8));
    CHK(ensure(c, c->cvbpos, (size_t)num_folds * N * 4));
    Range r_call("pls_hip_cv_press_batch (sample space)");
    DualRounds r;
    // (the only pass over X; N * C of the product stays below 2^30 values)
    DualRounds::Sizing sz;
    sz.items = items;
    sz.value_cap = ((i64)1 << 30) / NM;
    sz.env_cap = c->env.dualcvb_round;
    sz.refusal = "cv_press_batch: the workspace of one item does not fit";
    CHK(r.open<T>(c, X, ldx, N, K, M, plsk::cvbatch_layout(N, M, A, ts), sz, c->dcvb));
    const i64 *idx = (const i64 *)c->cvbidx.p;
    int *pos = (int *)c->cvbpos.p;
    double *Ya = r.field(plsk::DUAL_YA), *Z = r.field(plsk::DUAL_Z), *T64 = r.field(plsk::CV_T), *ttv = r.field(plsk::CV_TT);
    double *scr = r.field(plsk::CV_SCR), *pred = r.field(plsk::CV_PRED), *yte = r.field(plsk::CVB_YTE), *escr = r.field(plsk::CVB_ESCR);
    double *pressp = r.field(plsk::CVB_PRESS), *ssyp = r.field(plsk::CVB_SSY);
    const int nblk = (int)((MA + M + plsk::WG - 1) / plsk::WG);
    HIPCHK(c, hipMemcpyAsync(c->cvbidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, PLS_HIP_FAM_SMALL, nobs * 8 + num_folds * N * 4);
        hipLaunchKernelGGL(plsk::dual_cvb_pos_kernel, dim3((unsigned)num_folds), dim3(plsk::WG), 0, c->stream, idx, N, ts, pos);
        LAUNCH_CHECK(c);
    }
    auto init = [&](i64 i0, i64 nb) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (NM * (es + 8) + (i64)N * 4 + tsM * (es + 16)));
        hipLaunchKernelGGL((plsk::dual_cvb_init_kernel<T>), dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, Ys, ldy, idx,
                           (const int *)pos, N, M, ts, num_folds, i0, Ya, pred, yte, ssyp);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto step = [&](i64 i0, i64 nb, int a) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
        hipLaunchKernelGGL(plsk::dual_cvb_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                           T64, ttv, scr, (const int *)pos, pred, (const double *)yte, escr, pressp, E, N, M, A, a, ts, i0, num_folds,
                           nobs, (int)c->opt_power_iters);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto after = [&](i64 i0, i64 nb) -> int {
        if (!PRESS && !ssy) return PLS_HIP_OK;
        const i64 np = (i0 + nb - 1) / num_folds - i0 / num_folds + 1;  // problems with an item in the round
        Scope s(c, PLS_HIP_FAM_SMALL, (nb + 2 * np) * (MA + M) * 8);
        hipLaunchKernelGGL(plsk::dual_cvb_reduce_kernel, dim3((unsigned)(np * nblk)), dim3(plsk::WG), 0, c->stream, (const double *)pressp,
                           (const double *)ssyp, i0, nb, num_folds, (int)MA, M, nblk, PRESS, ssy);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    return r.run(c, N, M, A, plsk::DUAL_YA, "round of items", init, step, after);
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
    const i64 nobs = num_folds * ts, MA = M * A, C = nprob * M;
    const void *dX = X, *dY = Ys;
    i64 dldx = ldx, dldy = ldy;
    double *dP = PRESS, *dS = ssy, *dE = E;
    const i64 ldn = ld_quad(N);
    const size_t sums = (size_t)nprob * (MA + M) * 8;  // cvbo = [PRESS | ssy]
    HostCall hc(h, mem);
    CHK(hc.out(dP, PRESS, h->cvbo, MA, nprob, 8, sums, 0));
    CHK(hc.out(dS, ssy, h->cvbo, M, nprob, 8, sums, (size_t)nprob * MA * 8));
    CHK(hc.out(dE, E, h->cvboE, nobs, nprob * MA));
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Ys, ldy, h->bY, N, C, es, ldn));
    int rc = PLS_HIP_ERR_ALLOC;
    if (cvbatch_dual_covers(h, N, M)) {  // the sample-space plan, an explicit opt-in: every problem and fold from one X X^T
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_press_batch_dual<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, (int)N, (int)K, (int)M, (int)A, nprob, test_idx,
                                          (int)ts, num_folds, dP, dS, dE);
        });
        if (rc == PLS_HIP_ERR_ALLOC) h->err.clear();  // its workspace does not fit: the general route
    }
    if (rc == PLS_HIP_ERR_ALLOC)
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_press_batch_refit<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, K, M, A, nprob, test_idx, ts, num_folds, dtype,
                                           dP, dS, dE);
        });
    if (rc != PLS_HIP_OK) return rc;
    // the index list is host memory of the caller, and the call returns after the work has completed, whatever `mem` is
    return hc.finish(false, true);
}

}  // namespace
