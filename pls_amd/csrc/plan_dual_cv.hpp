// plan_dual_cv.hpp -- cv_folds_dual: pls_hip_cv_folds under PLS_HIP_ALGO_DUAL, every fold from one G = X X^T.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// One sweep over X whatever A and the number of folds are.  The folds run in rounds; per component a round costs one product
// Z = G [Y_a(0) | Y_a(1) | ...] (N x N by N x (folds M)) and one launch of dual_cv_step_kernel, a workgroup per fold
// (dual_cv_kernels.hpp has the algebra).  Nothing K-sized exists after G.
#pragma once

namespace {

// the calls this route takes; every other call routes as without it
bool cv_dual_covers(const pls_hip_context *c, i64 N, i64 M) {
    return c->opt_algo == PLS_HIP_ALGO_DUAL && !c->reducer && c->nranks == 1 && N <= plsk::DUAL_NMAX && M <= plsk::DUAL_MMAX &&
           !c->env.cv_refit;
}

// bytes of one fold's state: Y_a and Z (N x M), the scores (N x A), tt (A), g and c (N + A), the predictions (ts x M), pos (N)
i64 cv_dual_fold_bytes(i64 N, i64 M, i64 A, i64 ts) { return (2 * N * M + N * A + 2 * A + N + ts * M) * 8 + N * 4; }

// folds per round: as many as 4 GB and half of the free device memory hold (0: not even one)
i64 cv_dual_round_size(pls_hip_context *c, i64 N, i64 M, i64 A, i64 ts, i64 num_folds) {
    // N * C of the product stays below 2^31 values
    return round_size(cv_dual_fold_bytes(N, M, A, ts), ((i64)1 << 30) / (N * M), c->env.dualcv_round, num_folds);
}

// X, Y device pointers, test_idx host memory, E device memory.  PLS_HIP_ERR_ALLOC: the workspace does not fit.
template <typename T>
int cv_folds_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, int N, int K, int M, int A, const int64_t *test_idx,
                  int ts, i64 num_folds, double *E) {
    const i64 nobs = num_folds * ts, NN = (i64)N * N, es = (i64)sizeof(T);
    // G and the partial blocks of its sweep first: the round is sized by what they leave
    CHK(ensure(c, c->dG, (size_t)NN * 8));
    CHK(ensure(c, c->dY, (size_t)N * M * 8));
    CHK(ensure(c, c->cvidx, (size_t)nobs * 8));
    Range r_cv("pls_hip_cv_folds (sample space)");
    CHK(dual_gram<T>(c, X, ldx, N, K));  // the only pass over X
    const i64 nround = cv_dual_round_size(c, N, M, A, ts, num_folds);
    if (nround < 1) return fail(c, PLS_HIP_ERR_ALLOC, "cv_folds: the workspace of one fold does not fit");
    CHK(ensure(c, c->dcv, (size_t)(nround * cv_dual_fold_bytes(N, M, A, ts))));
    const double *G = (const double *)c->dG.p;
    double *Y64 = (double *)c->dY.p;
    double *Ya = (double *)c->dcv.p, *Z = Ya + nround * M * N, *T64 = Z + nround * M * N, *ttv = T64 + nround * N * A;
    double *scr = ttv + nround * A, *pred = scr + nround * (N + A);
    int *pos = (int *)(pred + nround * ts * M);
    // one product kernel for the whole call: the single-wave rows of dual_gy_kernel up to 32 columns per round (the 128-wide
    // tile of the matrix-core kernel would be mostly padding), xtg_kernel with X := G beyond (G is symmetric)
    const bool gy = nround * M <= 32;
    HIPCHK(c, hipMemcpyAsync(c->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * M * (es + 8));
        hipLaunchKernelGGL((plsk::dual_convert_kernel<T, double>), dim3((unsigned)(((i64)N * M + 255) / 256)), dim3(256), 0, c->stream, Y,
                           ldy, Y64, (i64)N, N, M);
        LAUNCH_CHECK(c);
    }
    for (i64 f0 = 0; f0 < num_folds; f0 += nround) {
        Range r_round("round of folds", (int)(f0 / nround));
        const i64 nb = std::min(nround, num_folds - f0);
        const int C = (int)(nb * M);
        {
            Scope s(c, PLS_HIP_FAM_SMALL, nb * ((i64)N * (2 * M + 1) + (i64)ts * (M + 1)) * 8);
            hipLaunchKernelGGL(plsk::dual_cv_init_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const double *)Y64,
                               (const i64 *)c->cvidx.p + f0 * ts, N, M, ts, Ya, pos, pred);
            LAUNCH_CHECK(c);
        }
        for (int a = 0; a < A; ++a) {
            if (gy) CHK(launch_dual_gy(c, G, Ya, N, C, Z));
            else CHK(launch_sym_product(c, G, N, Ya, (i64)N, C, Z, (i64)N));
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
            hipLaunchKernelGGL(plsk::dual_cv_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                               T64, ttv, scr, (const int *)pos, pred, (const double *)Y64, E, N, M, A, a, ts, f0, nobs,
                               (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
    }
    return PLS_HIP_OK;
}

}  // namespace
