// plan_dual_batch.hpp -- fit_batch_dual: pls_hip_fit_batch under PLS_HIP_ALGO_DUAL, every problem from one G = X X^T.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// One sweep over X for Q, tt and ssy whatever A and the number of problems are.  The problems run in rounds; per component a
// round costs one product Z = G [Y_a(0) | Y_a(1) | ...] and one launch of dual_batch_step_kernel, a workgroup per problem.
// R and B, where asked for, are one wide product each per round, X^T [S(0) | S(1) | ...] and X^T [D(0) | D(1) | ...], written
// straight into the caller's arrays (dual_batch_kernels.hpp has the algebra).
#pragma once

namespace {

// the calls this route takes; every other call routes as without it
bool batch_dual_covers(const pls_hip_context *c, i64 N, i64 M) {
    return c->opt_algo == PLS_HIP_ALGO_DUAL && !c->reducer && c->nranks == 1 && N >= 1 && N <= plsk::DUAL_NMAX &&
           M <= plsk::DUAL_MMAX && !c->env.batch_refit;
}

// doubles of one problem's state: Y_a and Z (N x M; D reuses Z), T and U (N x A; S overwrites U), C (A x A), Q (M x A), tt (A),
// g and c (N + A)
i64 batch_dual_problem_doubles(i64 N, i64 M, i64 A) { return 2 * N * M + 2 * N * A + A * A + M * A + A + N + A; }

// problems per round: as many as 4 GB and half of the free device memory hold (0: not even one)
i64 batch_dual_round_size(pls_hip_context *c, i64 N, i64 M, i64 A, i64 nprob) {
    if (A > ((i64)1 << 20)) return 0;  // (A x A doubles per problem)
    // N * C of the products (C = problems M, problems A) stays below 2^30 values
    return round_size(batch_dual_problem_doubles(N, M, A) * 8, ((i64)1 << 30) / (N * std::max(M, A)), c->env.dualbatch_round, nprob);
}

// out (K x cols, ld K) = X^T V, V = N x cols (ld N): one launch of dual_xtv_kernel up to 64 columns; beyond, one launch of
// dual_xtvb_kernel (the default) or, under PLS_HIP_DUALBATCH_SWEEPS=1, one sweep of dual_xtv_kernel per 64 columns
// (tools/dual_batch_bench.py measures the two).  Every launch is a bracket of PLS_HIP_FAM_XTY.  `blocks`: dual_xtvb_kernel for
// fewer columns as well (a caller whose rounds differ in width and whose bits must not: plan_resample.hpp).
template <typename T>
int batch_dual_xtv(pls_hip_context *c, const T *X, i64 ldx, int N, i64 K, const double *V, int cols, double *out, bool blocks = false) {
    const i64 es = (i64)sizeof(T);
    if ((cols > plsk::XTV_NC || blocks) && !c->env.dualbatch_sweeps) {
        if (!plsk::raise_dynamic_lds((const void *)plsk::dual_xtvb_kernel<T>, (int)plsk::XTVB_LDS_BYTES))
            return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the back-projection could not be raised");
        const i64 nbk = (K + plsk::XTVB_TB - 1) / plsk::XTVB_TB;
        const int nbc = (cols + plsk::XTVB_TB - 1) / plsk::XTVB_TB;
        Scope s(c, PLS_HIP_FAM_XTY, (i64)N * K * es + ((i64)N + K) * cols * 8);
        hipLaunchKernelGGL((plsk::dual_xtvb_kernel<T>), dim3((unsigned)(nbk * nbc)), dim3(256), plsk::XTVB_LDS_BYTES, c->stream, X, ldx, N,
                           K, V, cols, nbc, out);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    }
    for (int c0 = 0; c0 < cols; c0 += plsk::XTV_NC) {
        const int nc = std::min(plsk::XTV_NC, cols - c0);
        CHK(launch_dual_xtv<T>(c, X, ldx, N, K, V, c0, nc, cols, out, (double *)nullptr));  // (A = cols: everything to `out`)
    }
    return PLS_HIP_OK;
}

// X, Ys device pointers; any of R, Q, tt, B, ssy (device memory) may be null.  PLS_HIP_ERR_ALLOC: the workspace does not fit.
template <typename T>
int fit_batch_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Ys, i64 ldy, int N, i64 K, int M, int A, i64 nprob, double *R,
                   double *Q, double *tt, double *B, double *ssy) {
    const i64 NN = (i64)N * N, NM = (i64)N * M, NA = (i64)N * A, es = (i64)sizeof(T);
    // G and the partial blocks of its sweep first: the round is sized by what they leave
    CHK(ensure(c, c->dG, (size_t)NN * 8));
    Range r_batch("pls_hip_fit_batch (sample space)");
    CHK(dual_gram<T>(c, X, ldx, N, (int)K));  // the only pass over X unless R or B is asked for
    const i64 nround = batch_dual_round_size(c, N, M, A, nprob);
    if (nround < 1) return fail(c, PLS_HIP_ERR_ALLOC, "fit_batch: the workspace of one problem does not fit");
    CHK(ensure(c, c->dbat, (size_t)(nround * batch_dual_problem_doubles(N, M, A) * 8)));
    const double *G = (const double *)c->dG.p;
    double *Ya = (double *)c->dbat.p, *Z = Ya + nround * NM, *T64 = Z + nround * NM, *U = T64 + nround * NA, *C = U + nround * NA;
    double *Qw = C + nround * A * A, *ttw = Qw + nround * M * A, *scr = ttw + nround * A;
    // one product kernel for the whole call, as the folds choose theirs (plan_dual_cv.hpp)
    const bool gy = nround * M <= 32;
    for (i64 b0 = 0; b0 < nprob; b0 += nround) {
        Range r_round("round of problems", (int)(b0 / nround));
        const i64 nb = std::min(nround, nprob - b0);
        const int Cy = (int)(nb * M);
        double *Qr = Q ? Q + b0 * M * A : Qw, *ttr = tt ? tt + b0 * A : ttw;
        {
            Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * Cy * (es + 8));
            hipLaunchKernelGGL((plsk::dual_batch_init_kernel<T>), dim3((unsigned)Cy), dim3(plsk::WG), 0, c->stream, Ys + b0 * M * ldy, ldy,
                               N, Ya, ssy ? ssy + b0 * M : nullptr);
            LAUNCH_CHECK(c);
        }
        for (int a = 0; a < A; ++a) {
            if (gy) CHK(launch_dual_gy(c, G, Ya, N, Cy, Z));
            else CHK(launch_sym_product(c, G, N, Ya, (i64)N, Cy, Z, (i64)N));
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
            hipLaunchKernelGGL(plsk::dual_batch_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z,
                               Ya, T64, U, Qr, C, ttr, scr, N, M, A, a, (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
        if (!R && !B) continue;
        {
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (2 * NA + (i64)A * A + (i64)M * A + (B ? NM : 0)) * 8);
            hipLaunchKernelGGL(plsk::dual_batch_sd_kernel, dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, U, (const double *)C,
                               (const double *)Qr, N, M, A, B ? Z : (double *)nullptr);
            LAUNCH_CHECK(c);
        }
        Range r_b("X^T [S D]");
        if (R) CHK(batch_dual_xtv<T>(c, X, ldx, N, K, U, (int)(nb * A), R + b0 * K * A));
        if (B) CHK(batch_dual_xtv<T>(c, X, ldx, N, K, Z, Cy, B + b0 * K * M));
    }
    return PLS_HIP_OK;
}

}  // namespace
