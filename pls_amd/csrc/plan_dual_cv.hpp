// plan_dual_cv.hpp -- cv_folds_dual: pls_hip_cv_folds under PLS_HIP_ALGO_DUAL, every fold from one G = X X^T.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// One sweep over X whatever A and the number of folds are.  The folds run in rounds (DualRounds, dual_round.hpp); per component a round costs one product
// Z = G [Y_a(0) | Y_a(1) | ...] (N x N by N x (folds M)) and one launch of dual_cv_step_kernel, a workgroup per fold
// (dual_cv_kernels.hpp has the algebra).  Nothing K-sized exists after G.
#pragma once

namespace {

// the calls this route takes; every other call routes as without it
bool cv_dual_covers(const pls_hip_context *c, i64 N, i64 M) { return dual_rounds_cover(c, N, M) && !c->env.cv_refit; }

// X, Y device pointers, test_idx host memory, E device memory.  PLS_HIP_ERR_ALLOC: the workspace does not fit.
template <typename T>
int cv_folds_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, int N, int K, int M, int A, const int64_t *test_idx,
                  int ts, i64 num_folds, double *E) {
    const i64 nobs = num_folds * ts, es = (i64)sizeof(T);
    // before G: the round is sized by what is left
    CHK(ensure(c, c->dY, (size_t)N * M * 8));
    CHK(ensure(c, c->cvidx, (size_t)nobs * 8));
    Range r_cv("pls_hip_cv_folds (sample space)");
    DualRounds r;
    // (the only pass over X; N * C of the product stays below 2^31 values)
    DualRounds::Sizing sz;
    sz.items = num_folds;
    sz.value_cap = ((i64)1 << 30) / ((i64)N * M);
    sz.env_cap = c->env.dualcv_round;
    sz.refusal = "cv_folds: the workspace of one fold does not fit";
    CHK(r.open<T>(c, X, ldx, N, K, M, plsk::cv_dual_layout(N, M, A, ts), sz, c->dcv));
    double *Y64 = (double *)c->dY.p;
    double *Ya = r.field(plsk::DUAL_YA), *Z = r.field(plsk::DUAL_Z), *T64 = r.field(plsk::CV_T), *ttv = r.field(plsk::CV_TT);
    double *scr = r.field(plsk::CV_SCR), *pred = r.field(plsk::CV_PRED);
    int *pos = r.int_field();
    HIPCHK(c, hipMemcpyAsync(c->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, c->stream));
    {
        Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * M * (es + 8));
        hipLaunchKernelGGL((plsk::dual_convert_kernel<T, double>), dim3((unsigned)(((i64)N * M + 255) / 256)), dim3(256), 0, c->stream, Y,
                           ldy, Y64, (i64)N, N, M);
        LAUNCH_CHECK(c);
    }
    auto init = [&](i64 f0, i64 nb) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * ((i64)N * (2 * M + 1) + (i64)ts * (M + 1)) * 8);
        hipLaunchKernelGGL(plsk::dual_cv_init_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const double *)Y64,
                           (const i64 *)c->cvidx.p + f0 * ts, N, M, ts, Ya, pos, pred);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto step = [&](i64 f0, i64 nb, int a) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
        hipLaunchKernelGGL(plsk::dual_cv_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                           T64, ttv, scr, (const int *)pos, pred, (const double *)Y64, E, N, M, A, a, ts, f0, nobs,
                           (int)c->opt_power_iters);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    return r.run(c, N, M, A, plsk::DUAL_YA, "round of folds", init, step, [](i64, i64) { return (int)PLS_HIP_OK; });
}

}  // namespace
