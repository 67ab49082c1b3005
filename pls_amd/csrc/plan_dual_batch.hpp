// plan_dual_batch.hpp -- fit_batch_dual: pls_hip_fit_batch under PLS_HIP_ALGO_DUAL, every problem from one G = X X^T.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// One sweep over X for Q, tt and ssy whatever A and the number of problems are.  The problems run in rounds (DualRounds, dual_round.hpp); per component a
// round costs one product Z = G [Y_a(0) | Y_a(1) | ...] and one launch of dual_batch_step_kernel, a workgroup per problem.
// R and B, where asked for, are one wide product each per round, X^T [S(0) | S(1) | ...] and X^T [D(0) | D(1) | ...], written
// straight into the caller's arrays (dual_batch_kernels.hpp has the algebra).
#pragma once

namespace {

// the calls this route takes; every other call routes as without it
bool batch_dual_covers(const pls_hip_context *c, i64 N, i64 M) { return N >= 1 && dual_rounds_cover(c, N, M) && !c->env.batch_refit; }

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
    const i64 NM = (i64)N * M, NA = (i64)N * A, es = (i64)sizeof(T);
    Range r_batch("pls_hip_fit_batch (sample space)");
    DualRounds r;
    // (the only pass over X unless R or B is asked for.)  N * C of the products (C = problems M, problems A) stays below 2^30
    // values; no round at all beyond A = 2^20 (A x A doubles per problem)
    DualRounds::Sizing sz;
    sz.items = nprob;
    sz.value_cap = A > ((i64)1 << 20) ? 0 : ((i64)1 << 30) / ((i64)N * std::max(M, A));
    sz.env_cap = c->env.dualbatch_round;
    sz.refusal = "fit_batch: the workspace of one problem does not fit";
    CHK(r.open<T>(c, X, ldx, N, (int)K, M, plsk::batch_dual_layout(N, M, A), sz, c->dbat));
    double *Ya = r.field(plsk::DUAL_YA), *Z = r.field(plsk::DUAL_Z), *T64 = r.field(plsk::BAT_T), *U = r.field(plsk::BAT_U);
    double *C = r.field(plsk::BAT_C), *Qw = r.field(plsk::BAT_Q), *ttw = r.field(plsk::BAT_TT), *scr = r.field(plsk::BAT_SCR);
    // the caller's arrays from the round's first problem on where they were asked for, workspace otherwise
    auto Qr = [&](i64 b0) { return Q ? Q + b0 * M * A : Qw; };
    auto init = [&](i64 b0, i64 nb) -> int {
        const int Cy = (int)(nb * M);
        Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * Cy * (es + 8));
        hipLaunchKernelGGL((plsk::dual_batch_init_kernel<T>), dim3((unsigned)Cy), dim3(plsk::WG), 0, c->stream, Ys + b0 * M * ldy, ldy, N,
                           Ya, ssy ? ssy + b0 * M : nullptr);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto step = [&](i64 b0, i64 nb, int a) -> int {
        Scope s(c, PLS_HIP_FAM_SMALL, nb * (i64)N * (3 * M + a + 4) * 8);
        hipLaunchKernelGGL(plsk::dual_batch_step_kernel, dim3((unsigned)nb), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya,
                           T64, U, Qr(b0), C, tt ? tt + b0 * A : ttw, scr, N, M, A, a, (int)c->opt_power_iters);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    };
    auto after = [&](i64 b0, i64 nb) -> int {
        if (!R && !B) return PLS_HIP_OK;
        {
            Scope s(c, PLS_HIP_FAM_SMALL, nb * (2 * NA + (i64)A * A + (i64)M * A + (B ? NM : 0)) * 8);
            hipLaunchKernelGGL(plsk::dual_batch_sd_kernel, dim3((unsigned)nb), dim3(plsk::WG), 0, c->stream, U, (const double *)C,
                               (const double *)Qr(b0), N, M, A, B ? Z : (double *)nullptr);
            LAUNCH_CHECK(c);
        }
        Range r_b("X^T [S D]");
        if (R) CHK(batch_dual_xtv<T>(c, X, ldx, N, K, U, (int)(nb * A), R + b0 * K * A));
        if (B) CHK(batch_dual_xtv<T>(c, X, ldx, N, K, Z, (int)(nb * M), B + b0 * K * M));
        return PLS_HIP_OK;
    };
    return r.run(c, N, M, A, plsk::DUAL_YA, "round of problems", init, step, after);
}

}  // namespace
