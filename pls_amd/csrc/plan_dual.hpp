// plan_dual.hpp -- fit_dual: the sample-space plan (PLS_HIP_ALGO_DUAL) of a KERNEL_TYPE1 fit, for short, wide X.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// Model::plsr (src/pls.cpp:390-437) with every K-sized quantity expressed through N-sized ones.  The scores are mutually
// orthogonal, so the deflated cross product is a projection, XY_a = X^T Y_a with Y_a = Y - T_a Q_a^T, and with G = X X^T
//     XY_a^T XY_a = Y_a^T G Y_a,   w_a = X^T u / nw with u = Y_a q^ and nw^2 = u^T G u,   t_a = X r_a = (G u - sum_j c_j t_j) / nw.
// Two sweeps over X whatever A is: G on the matrix cores, then [W | P] = X^T [U | T diag(1/tt)] (one sweep per 64 columns
// of [U | T]); the component loop between them touches N-sized data only.  R comes from the recurrence of :412-416 with
// p_j^T w_a = c_j / nw, the coefficients of the orthogonalisation (no product of K-long columns).
#pragma once

namespace {

// refused before anything is written (pls_hip_fit): the limits of the plan
inline const char *dual_refusal(const pls_hip_context *c, i64 N, i64 M) {
    if (c->reducer || c->nranks > 1) return "ALGO_DUAL needs every row of X on one handle: not on a row-sharded fit";
    if (N > plsk::DUAL_NMAX) return "ALGO_DUAL keeps X X^T (N x N doubles): N <= 8192";
    if (M > plsk::DUAL_MMAX) return "ALGO_DUAL: at most 32 responses";
    return nullptr;
}

// what every multi-item route of the plan (dual_round.hpp) asks of a call, besides its own *_REFIT switch and lower bound on N
inline bool dual_rounds_cover(const pls_hip_context *c, i64 N, i64 M) {
    return c->opt_algo == PLS_HIP_ALGO_DUAL && !c->reducer && c->nranks == 1 && N <= plsk::DUAL_NMAX && M <= plsk::DUAL_MMAX;
}

// The sweep over X that every user of the plan begins with (the fit here, the rounds of dual_round.hpp):
// c->dG = G = X X^T on the matrix cores, one bracket of PLS_HIP_FAM_XTY.
template <typename T>
int dual_gram(pls_hip_context *c, const T *X, i64 ldx, int N, int K) {
    const i64 NN = (i64)N * N, es = (i64)sizeof(T);
    // split of the sum over the columns of X: N is small, the blocks alone cannot fill the chip.  All workgroups resident at
    // once (two per CU) when the blocks allow it, no split otherwise; the partial blocks stay below 4 GB.
    const int nbn = (N + plsk::XXT_TB - 1) / plsk::XXT_TB, nblk = nbn * (nbn + 1) / 2;
    const i64 nslabs = ((i64)K + plsk::XXT_KC - 1) / plsk::XXT_KC, slots = 2 * (i64)c->num_cu;
    i64 S = plsk::row_splits(nblk, slots, 1);
    S = std::max<i64>(1, std::min<i64>(S, nslabs));
    S = std::max<i64>(1, std::min<i64>(S, ((i64)4 << 30) / (NN * 8)));
    const i64 per_split = (nslabs + S - 1) / S;
    S = (nslabs + per_split - 1) / per_split;  // (no split without a slab)
    CHK(ensure(c, c->dG, (size_t)NN * 8));
    CHK(ensure(c, c->dpart, (size_t)S * NN * 8));
    double *G = (double *)c->dG.p, *part = (double *)c->dpart.p;
    Range r_g("X X^T");
    Scope s(c, PLS_HIP_FAM_XTY, (i64)N * K * es + NN * 8);
    hipLaunchKernelGGL((plsk::xxt_kernel<T>), dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, c->stream, X, ldx, N, (i64)K, nbn,
                       per_split, part);
    LAUNCH_CHECK(c);
    hipLaunchKernelGGL(plsk::xxt_reduce_kernel, dim3((unsigned)nblk, plsk::XXT_TB * plsk::XXT_TB / 256), dim3(256), 0, c->stream,
                       (const double *)part, (int)S, N, nbn, G);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// Z (N x cols) = G Ya, dual_gy_kernel with the fewest accumulators that hold cols <= 32 columns
int launch_dual_gy(pls_hip_context *c, const double *G, const double *Ya, int N, int cols, double *Z) {
    Scope s(c, PLS_HIP_FAM_SMALL, ((i64)N * N + 2 * (i64)N * cols) * 8);
    pick_int<1, 2, 4, 8, 16, 32>(cols, [&](auto mt) {
        hipLaunchKernelGGL((plsk::dual_gy_kernel<decltype(mt)::value>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, G, Ya, N, cols, Z);
    });
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// One sweep of dual_xtv_kernel over X, a bracket of PLS_HIP_FAM_XTY: columns c0 .. c0 + nc - 1 (nc <= 64) of X^T V go to W[:, c0 + c]
// while c0 + c < A and to P[:, c0 + c - A] beyond (dual_kernels.hpp), with the fewest 16-column tiles that hold nc.
template <typename T>
int launch_dual_xtv(pls_hip_context *c, const T *X, i64 ldx, int N, i64 K, const double *V, int c0, int nc, int A, double *W, double *P) {
    Scope s(c, PLS_HIP_FAM_XTY, (i64)N * K * (i64)sizeof(T) + ((i64)N + K) * nc * 8);
    return pick_int<1, 2, 3, 4>((nc + 15) / 16, [&](auto nct) -> int {
        const auto kernel = plsk::dual_xtv_kernel<T, decltype(nct)::value>;
        if (!plsk::raise_dynamic_lds((const void *)kernel, (int)plsk::XTV_LDS_BYTES)) {
            s.on = false;
            return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the back-projection could not be raised");
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)((K + plsk::XTV_KB - 1) / plsk::XTV_KB)), dim3(256), plsk::XTV_LDS_BYTES, c->stream, X, ldx, N, K,
                           V, c0, nc, A, W, P);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    });
}

template <typename T>
int fit_dual(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N64, int K, int M, int A, double *W, double *P,
             double *Q, double *R, T *Tm, i64 ldt, double *B) {
    if (const char *why = dual_refusal(c, N64, M)) return fail(c, PLS_HIP_ERR_UNSUPPORTED, why);
    const int N = (int)N64;
    const i64 NN = (i64)N * N, es = (i64)sizeof(T);
    CHK(ensure(c, c->dG, (size_t)NN * 8));  // (dual_gram sizes it again: the pointers are taken before the sweep)
    CHK(ensure(c, c->dV, (size_t)N * 2 * A * 8));
    CHK(ensure(c, c->dT, (size_t)N * A * 8));
    CHK(ensure(c, c->dY, (size_t)N * M * 8));
    CHK(ensure(c, c->dZ, (size_t)N * M * 8));
    CHK(ensure(c, c->dC, (size_t)A * A * 8));
    CHK(ensure(c, c->dscr, (size_t)(N + 2 * (i64)A) * 8));
    double *G = (double *)c->dG.p, *V = (double *)c->dV.p, *T64 = (double *)c->dT.p;
    double *Ya = (double *)c->dY.p, *Z = (double *)c->dZ.p, *C = (double *)c->dC.p;
    double *ttv = (double *)c->dscr.p, *scr = ttv + A;

    Range r_fit("pls_hip_fit (sample space)");
    CHK(dual_gram<T>(c, X, ldx, N, K));  // first sweep over X: G = X X^T
    {
        Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * M * (es + 8));
        hipLaunchKernelGGL((plsk::dual_convert_kernel<T, double>), dim3((unsigned)(((i64)N * M + 255) / 256)), dim3(256), 0, c->stream, Y,
                           ldy, Ya, (i64)N, N, M);
        LAUNCH_CHECK(c);
    }
    for (int a = 0; a < A; ++a) {
        Range r_comp("component", a);
        CHK(launch_dual_gy(c, G, Ya, N, M, Z));
        {
            Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * (3 * M + a + 4) * 8);
            hipLaunchKernelGGL(plsk::dual_step_kernel, dim3(1), dim3(plsk::UPD_THREADS), 0, c->stream, (const double *)Z, Ya, T64, V, Q, C,
                               ttv, scr, N, M, A, a, (int)c->opt_power_iters);
            LAUNCH_CHECK(c);
        }
    }
    {  // second sweep over X (one per 64 columns of [U | T]): [W | P] = X^T [U | T diag(1/tt)]
        Range r_b("X^T [U T]");
        for (int c0 = 0; c0 < 2 * A; c0 += plsk::XTV_NC) {
            const int nc = std::min(plsk::XTV_NC, 2 * A - c0);
            CHK(launch_dual_xtv<T>(c, X, ldx, N, (i64)K, (const double *)V, c0, nc, A, W, P));
        }
    }
    {
        Scope s(c, PLS_HIP_FAM_SMALL, ((i64)K * A * (A + 3) / 2 + (i64)A * A) * 8);
        hipLaunchKernelGGL(plsk::dual_r_kernel, dim3((unsigned)(((i64)K + 255) / 256)), dim3(256), 0, c->stream, (const double *)W,
                           (const double *)C, (i64)K, A, R);
        LAUNCH_CHECK(c);
    }
    if (B) {
        Scope s(c, PLS_HIP_FAM_SMALL, ((i64)K * A + (i64)M * A + (i64)K * M) * 8);
        const int nblkb = (int)(((i64)K * M + plsk::WG - 1) / plsk::WG);
        hipLaunchKernelGGL(plsk::coefficients_kernel, dim3(nblkb), dim3(plsk::WG), 0, c->stream, R, Q, K, M, A, B);
        LAUNCH_CHECK(c);
    }
    {
        Scope s(c, PLS_HIP_FAM_SMALL, (i64)N * A * (es + 8));
        hipLaunchKernelGGL((plsk::dual_convert_kernel<double, T>), dim3((unsigned)(((i64)N * A + 255) / 256)), dim3(256), 0, c->stream,
                           (const double *)T64, (i64)N, Tm, ldt, N, A);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

}  // namespace
