// plan_missing.hpp -- NIPALS fits of X with missing values (pls_hip_fit_missing), scores of rows with missing cells
// (pls_hip_scores_missing) and column statistics over the observed cells (pls_hip_colwise_z_scores_missing): one route each,
// over the kernels of missing_kernels.hpp.  DESIGN.md f13 has the launches and the bytes per component.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

constexpr int MISS_BATCH = 8;  // iterations of the M > 1 loop enqueued between two reads of the convergence word

// geometry of the three sweeps of one call: miss_layout.hpp, a pure function of (N, K, type, CU count)
using plsk::MissGeom;
template <typename T>
MissGeom miss_geom(const pls_hip_context *c, i64 N, int K) {
    return plsk::miss_geom_of(N, K, (int)sizeof(T), c->num_cu);
}

// the small workspace of a call, carved from c->mws in doubles
struct MissWs {
    double *u, *t, *tprev, *Ya, *colpart, *sspart, *tpart, *ypart, *yss, *cvec, *qq;
    int *jstar, *stop;
};
int miss_workspace(pls_hip_context *c, const MissGeom &g, i64 N, int K, int M, int A, MissWs *w) {
    i64 off = 0;
    auto take = [&](i64 n) { const i64 o = off; off += (n + 1) & ~(i64)1; return o; };
    const i64 o_u = take(N), o_t = take(N), o_tp = take(N), o_ya = take(N * M), o_cp = take((i64)g.G * K * 2), o_ss = take(g.nbK),
              o_tpart = take(g.S > 1 ? (i64)g.S * N * 2 : 0), o_yp = take((i64)g.GY * (M + 2)), o_yss = take((i64)g.GY * M),
              o_c = take((i64)A * plsk::MISS_PW_SLICES), o_qq = take(2), o_words = take(2);
    CHK(ensure(c, c->mws, (size_t)off * 8));
    double *b = (double *)c->mws.p;
    *w = MissWs{b + o_u, b + o_t, b + o_tp, b + o_ya, b + o_cp, b + o_ss, g.S > 1 ? b + o_tpart : nullptr, b + o_yp, b + o_yss,
                b + o_c, b + o_qq, (int *)(b + o_words), (int *)(b + o_words) + 1};
    return PLS_HIP_OK;
}

// The column sweep: [deflate and store] and / or accumulate, then the quotient -> out (K values), sspart for w
template <typename T>
int miss_col_sweep(pls_hip_context *c, const MissGeom &g, const T *src, i64 lds, T *dst, i64 ldd, i64 N, int K, const double *v,
                   const double *tp, const double *pp, bool store, bool defl, bool acc, const MissWs &w, double *out, bool want_ss,
                   const int *stop) {
    constexpr int FV = 16 / (int)sizeof(T);
    const bool wide = plsk::vec_ok((uintptr_t)src, lds, sizeof(T), FV) && (!store || plsk::vec_ok((uintptr_t)dst, ldd, sizeof(T), FV));
    const dim3 grid((unsigned)g.nkg, (unsigned)g.G), blk(plsk::WG);
    {
        Scope s(c, store ? PLS_HIP_FAM_DEFLATE : PLS_HIP_FAM_XTY, (store ? 2 : 1) * N * (i64)K * (i64)sizeof(T) + (2 * N + 2 * (i64)K) * 8);
#define MISS_COL(V_, S_, D_, A_) \
    hipLaunchKernelGGL((plsk::miss_col_kernel<T, V_, S_, D_, A_>), grid, blk, 0, c->stream, src, lds, dst, ldd, N, K, v, tp, pp, w.colpart, stop)
#define MISS_COL_V(S_, D_, A_) do { if (wide) MISS_COL(FV, S_, D_, A_); else MISS_COL(1, S_, D_, A_); } while (0)
        if (store && defl && acc) MISS_COL_V(true, true, true);
        else if (store && acc) MISS_COL_V(true, false, true);
        else if (store && defl) MISS_COL_V(true, true, false);
        else if (store) MISS_COL_V(true, false, false);
        else MISS_COL_V(false, false, true);
#undef MISS_COL_V
#undef MISS_COL
        LAUNCH_CHECK(c);
    }
    if (!acc) return PLS_HIP_OK;
    Scope s(c, PLS_HIP_FAM_SMALL, (i64)g.G * K * 16);
    hipLaunchKernelGGL(plsk::miss_col_finish_kernel, dim3((unsigned)g.nbK), dim3(plsk::WG), 0, c->stream, (const double *)w.colpart, g.G, K,
                       out, want_ss ? w.sspart : nullptr, stop);
    LAUNCH_CHECK(c);
    if (want_ss) {
        hipLaunchKernelGGL(plsk::miss_normalize_kernel, dim3((unsigned)g.nbK), dim3(plsk::WG), 0, c->stream, out, K,
                           (const double *)w.sspart, (int)g.nbK, stop);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

// The row sweep over the work copy: t = (sum_obs x w) / (sum_obs w^2)
template <typename T>
int miss_row_sweep(pls_hip_context *c, const MissGeom &g, const T *work, i64 N, int K, const double *wv, const MissWs &w, const int *stop) {
    constexpr int FV = 16 / (int)sizeof(T);
    {
        Scope s(c, PLS_HIP_FAM_XB, N * (i64)K * (i64)sizeof(T) + ((i64)K + N) * 8 + (g.S > 1 ? (i64)g.S * N * 32 : 0));
        hipLaunchKernelGGL((plsk::miss_row_kernel<T, FV>), dim3((unsigned)g.nrb, (unsigned)g.S), dim3(plsk::WG), 0, c->stream, work, g.ldw, N, K,
                           wv, g.lrl, g.kper, w.t, w.tpart, stop);
        LAUNCH_CHECK(c);
    }
    if (g.S > 1) {
        hipLaunchKernelGGL(plsk::miss_row_finish_kernel, dim3((unsigned)((N + plsk::MISS_RF_ROWS - 1) / plsk::MISS_RF_ROWS)), dim3(plsk::WG), 0,
                           c->stream, (const double *)w.tpart, g.S, N, w.t, stop);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

// All pointers device memory.  M == 1: enqueues only.  M > 1: returns after the work has completed.
template <typename T>
int fit_missing_device(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M, int A, double *W, double *P,
                       double *Q, double *R, T *Tm, i64 ldt, double *B, long long *iters) {
    const MissGeom g = miss_geom<T>(c, N, K);
    MissWs w;
    CHK(miss_workspace(c, g, N, K, M, A, &w));
    CHK(ensure(c, c->mX, (size_t)g.ldw * K * sizeof(T)));
    T *work = (T *)c->mX.p;
    const bool multi = M > 1;
    const int max_it = (int)c->opt_missing_iters;
    if (multi && !c->mconv_host) HIPCHK(c, hipHostMalloc((void **)&c->mconv_host, 64, hipHostMallocDefault));
    const dim3 blk(plsk::WG), gN((unsigned)g.nbN), gK((unsigned)g.nbK), gY((unsigned)g.GY);
    const int *stop = multi ? w.stop : nullptr;

    hipLaunchKernelGGL((plsk::miss_y_init_kernel<T>), gY, blk, 0, c->stream, Y, ldy, N, M, w.Ya, multi ? w.yss : nullptr);
    LAUNCH_CHECK(c);
    for (int a = 0; a < A; ++a) {
        Range r_comp("component", a);
        double *wa = W + (i64)a * K, *pa = P + (i64)a * K, *qa = Q + (i64)a * M;
        const double *u = w.Ya;
        if (multi) {
            hipLaunchKernelGGL(plsk::miss_u_pick_kernel, dim3(1), dim3(plsk::WAVE), 0, c->stream, (const double *)w.yss, g.GY, M, w.jstar, w.stop);
            LAUNCH_CHECK(c);
            hipLaunchKernelGGL(plsk::miss_u_copy_kernel, gN, blk, 0, c->stream, (const double *)w.Ya, N, (const int *)w.jstar, w.u);
            LAUNCH_CHECK(c);
            u = w.u;
        }
        bool done = false;
        for (int it = 1; !done; ++it) {
            if (it == 1) {
                // deflate-and-accumulate: reads X_{a-1} (the caller's matrix for a = 0), stores X_a, sums for w with u_a
                if (a == 0) CHK(miss_col_sweep<T>(c, g, X, ldx, work, g.ldw, N, K, u, nullptr, nullptr, true, false, true, w, wa, true, stop));
                else CHK(miss_col_sweep<T>(c, g, work, g.ldw, work, g.ldw, N, K, u, w.t, pa - K, true, true, true, w, wa, true, stop));
            } else {
                hipLaunchKernelGGL(plsk::miss_u_kernel, gN, blk, 0, c->stream, (const double *)w.Ya, N, M, (const double *)qa,
                                   (const double *)w.qq, w.u, stop);
                LAUNCH_CHECK(c);
                CHK(miss_col_sweep<T>(c, g, work, g.ldw, work, g.ldw, N, K, u, nullptr, nullptr, false, false, true, w, wa, true, stop));
            }
            CHK(miss_row_sweep<T>(c, g, work, N, K, wa, w, stop));
            hipLaunchKernelGGL(plsk::miss_yt_kernel, gY, blk, 0, c->stream, (const double *)w.Ya, N, M, (const double *)w.t, w.tprev, w.ypart, stop);
            LAUNCH_CHECK(c);
            hipLaunchKernelGGL(plsk::miss_q_kernel, dim3(1), dim3(plsk::WAVE), 0, c->stream, (const double *)w.ypart, g.GY, M, it, max_it, qa,
                               w.qq, multi ? w.stop : nullptr, iters ? iters + a : nullptr);
            LAUNCH_CHECK(c);
            if (!multi || it >= max_it) {
                done = true;
            } else if (it % MISS_BATCH == 0) {  // the host reads the convergence word through pinned memory
                HIPCHK(c, hipMemcpyAsync(c->mconv_host, w.stop, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                done = *c->mconv_host != 0;
            }
        }
        CHK(miss_col_sweep<T>(c, g, work, g.ldw, work, g.ldw, N, K, w.t, nullptr, nullptr, false, false, true, w, pa, false, nullptr));
        {
            Scope s(c, PLS_HIP_FAM_SMALL, (i64)K * (a + 2) * 8 * 2);
            const int PB = (int)std::min<i64>(plsk::MISS_PW_SLICES, g.nbK);
            if (a > 0) {
                hipLaunchKernelGGL(plsk::miss_pw_kernel, dim3(PB, a), blk, 0, c->stream, (const double *)P, (const double *)wa, K, w.cvec);
                LAUNCH_CHECK(c);
            }
            hipLaunchKernelGGL(plsk::miss_r_kernel, gK, blk, 0, c->stream, (const double *)wa, (const double *)R, (const double *)w.cvec, PB, a,
                               K, R + (i64)a * K);
            LAUNCH_CHECK(c);
            hipLaunchKernelGGL((plsk::miss_store_scores_kernel<T>), gN, blk, 0, c->stream, (const double *)w.t, N, Tm + (i64)a * ldt);
            LAUNCH_CHECK(c);
            if (a + 1 < A) {
                hipLaunchKernelGGL(plsk::miss_y_deflate_kernel, gY, blk, 0, c->stream, w.Ya, N, M, (const double *)w.t, (const double *)qa,
                                   multi ? w.yss : nullptr);
                LAUNCH_CHECK(c);
            }
        }
    }
    if (B) {
        hipLaunchKernelGGL(plsk::coefficients_kernel, dim3((unsigned)(((i64)K * M + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream,
                           (const double *)R, (const double *)Q, K, M, A, B);
        LAUNCH_CHECK(c);
    }
    if (multi) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PLS_HIP_OK;
}

// Sequential deflation of rows with the model's W, P: t_a from the row sweep, x <- x - t_a p_a with the fit's own sweep
template <typename T>
int scores_missing_device(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, int A, const double *W, const double *P, T *S, i64 lds) {
    const MissGeom g = miss_geom<T>(c, N, K);
    MissWs w;
    CHK(miss_workspace(c, g, N, K, 1, A, &w));
    CHK(ensure(c, c->mX, (size_t)g.ldw * K * sizeof(T)));
    T *work = (T *)c->mX.p;
    for (int a = 0; a < A; ++a) {
        if (a == 0) CHK(miss_col_sweep<T>(c, g, X, ldx, work, g.ldw, N, K, nullptr, nullptr, nullptr, true, false, false, w, nullptr, false, nullptr));
        else CHK(miss_col_sweep<T>(c, g, work, g.ldw, work, g.ldw, N, K, nullptr, w.t, P + (i64)(a - 1) * K, true, true, false, w, nullptr, false, nullptr));
        CHK(miss_row_sweep<T>(c, g, work, N, K, W + (i64)a * K, w, nullptr));
        hipLaunchKernelGGL((plsk::miss_store_scores_kernel<T>), dim3((unsigned)g.nbN), dim3(plsk::WG), 0, c->stream, (const double *)w.t, N,
                           S + (i64)a * lds);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

// mean, sd, nobs over the observed cells in one sweep, then Z = (X - mean) / sd (Z may be null or X)
template <typename T>
int zscores_missing_device(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, T *Z, i64 ldz, double *mean, double *sd, long long *nobs) {
    const i64 nch = (N + plsk::WG - 1) / plsk::WG;
    const int G = (int)std::min<i64>(std::min<i64>(std::max<i64>(1, (8 * (i64)c->num_cu) / K), nch), 65535);
    CHK(ensure(c, c->mws, (size_t)G * K * 4 * 8));  // (n, anchor, mean - anchor, M2) per row group and column
    double *part = (double *)c->mws.p;
    const dim3 grid((unsigned)K, (unsigned)G), blk(plsk::WG);
    {
        Scope s(c, PLS_HIP_FAM_XTY, N * (i64)K * (i64)sizeof(T) + 3 * (i64)K * 8);
        hipLaunchKernelGGL((plsk::miss_colmoments_kernel<T>), grid, blk, 0, c->stream, X, ldx, N, K, part);
        LAUNCH_CHECK(c);
    }
    hipLaunchKernelGGL(plsk::miss_colmoments_finish_kernel, dim3((unsigned)(((i64)K + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream,
                       (const double *)part, G, K, mean, sd, nobs);
    LAUNCH_CHECK(c);
    if (Z) {
        Scope s(c, PLS_HIP_FAM_DEFLATE, 2 * N * (i64)K * (i64)sizeof(T) + 2 * (i64)K * 8);
        const dim3 g2((unsigned)K, (unsigned)std::min<i64>(std::min<i64>(std::max<i64>(1, (16 * (i64)c->num_cu) / K), nch), 65535));
        hipLaunchKernelGGL((plsk::miss_zscale_kernel<T>), g2, blk, 0, c->stream, X, ldx, Z, ldz, N, (const double *)mean, (const double *)sd);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

}  // namespace
