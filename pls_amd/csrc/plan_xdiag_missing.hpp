// plan_xdiag_missing.hpp -- X-space diagnostics of rows with missing cells (pls_hip_x_diagnostics_missing): scores, Q residuals for
// every component count, T^2, ssx, sst and the observed cells per row from ONE read of X (row-resident route) or A + 1 read-only
// sweeps (streaming route), over the kernels of xdiag_missing_kernels.hpp.  The route, the tile, the K split and the workspace are
// xdiagmiss_geom_of's (xdiagmiss_layout.hpp); this file only executes them.  DESIGN.md f14 has the launches per call.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

static_assert(plsk::XDM_RED_SLICES == plsk::RED_SLICES, "the slices of xdiagmiss_layout.hpp are those of reduce_partials_kernel");

// All pointers device memory; enqueues only.  Any of Qres, T2, S, ssx, sst, nobs may be null; tvar null = from this call's scores.
template <typename T>
int xdiag_missing_device(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, int A, const double *W, const double *P,
                         const double *tvar, double *Qres, i64 ldq, double *T2, i64 ldt2, T *S, i64 lds, double *ssx, double *sst,
                         long long *nobs) {
    constexpr int FV = 16 / (int)sizeof(T);
    constexpr bool F64 = std::is_same<T, double>::value;
    const bool aligned = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), FV);
    const plsk::XdmGeom g = plsk::xdiagmiss_geom_of(N, K, A, (int)sizeof(T), c->num_cu, aligned, c->env.xdiagmiss_stream);
    CHK(ensure(c, c->xmws, (size_t)g.ws_bytes));
    char *ws = (char *)c->xmws.p;
    const i64 LP = 2 * (i64)A + 1;
    const bool own_tvar = T2 && !tvar, need_sst = sst || own_tvar, need_q = Qres || ssx, need_red = ssx || need_sst;
    const dim3 blk(plsk::WG);
    // where the kernels write: an output that is asked for in fp64 is written in place, everything else goes to the workspace
    double *Sd = (F64 && S) ? (double *)S : (double *)(ws + g.o_sd);
    const i64 ldsd = (F64 && S) ? lds : N;
    double *q0 = ssx ? (double *)(ws + g.o_q0) : nullptr;
    double *Qd = Qres ? Qres : (ssx ? (double *)(ws + g.o_qd) : nullptr);
    const i64 ldqd = Qres ? ldq : N;
    const int npass = need_q ? A + 1 : A;
    double *red = (double *)(ws + g.o_red);
    if (need_red) HIPCHK(c, hipMemsetAsync(red, 0, (size_t)plsk::RED_SLICES * LP * 8, c->stream));
    const i64 out_bytes = N * (i64)A * 8 + (need_q ? N * (i64)(A + 1) * 8 : 0) + (nobs ? N * 8 : 0) + 2 * (i64)K * A * 8;

    if (g.route == plsk::XDM_RESIDENT) {
        int lrt = 0;
        while ((1 << lrt) < g.rt) ++lrt;
        Scope s(c, PLS_HIP_FAM_XB, N * (i64)K * (i64)sizeof(T) + out_bytes);
#define XDM_RES(V_)                                                                                                                      \
    do {                                                                                                                                 \
        if (!plsk::raise_dynamic_lds((const void *)plsk::xdm_resident_kernel<T, V_>, (int)g.lds_bytes))                                  \
            return fail(c, PLS_HIP_ERR_DEVICE, "x_diagnostics_missing: the resident tile does not fit the device's LDS");                \
        hipLaunchKernelGGL((plsk::xdm_resident_kernel<T, V_>), dim3((unsigned)g.ntiles), blk, (size_t)g.lds_bytes, c->stream, X, ldx, N, K, \
                           A, lrt, npass, W, P, Sd, ldsd, q0, Qd, ldqd, nobs);                                                           \
    } while (0)
        if (g.vec > 1) XDM_RES(FV); else XDM_RES(1);
#undef XDM_RES
        LAUNCH_CHECK(c);
    } else {
        double *part = (double *)(ws + g.o_part);
        const dim3 grid((unsigned)g.nrb, (unsigned)g.S), gfin((unsigned)((N + plsk::MISS_RF_ROWS - 1) / plsk::MISS_RF_ROWS));
        for (int a = 0; a < npass; ++a) {
            const int last = a == A ? 1 : 0;
            const double *wa = last ? nullptr : W + (i64)a * K;
            {
                Scope s(c, PLS_HIP_FAM_XB, N * (i64)K * (i64)sizeof(T) + (i64)g.S * N * plsk::XDM_PART * 8 + (i64)K * (a + 1) * 8 + N * (i64)a * 8);
                if (g.vec > 1)
                    hipLaunchKernelGGL((plsk::xdm_stream_kernel<T, FV>), grid, blk, 0, c->stream, X, ldx, N, K, a, last, wa, P,
                                       (const double *)Sd, ldsd, g.lrl, g.kper, part);
                else
                    hipLaunchKernelGGL((plsk::xdm_stream_kernel<T, 1>), grid, blk, 0, c->stream, X, ldx, N, K, a, last, wa, P,
                                       (const double *)Sd, ldsd, g.lrl, g.kper, part);
                LAUNCH_CHECK(c);
            }
            Scope s(c, PLS_HIP_FAM_SMALL, (i64)g.S * N * plsk::XDM_PART * 8 + 2 * N * 8);
            hipLaunchKernelGGL(plsk::xdm_stream_finish_kernel, gfin, blk, 0, c->stream, (const double *)part, g.S, N,
                               last ? nullptr : Sd + (i64)a * ldsd, a == 0 ? q0 : (Qd ? Qd + (i64)(a - 1) * ldqd : nullptr),
                               a == 0 ? nobs : nullptr);
            LAUNCH_CHECK(c);
        }
    }
    // ---- ssx: column sums of q_0 and of the Q columns; sst and the fp32 copy of the scores: the kernels of pls_hip_x_diagnostics
    const int G = (int)std::min<i64>((N + plsk::WG - 1) / plsk::WG, 4 * (i64)c->num_cu);
    constexpr int CH = 1024;  // columns per launch: (WG / WAVE) * CH doubles of LDS
    if (ssx) {
        CHK(ensure(c, c->part, (size_t)G * std::min(A, CH) * 8));
        double *part = (double *)c->part.p;
        {
            Scope s(c, PLS_HIP_FAM_SMALL, N * 8);
            hipLaunchKernelGGL(plsk::xdiag_score_stats_kernel<false>, dim3(G), blk, (size_t)(plsk::WG / plsk::WAVE) * 8, c->stream,
                               (const double *)q0, N, N, 0, 1, (float *)nullptr, (i64)0, part);
            LAUNCH_CHECK(c);
        }
        CHK(launch_reduce(c, part, G, 1, nullptr, 0, red, LP));
        for (int c_lo = 0; c_lo < A; c_lo += CH) {
            const int nc = std::min(A, c_lo + CH) - c_lo;
            {
                Scope s(c, PLS_HIP_FAM_SMALL, N * (i64)nc * 8);
                hipLaunchKernelGGL(plsk::xdiag_score_stats_kernel<false>, dim3(G), blk, (size_t)(plsk::WG / plsk::WAVE) * nc * 8,
                                   c->stream, (const double *)(Qd + (i64)c_lo * ldqd), ldqd, N, 0, nc, (float *)nullptr, (i64)0, part);
                LAUNCH_CHECK(c);
            }
            CHK(launch_reduce(c, part, G, nc, nullptr, 0, red + 1 + c_lo, LP));
        }
    }
    const bool copy_s = !F64 && S;
    if (need_sst || copy_s) {
        for (int c_lo = 0; c_lo < A; c_lo += CH) {
            const int c_hi = std::min(A, c_lo + CH), nc = c_hi - c_lo;
            double *part = nullptr;
            if (need_sst) {
                CHK(ensure(c, c->part, (size_t)G * nc * 8));
                part = (double *)c->part.p;
            }
            {
                Scope s(c, PLS_HIP_FAM_SMALL, N * (i64)nc * 12);
                hipLaunchKernelGGL(plsk::xdiag_score_stats_kernel<true>, dim3(G), blk, (size_t)(plsk::WG / plsk::WAVE) * nc * 8,
                                   c->stream, (const double *)Sd, ldsd, N, c_lo, c_hi, copy_s ? (float *)S : nullptr, lds, part);
                LAUNCH_CHECK(c);
            }
            if (need_sst) CHK(launch_reduce(c, part, G, nc, nullptr, 0, red + A + 1 + c_lo, LP));
        }
    }
    const double *tv = tvar;
    if (need_red) {
        double *tw = own_tvar ? (double *)(ws + g.o_tv) : nullptr;
        if (tw) tv = tw;
        hipLaunchKernelGGL(plsk::xdiag_finish_kernel, dim3((unsigned)((LP + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream, (const double *)red, A,
                           (double)(N - 1), ssx, sst, tw);
        LAUNCH_CHECK(c);
    }
    if (T2) {
        hipLaunchKernelGGL(plsk::xdiag_t2_kernel, dim3((unsigned)((N + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream, (const double *)Sd, ldsd,
                           N, A, tv, T2, ldt2);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

}  // namespace
