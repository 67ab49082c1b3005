// plan_xdiag.hpp -- X-space diagnostics of a model on the device: scores, the residual sweep for every component count, T^2.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

constexpr int XD_RANGE = 24;  // component counts per sweep: 4 VGPRs each (score + running sum of one row) -- kernel_resources.md

// rows of the transposed loadings: A rounded up to whole ranges, so that a range's kernel reads its CR <= XD_RANGE values untested
int xdiag_ap(int A) { return (A + XD_RANGE - 1) / XD_RANGE * XD_RANGE; }

// M^T (AP x K, zero-padded) of R or P in the handle's workspace (the scores are done with R^T before the sweep takes the buffer for P^T)
int xdiag_transposed(pls_hip_context *c, const double *M, int K, int A, const double **MT) {
    const int AP = xdiag_ap(A);
    CHK(ensure(c, c->xdPT, (size_t)K * AP * 8));
    hipLaunchKernelGGL(plsk::xdiag_transpose_kernel, dim3((unsigned)(((i64)K * AP + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream, M,
                       K, A, AP, (double *)c->xdPT.p);
    LAUNCH_CHECK(c);
    *MT = (const double *)c->xdPT.p;
    return PLS_HIP_OK;
}

template <typename T, int VEC>
int xdiag_launch_scores(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, const double *RT, int A, int c_lo, int c_hi,
                        double *Sd, i64 ldsd) {
    const dim3 grid((unsigned)((N + (i64)plsk::WG * VEC - 1) / ((i64)plsk::WG * VEC))), blk(plsk::WG);
    Scope s(c, PLS_HIP_FAM_XB, (i64)N * K * sizeof(T) + (i64)N * (c_hi - c_lo) * 8);
    const int AP = xdiag_ap(A);
    if (c_hi - c_lo <= 8)
        hipLaunchKernelGGL((plsk::xdiag_scores_kernel<T, VEC, 8>), grid, blk, 0, c->stream, X, ldx, N, K, RT, AP, c_lo, c_hi, Sd, ldsd);
    else if (c_hi - c_lo <= 16)
        hipLaunchKernelGGL((plsk::xdiag_scores_kernel<T, VEC, 16>), grid, blk, 0, c->stream, X, ldx, N, K, RT, AP, c_lo, c_hi, Sd, ldsd);
    else
        hipLaunchKernelGGL((plsk::xdiag_scores_kernel<T, VEC, XD_RANGE>), grid, blk, 0, c->stream, X, ldx, N, K, RT, AP, c_lo, c_hi, Sd, ldsd);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

template <typename T, int VEC, int CR>
void xdiag_launch_sweep_t(pls_hip_context *c, dim3 grid, const T *X, i64 ldx, i64 N, int K, int kper, const double *Sd, i64 ldsd,
                          const double *PT, int A, int c_lo, int c_hi, double *xout, double *qout, i64 ldq, i64 slice, int first,
                          double *part) {
    hipLaunchKernelGGL((plsk::xdiag_sweep_kernel<T, VEC, CR>), grid, dim3(plsk::WG), 0, c->stream, X, ldx, N, K, kper, Sd, ldsd, PT,
                       xdiag_ap(A), c_lo, c_hi, xout, qout, ldq, slice, first, part);
}

// The score stage of xdiag_device and vardiag_device (plan_vardiag.hpp): Sd (N x A, ld *ldsd) = X R in fp64 whatever the storage
// type -- launch_xb for fp64 storage, into S when the caller's own fp64 output takes them, xdiag_scores_kernel for fp32 storage.
// N >= 1.  Uses c->xdS (the scores) and c->xdPT (R^T).
template <typename T>
int xdiag_scores(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, int A, const double *R, T *S, i64 lds, const double **Sd_out,
                 i64 *ldsd_out) {
    const double *Sd = nullptr;
    i64 ldsd = 0;
    if (std::is_same<T, double>::value && S) {
        Sd = (const double *)S;
        ldsd = lds;
        int nss = 0;
        CHK(launch_xb<double>(c, (const double *)X, ldx, N, K, R, K, A, (double *)S, lds, nullptr, &nss));
    } else {
        const i64 ldn = N + (N & 1);
        CHK(ensure(c, c->xdS, (size_t)ldn * A * 8));
        double *ws = (double *)c->xdS.p;
        Sd = ws;
        ldsd = ldn;
        if (std::is_same<T, double>::value) {
            int nss = 0;
            CHK(launch_xb<double>(c, (const double *)X, ldx, N, K, R, K, A, ws, ldn, nullptr, &nss));
        } else {
            const bool wide = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), 2);
            const double *RT = nullptr;
            CHK(xdiag_transposed(c, R, K, A, &RT));
            for (int c_lo = 0; c_lo < A; c_lo += XD_RANGE) {
                const int c_hi = std::min(A, c_lo + XD_RANGE);
                if (wide) CHK((xdiag_launch_scores<T, 2>(c, X, ldx, N, K, RT, A, c_lo, c_hi, ws, ldn)));
                else CHK((xdiag_launch_scores<T, 1>(c, X, ldx, N, K, RT, A, c_lo, c_hi, ws, ldn)));
            }
        }
    }
    *Sd_out = Sd;
    *ldsd_out = ldsd;
    return PLS_HIP_OK;
}

// All pointers are device memory.  Any of Qres, T2, S, ssx, sst may be null; tvar null = derive it from this call's scores.
// On a handle with a reducer the call sends exactly one message of RED_SLICES * (2A + 1) values, whatever was asked for.
template <typename T>
int xdiag_device(pls_hip_context *c, const T *X, i64 ldx, i64 N, i64 n_total, int K, int A, const double *R, const double *P,
                 const double *tvar, double *Qres, i64 ldq, double *T2, i64 ldt2, T *S, i64 lds, double *ssx, double *sst) {
    const i64 LP = 2 * (i64)A + 1;
    const bool own_tvar = T2 && !tvar;
    const bool need_sweep = (Qres || ssx) && N > 0;
    const bool need_sst = sst || own_tvar;
    const bool need_red = ssx || need_sst || c->reducer;
    const dim3 blk(plsk::WG);
    double *red = nullptr;
    if (need_red) {
        CHK(ensure(c, c->xdred, (size_t)plsk::RED_SLICES * LP * 8));
        red = (double *)c->xdred.p;
        HIPCHK(c, hipMemsetAsync(red, 0, (size_t)plsk::RED_SLICES * LP * 8, c->stream));
    }
    // ---- scores, fp64 whatever the storage type
    const double *Sd = nullptr;
    i64 ldsd = 0;
    if (N > 0) CHK(xdiag_scores<T>(c, X, ldx, N, K, A, R, S, lds, &Sd, &ldsd));
    // ---- the residual sweep: XD_RANGE component counts at a time
    if (need_sweep) {
        const bool wide = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), 2);
        const double *PT = nullptr;
        CHK(xdiag_transposed(c, P, K, A, &PT));
        for (int c_lo = 0; c_lo < A; c_lo += XD_RANGE) {
            const int c_hi = std::min(A, c_lo + XD_RANGE), nc = c_hi - c_lo;
            const int CR = (nc + 3) / 4 * 4;                   // the kernel computes all CR counts: at most three idle ones
            const int vec = (wide && CR <= 16) ? 2 : 1;        // (more than 16 counts of two rows would not fit the registers)
            const i64 nrb = (N + (i64)plsk::WG * vec - 1) / ((i64)plsk::WG * vec);
            // short and wide: fewer row groups than CUs -- column blocks of at least 128 columns, about two workgroups per CU
            int KS = 1, kper = K;
            if (nrb < c->num_cu && K >= 256) {
                KS = (int)std::min<i64>((2 * (i64)c->num_cu + nrb - 1) / nrb, K / 128);
                kper = ((K + KS - 1) / KS + 7) / 8 * 8;
                KS = (K + kper - 1) / kper;
            }
            const int first = c_lo == 0 ? 1 : 0, L = nc + first;
            double *qcol = Qres ? Qres + (i64)c_lo * ldq : nullptr;
            double *part = nullptr, *xout = nullptr, *qout = qcol;
            i64 oldq = ldq, slice = 0;
            i64 nb = nrb;
            if (KS > 1) {
                CHK(ensure(c, c->xdQ, (size_t)KS * (nc + 1) * N * 8));
                xout = (double *)c->xdQ.p;
                qout = xout + N;
                oldq = N;
                slice = (i64)(nc + 1) * N;
                nb = (N + plsk::WG - 1) / plsk::WG;
            }
            if (ssx) {
                CHK(ensure(c, c->part, (size_t)nb * L * 8));
                part = (double *)c->part.p;
            }
            {
                Scope s(c, PLS_HIP_FAM_XB, (i64)N * K * sizeof(T) + (i64)N * (c_hi + nc) * 8 + (i64)K * c_hi * 8);
                const dim3 grid((unsigned)nrb, (unsigned)KS);
                double *kpart = KS > 1 ? nullptr : part;
#define XD_SWEEP(V_, C_) xdiag_launch_sweep_t<T, V_, C_>(c, grid, X, ldx, N, K, kper, Sd, ldsd, PT, A, c_lo, c_hi, xout, qout, oldq, slice, first, kpart)
                switch (CR) {
                    case 4: if (vec == 2) XD_SWEEP(2, 4); else XD_SWEEP(1, 4); break;
                    case 8: if (vec == 2) XD_SWEEP(2, 8); else XD_SWEEP(1, 8); break;
                    case 12: if (vec == 2) XD_SWEEP(2, 12); else XD_SWEEP(1, 12); break;
                    case 16: if (vec == 2) XD_SWEEP(2, 16); else XD_SWEEP(1, 16); break;
                    case 20: XD_SWEEP(1, 20); break;
                    default: XD_SWEEP(1, XD_RANGE); break;
                }
#undef XD_SWEEP
                LAUNCH_CHECK(c);
            }
            if (KS > 1) {
                hipLaunchKernelGGL(plsk::xdiag_split_finish_kernel, dim3((unsigned)nb), blk, (size_t)(plsk::WG / plsk::WAVE) * (nc + 1) * 8,
                                   c->stream, (const double *)c->xdQ.p, N, nc, KS, first, qcol, ldq, part);
                LAUNCH_CHECK(c);
            }
            if (ssx) CHK(launch_reduce(c, part, (int)nb, L, nullptr, 0, red + (first ? 0 : 1 + c_lo), LP));
        }
    }
    // ---- column sums of squares of the scores; the fp32 copy of the scores
    const bool copy_s = !std::is_same<T, double>::value && S;
    if ((need_sst || copy_s) && N > 0) {
        const int G = (int)std::min<i64>((N + plsk::WG - 1) / plsk::WG, 4 * (i64)c->num_cu);
        for (int c_lo = 0; c_lo < A; c_lo += 1024) {
            const int c_hi = std::min(A, c_lo + 1024), nc = c_hi - c_lo;
            double *part = nullptr;
            if (need_sst) {
                CHK(ensure(c, c->part, (size_t)G * nc * 8));
                part = (double *)c->part.p;
            }
            hipLaunchKernelGGL(plsk::xdiag_score_stats_kernel<true>, dim3(G), blk, (size_t)(plsk::WG / plsk::WAVE) * nc * 8, c->stream, Sd, ldsd,
                               N, c_lo, c_hi, copy_s ? (float *)S : nullptr, lds, part);
            LAUNCH_CHECK(c);
            if (need_sst) CHK(launch_reduce(c, part, G, nc, nullptr, 0, red + A + 1 + c_lo, LP));
        }
    }
    // ---- one message for ssx and sst, then the values and tvar
    const double *tv = tvar;
    if (need_red) {
        CHK(do_allreduce(c, red, (i64)plsk::RED_SLICES * LP));
        double *tw = nullptr;
        if (own_tvar) {
            CHK(ensure(c, c->xdtv, (size_t)A * 8));
            tw = (double *)c->xdtv.p;
            tv = tw;
        }
        if (ssx || sst || tw) {
            hipLaunchKernelGGL(plsk::xdiag_finish_kernel, dim3((unsigned)((LP + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream,
                               (const double *)red, A, (double)(n_total - 1), ssx, sst, tw);
            LAUNCH_CHECK(c);
        }
    }
    if (T2 && N > 0) {
        hipLaunchKernelGGL(plsk::xdiag_t2_kernel, dim3((unsigned)((N + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream, Sd, ldsd, N, A, tv,
                           T2, ldt2);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

}  // namespace
