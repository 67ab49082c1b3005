// plan_vardiag.hpp -- variable-space diagnostics of a model on the device: scores, the column sweep for every component count, VIP.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

static_assert(plsk::VD_RANGE == XD_RANGE, "the column sweep takes the ranges of the row sweep");

template <typename T, int VEC, int CR>
int vardiag_launch_sweep_t(pls_hip_context *c, const plsk::VdGeom &g, const T *X, i64 ldx, i64 N, i64 K, const double *ST,
                           const double *P, int c_lo, int c_hi, double *part, i64 p_rs, i64 p_j) {
    const auto fn = plsk::vardiag_sweep_kernel<T, VEC, CR>;
    if (!plsk::raise_dynamic_lds((const void *)fn, (int)g.lds_bytes))
        return fail(c, PLS_HIP_ERR_DEVICE, "var_diagnostics: the device refuses the tile's LDS");
    hipLaunchKernelGGL(fn, dim3((unsigned)(g.CB * g.RS)), dim3(plsk::WG), (size_t)g.lds_bytes, c->stream, X, ldx, N, K, g.NT, g.RS,
                       ST, g.AS, P, c_lo, c_hi, part, p_rs, p_j);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

template <typename T, int CR>
int vardiag_launch_sweep(pls_hip_context *c, const plsk::VdGeom &g, const T *X, i64 ldx, i64 N, i64 K, const double *ST, const double *P,
                         int c_lo, int c_hi, double *part, i64 p_rs, i64 p_j) {
    if (g.vec > 1) return vardiag_launch_sweep_t<T, 16 / sizeof(T), CR>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j);
    return vardiag_launch_sweep_t<T, 1, CR>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j);
}

// All pointers are device memory.  Any of ssxk, VIP, sst may be null; tt null = VIP takes this call's sst.  X is read only when
// need_x = ssxk || sst || (VIP && !tt); exactly then a handle with a reducer sends one message of RED_SLICES * (A [+ K (A + 1)
// with ssxk]) values.
template <typename T>
int vardiag_device(pls_hip_context *c, const T *X, i64 ldx, i64 N, i64 K, i64 M, int A, const double *W, const double *R,
                   const double *P, const double *Q, const double *tt, double *ssxk, i64 ldk, double *VIP, i64 ldv, double *sst) {
    const bool need_x = ssxk || sst || (VIP && !tt);
    const bool need_sst = sst || (VIP && !tt);
    const dim3 blk(plsk::WG);
    const double *tau = tt;
    if (need_x) {
        const bool aligned = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), 16 / sizeof(T));
        const plsk::VdGeom g = plsk::vardiag_geom_of(N, K, A, (int)sizeof(T), c->num_cu, aligned, ssxk != nullptr);
        const i64 L = g.msg_values;
        CHK(ensure(c, c->vdred, (size_t)plsk::RED_SLICES * L * 8));
        double *red = (double *)c->vdred.p;
        HIPCHK(c, hipMemsetAsync(red, 0, (size_t)plsk::RED_SLICES * L * 8, c->stream));
        if (N > 0) {
            const double *Sd = nullptr;
            i64 ldsd = 0;
            CHK(xdiag_scores<T>(c, X, ldx, N, (int)K, A, R, (T *)nullptr, 0, &Sd, &ldsd));
            if (need_sst) {  // column sums of squares of the scores
                const int G = (int)std::min<i64>((N + plsk::WG - 1) / plsk::WG, 4 * (i64)c->num_cu);
                for (int c_lo = 0; c_lo < A; c_lo += 1024) {
                    const int c_hi = std::min(A, c_lo + 1024), nc = c_hi - c_lo;
                    CHK(ensure(c, c->part, (size_t)G * nc * 8));
                    hipLaunchKernelGGL(plsk::xdiag_score_stats_kernel<true>, dim3(G), blk, (size_t)(plsk::WG / plsk::WAVE) * nc * 8, c->stream,
                                       Sd, ldsd, N, c_lo, c_hi, (float *)nullptr, (i64)0, (double *)c->part.p);
                    LAUNCH_CHECK(c);
                    CHK(launch_reduce(c, (const double *)c->part.p, G, nc, nullptr, 0, red + c_lo, L));
                }
            }
            if (ssxk) {  // the column sweep: VD_RANGE component counts at a time
                CHK(ensure(c, c->vdST, (size_t)g.st_bytes));
                CHK(ensure(c, c->vdpart, (size_t)g.part_bytes));
                double *ST = (double *)c->vdST.p, *part = (double *)c->vdpart.p;
                const i64 rows = g.NT * plsk::VD_TR;
                hipLaunchKernelGGL(plsk::vardiag_rows_kernel, dim3((unsigned)((rows + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream, Sd, ldsd,
                                   N, A, g.AS, rows, ST);
                LAUNCH_CHECK(c);
                for (int j = 0; j < g.nranges; ++j) {
                    const int c_lo = plsk::vd_range_lo(j), c_hi = plsk::vd_range_hi(j, A), nc = c_hi - c_lo;
                    const int first = c_lo == 0 ? 1 : 0, Lr = nc + first;
                    const i64 p_rs = g.p_one_launch ? (i64)Lr * K : K, p_j = g.p_one_launch ? K : (i64)g.RS * K;
                    {
                        Scope s(c, PLS_HIP_FAM_XB, (i64)N * K * sizeof(T) + (i64)N * c_hi * 8 + (i64)K * c_hi * 8);
                        switch (plsk::vd_cr(nc)) {
                            case 4: CHK((vardiag_launch_sweep<T, 4>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                            case 8: CHK((vardiag_launch_sweep<T, 8>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                            case 12: CHK((vardiag_launch_sweep<T, 12>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                            case 16: CHK((vardiag_launch_sweep<T, 16>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                            case 20: CHK((vardiag_launch_sweep<T, 20>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                            default: CHK((vardiag_launch_sweep<T, plsk::VD_RANGE>(c, g, X, ldx, N, K, ST, P, c_lo, c_hi, part, p_rs, p_j))); break;
                        }
                    }
                    // the row splits in split order, into the planes [first ? 0 : 1 + c_lo, + Lr) of ssxk
                    double *dst = red + A + (i64)(first ? 0 : 1 + c_lo) * K;
                    if (g.p_one_launch) {
                        CHK(launch_reduce(c, part, g.RS, (int)(Lr * K), nullptr, 0, dst, L));
                    } else {
                        for (int jj = 0; jj < Lr; ++jj) CHK(launch_reduce(c, part + jj * p_j, g.RS, (int)K, nullptr, 0, dst + jj * K, L));
                    }
                }
            }
        }
        CHK(do_allreduce(c, red, (i64)plsk::RED_SLICES * L));
        double *sst_to = sst;
        if (!sst && VIP && !tt) {
            CHK(ensure(c, c->vdsm, (size_t)3 * A * 8));
            sst_to = (double *)c->vdsm.p + 2 * (i64)A;
        }
        if (VIP && !tt) tau = sst_to;
        hipLaunchKernelGGL(plsk::vardiag_finish_kernel, dim3((unsigned)((L + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream,
                           (const double *)red, L, A, K, sst_to, ssxk, ldk);
        LAUNCH_CHECK(c);
    }
    if (VIP) {  // vdsm = [||w_a||^2 (A) | ssy_a (A) | sst of this call when nobody asked for it (A)]
        CHK(ensure(c, c->vdsm, (size_t)3 * A * 8));
        double *pre = (double *)c->vdsm.p;
        hipLaunchKernelGGL(plsk::vardiag_vip_prep_kernel, dim3((unsigned)A), blk, 0, c->stream, W, K, Q, M, tau, A, pre);
        LAUNCH_CHECK(c);
        hipLaunchKernelGGL(plsk::vardiag_vip_kernel, dim3((unsigned)((K + plsk::WG - 1) / plsk::WG)), blk, 0, c->stream, W, K, A,
                           (const double *)pre, VIP, ldv);
        LAUNCH_CHECK(c);
    }
    return PLS_HIP_OK;
}

}  // namespace
