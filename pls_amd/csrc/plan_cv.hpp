// plan_cv.hpp -- cross-validation folds (src/pls.cpp:469-549): all folds in one launch, the single-launch fold kernels, one refit per fold.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// device part of pls_hip_cv_folds on storage type T (X, Y device pointers; E device pointer)
template <typename T>
int cv_folds_device(pls_hip_context *h, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, int Ki, int Mi, int Ai,
                    const int64_t *test_idx, int ts, i64 num_folds, double *dE) {
    const i64 nobs = num_folds * ts;
    const i64 K = Ki, M = Mi, A = Ai;
    const plsk::CvLayout L(Ki, Mi, Ai, ts);
    CHK(ensure(h, h->xx, (size_t)K * K * 8));
    CHK(ensure(h, h->xy, (size_t)K * M * 8));
    CHK(ensure(h, h->cvidx, (size_t)nobs * 8));
    CHK(ensure(h, h->cvx, (size_t)nobs * K * 8));
    CHK(ensure(h, h->cvy, (size_t)nobs * M * 8));
    CHK(ensure(h, h->cvws, (size_t)num_folds * (size_t)L.total * 8));
    double *XX = (double *)h->xx.p, *XYd = (double *)h->xy.p;
    // XX and XY of the whole matrix, once (or taken from the upload that already formed them)
    if (h->pre_xx && h->pre_xy) {
        HIPCHK(h, hipMemcpyAsync(XX, h->pre_xx, (size_t)K * K * 8, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(XYd, h->pre_xy, (size_t)K * M * 8, hipMemcpyDeviceToDevice, h->stream));
    } else {
        CHK(compute_xx<T>(h, dX, dldx, N, Ki, XX));
    }
    if (!(h->pre_xx && h->pre_xy)) {
        CHK(ensure(h, h->part, (size_t)max_partial_rows(h, N, Ki) * (size_t)(K * M) * 8));
        CHK(ensure(h, h->red, (size_t)plsk::RED_SLICES * std::max<i64>(K * M, K + 1) * 8));
        int nb = 0;
        CHK(launch_xty<T>(h, dX, dldx, dY, dldy, N, Ki, Mi, (double *)h->part.p, &nb));
        CHK(launch_reduce(h, (const double *)h->part.p, nb, Ki * Mi, nullptr, 0, (double *)h->red.p));
        hipLaunchKernelGGL(plsk::sum_slices_kernel, dim3((Ki * Mi + plsk::WG - 1) / plsk::WG), dim3(plsk::WG), 0,
                           h->stream, (const double *)h->red.p, Ki * Mi, XYd);
        LAUNCH_CHECK(h);
    }
    HIPCHK(h, hipMemcpyAsync(h->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL((plsk::cv_gather_kernel<T>), dim3((unsigned)nobs), dim3(plsk::WG), 0, h->stream, dX, dldx, dY,
                       dldy, Ki, Mi, (const i64 *)h->cvidx.p, (double *)h->cvx.p, (double *)h->cvy.p);
    LAUNCH_CHECK(h);
    {
        Scope s(h, PLS_HIP_FAM_SMALL, (i64)num_folds * A * ((i64)K * K + 4 * K) * 8);
        hipLaunchKernelGGL(plsk::cv_folds_kernel, dim3((unsigned)num_folds), dim3(plsk::UPD_THREADS), (size_t)A * 8,
                           h->stream, (const double *)XX, (const double *)XYd, (const double *)h->cvx.p,
                           (const double *)h->cvy.p, Ki, Mi, Ai, ts, (double *)h->cvws.p, dE, (int)h->opt_power_iters, 0, nobs);
        LAUNCH_CHECK(h);
    }
    return PLS_HIP_OK;
}

// Small data (the reference's examples): every fold is a single-launch fit (tiny_kernels.hpp) on the whole X with its held-out
// rows masked, one workgroup -- for the smallest data (N <= 64, K <= 32) one WAVE -- per fold: no X^T X at all, which for N < K
// is the smaller object anyway.  kind: the kernel pls_hip_cv_folds chose.
enum class FoldKernel { micro, tiny, tiny_m };  // micro_fit_kernel; tiny_fit_kernel (one response); tiny_fit_m_kernel (2..8)
template <typename T>
int cv_folds_single_launch(pls_hip_context *h, FoldKernel kind, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, int Ki, int Mi,
                           int Ai, const int64_t *test_idx, int ts, i64 num_folds, double *dE) {
    const i64 nobs = num_folds * ts;
    CHK(ensure(h, h->cvidx, (size_t)nobs * 8));
    HIPCHK(h, hipMemcpyAsync(h->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    const i64 *idx = (const i64 *)h->cvidx.p;
    const dim3 grid((unsigned)num_folds);
    const size_t lds = kind == FoldKernel::micro ? 0 : plsk::single_fit_lds_bytes(Ki, Mi, Ai);  // (one wave: static LDS only)
    const int pit = (int)h->opt_power_iters;
    double *const none = nullptr;  // fold mode writes E only
    Scope s(h, PLS_HIP_FAM_SMALL, (i64)num_folds * N * Ki * (i64)sizeof(T));
    if (kind == FoldKernel::micro) {
        with_mm(Mi, [&](auto mm) {
            hipLaunchKernelGGL((plsk::micro_fit_kernel<T, decltype(mm)::value>), grid, dim3(plsk::WAVE), lds, h->stream, dX, dldx, dY, dldy, (int)N,
                               Ki, Mi, Ai, pit, none, none, none, none, (T *)nullptr, (i64)0, none, idx, ts, nobs, dE);
        });
    } else if (kind == FoldKernel::tiny) {
        if (!plsk::raise_dynamic_lds((const void *)plsk::tiny_fit_kernel<T>, (int)plsk::TINY_LDS_MAX)  /* raised once per device: to the most any fit asks for */)
            return fail(h, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the single-launch fit could not be raised");
        hipLaunchKernelGGL((plsk::tiny_fit_kernel<T>), grid, dim3(plsk::UPD_THREADS), lds, h->stream, dX, dldx, dY, (int)N, Ki, Ai, none, none,
                           none, none, (T *)nullptr, (i64)0, none, idx, ts, nobs, dE);
    } else {
        CHK(with_mm(Mi, [&](auto mm) {
            constexpr int MM = decltype(mm)::value;
            if (!plsk::raise_dynamic_lds((const void *)plsk::tiny_fit_m_kernel<T, MM>, (int)plsk::TINY_LDS_MAX))
                return fail(h, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the single-launch fit could not be raised");
            hipLaunchKernelGGL((plsk::tiny_fit_m_kernel<T, MM>), grid, dim3(plsk::UPD_THREADS), lds, h->stream, dX, dldx, dY, dldy, (int)N, Ki,
                               Mi, Ai, pit, none, none, none, none, (T *)nullptr, (i64)0, none, idx, ts, nobs, dE);
            return (int)PLS_HIP_OK;
        }));
    }
    LAUNCH_CHECK(h);
    return PLS_HIP_OK;
}

// The general form of the same call: one refit per fold on the rows that are not in its test set -- what the reference
// does (src/pls.cpp:478-488, :524-545), with the training rows gathered on the device and the fit running under the
// handle's own plan.  Serves the shapes the batched kernel declines (M > 32, A > 4096, K > 16384, a workspace that does
// not fit); costs num_folds fits.
template <typename T>
int cv_folds_refit(pls_hip_context *h, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, int Ki, int Mi, int Ai,
                   const int64_t *test_idx, int ts, i64 num_folds, double *dE) {
    const i64 nobs = num_folds * ts;
    const i64 K = Ki, M = Mi, A = Ai;
    const i64 ldtr = (N + 3) & ~(i64)3;
    CHK(ensure(h, h->cvidx, (size_t)nobs * 8));
    CHK(ensure(h, h->cvx, (size_t)nobs * K * 8));
    CHK(ensure(h, h->cvy, (size_t)nobs * M * 8));
    CHK(ensure(h, h->cvkeep, (size_t)N * 8));
    CHK(ensure(h, h->cvtx, (size_t)ldtr * K * sizeof(T)));
    CHK(ensure(h, h->cvty, (size_t)ldtr * M * sizeof(T)));
    CHK(ensure(h, h->cvtt, (size_t)ldtr * A * sizeof(T)));
    CHK(ensure(h, h->cvm, (size_t)(3 * K * A + M * A + (i64)ts * A) * 8));
    double *Wf = (double *)h->cvm.p, *Pf = Wf + K * A, *Rf = Pf + K * A, *Qf = Rf + K * A, *us = Qf + M * A;
    HIPCHK(h, hipMemcpyAsync(h->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL((plsk::cv_gather_kernel<T>), dim3((unsigned)nobs), dim3(plsk::WG), 0, h->stream, dX, dldx, dY,
                       dldy, Ki, Mi, (const i64 *)h->cvidx.p, (double *)h->cvx.p, (double *)h->cvy.p);
    LAUNCH_CHECK(h);
    const double *saved_xx = h->pre_xx, *saved_xy = h->pre_xy;  // products of ALL rows: not a fold's
    h->pre_xx = h->pre_xy = nullptr;
    // folds whose fit (N - ts training rows) the sample-space plan would refuse (plan_dual.hpp: dual_refusal) are fitted under
    // the default plan
    const i64 saved_algo = h->opt_algo;
    if (saved_algo == PLS_HIP_ALGO_DUAL && dual_refusal(h, N - ts, M)) h->opt_algo = PLS_HIP_ALGO_KERNEL;
    std::vector<char> held(N, 0);
    std::vector<int64_t> keep(N);
    int rc = PLS_HIP_OK;
    for (i64 f = 0; f < num_folds && rc == PLS_HIP_OK; ++f) {
        for (int i = 0; i < ts; ++i) held[test_idx[f * ts + i]] = 1;
        i64 ntr = 0;
        for (i64 r = 0; r < N; ++r)
            if (!held[r]) keep[ntr++] = r;
        for (int i = 0; i < ts; ++i) held[test_idx[f * ts + i]] = 0;
        if (ntr < 1 || A > K) { rc = fail(h, PLS_HIP_ERR_INVALID, "cv_folds: a fold leaves no training rows"); break; }
        if (hipMemcpyAsync(h->cvkeep.p, keep.data(), (size_t)ntr * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rc = fail(h, PLS_HIP_ERR_DEVICE, "cv_folds: upload of the training row list failed");
            break;
        }
        const unsigned gx = (unsigned)((ntr + plsk::WG - 1) / plsk::WG);
        hipLaunchKernelGGL((plsk::gather_rows_kernel<T>), dim3(gx, (unsigned)std::min<i64>(K, 1024)), dim3(plsk::WG), 0, h->stream,
                           dX, dldx, (const i64 *)h->cvkeep.p, ntr, Ki, (T *)h->cvtx.p, ldtr);
        hipLaunchKernelGGL((plsk::gather_rows_kernel<T>), dim3(gx, (unsigned)std::min<i64>(M, 1024)), dim3(plsk::WG), 0, h->stream,
                           dY, dldy, (const i64 *)h->cvkeep.p, ntr, Mi, (T *)h->cvty.p, ldtr);
        rc = fit_device<T>(h, (const T *)h->cvtx.p, ldtr, (const T *)h->cvty.p, ldtr, ntr, Ki, Mi, Ai, PLS_HIP_KERNEL_TYPE1,
                           Wf, Pf, Qf, Rf, (T *)h->cvtt.p, ldtr, nullptr);
        if (rc != PLS_HIP_OK) break;
        hipLaunchKernelGGL(plsk::cv_refit_residuals_kernel, dim3((unsigned)ts), dim3(plsk::WG), 0, h->stream,
                           (const double *)h->cvx.p + f * ts * K, (const double *)h->cvy.p + f * ts * M, (const double *)Rf,
                           (const double *)Qf, Ki, Mi, Ai, ts, f, nobs, us, dE);
        // `keep` is rewritten for the next fold: its copy must have been consumed
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            rc = fail(h, PLS_HIP_ERR_DEVICE, "cv_folds: a fold's refit failed on the device");
    }
    h->pre_xx = saved_xx;
    h->pre_xy = saved_xy;
    h->opt_algo = saved_algo;
    return rc;
}

// the batched kernel's shapes (cv_kernels.hpp): everything M-sized in one workgroup's LDS, X^T X resident
bool cv_batched_covers(const pls_hip_context *c, i64 K, i64 M, i64 A) {
    return !c->env.cv_refit && A <= 4096 && K <= 16384 && (M == 1 || M <= plsk::MMAX);
}

// ---- row-sharded handles (a reducer installed): pls_hip_cv_folds as a collective (include/pls_hip.h) ----
// The messages, in order: the partition (RED_SLICES * nranks values); on the batched route X^T X (8*K*K) and X^T Y (8*K*M) of
// all rows; the held-out rows of every fold, in messages of whole folds; then E (batched route, in pieces) or, on the refit
// route, the collectives of one sharded fit per fold.  Every message but X^T X / X^T Y has exactly ONE non-zero term per value
// over ranks and slices, so its sum is exact whatever the order of the reducer's additions: E is bit-identical on every rank.
constexpr i64 CV_MSG_CAP = (i64)1 << 20;  // values per slice of a held-out-rows or E message (8 MiB; 64 MiB with its slices)

// h->cvidx (the GLOBAL rows of every fold's test set) -> their x and y rows in h->cvx / h->cvy, on every rank
template <typename T>
int cv_share_test_rows(pls_hip_context *h, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, i64 row0, int Ki, int Mi,
                       int ts, i64 num_folds, i64 fchunk) {
    const i64 KM = (i64)Ki + Mi;
    double *red = (double *)h->cvred.p;
    for (i64 f0 = 0; f0 < num_folds; f0 += fchunk) {
        const i64 nrow = std::min(fchunk, num_folds - f0) * ts, L = nrow * KM;
        hipLaunchKernelGGL((plsk::cv_pack_test_rows_kernel<T>), dim3((unsigned)nrow), dim3(plsk::WG), 0, h->stream, dX, dldx, dY,
                           dldy, Ki, Mi, (const i64 *)h->cvidx.p + f0 * ts, row0, N, red, L);
        LAUNCH_CHECK(h);
        CHK(do_allreduce(h, red, (i64)plsk::RED_SLICES * L));
        const unsigned g = (unsigned)std::min<i64>((L + plsk::WG - 1) / plsk::WG, 4096);
        hipLaunchKernelGGL(plsk::cv_unpack_test_rows_kernel, dim3(g), dim3(plsk::WG), 0, h->stream, (const double *)red, L, Ki, Mi,
                           (double *)h->cvx.p + f0 * ts * Ki, (double *)h->cvy.p + f0 * ts * Mi);
        LAUNCH_CHECK(h);
    }
    return PLS_HIP_OK;
}

// Batched route: X^T X and X^T Y summed over the ranks (what a sharded KERNEL_TYPE2 fit sends), this rank's contiguous range
// of folds [fold0, fold0 + nfold) in one launch of cv_folds_kernel into a zeroed E, E summed over the ranks.
template <typename T>
int cv_folds_sharded_batched(pls_hip_context *h, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, i64 row0, int Ki, int Mi,
                             int Ai, int ts, i64 num_folds, int fold0, int nfold, i64 fchunk, double *dE) {
    const i64 nobs = num_folds * ts;
    const i64 K = Ki, M = Mi, A = Ai;
    double *XX = (double *)h->xx.p, *XYd = (double *)h->xy.p, *red = (double *)h->red.p;
    CHK(compute_xx<T>(h, dX, dldx, N, Ki, XX));  // (an empty shard contributes zero slices)
    if (N > 0) {
        CHK(ensure(h, h->part, (size_t)max_partial_rows(h, N, Ki) * (size_t)(K * M) * 8));
        int nb = 0;
        CHK(launch_xty<T>(h, dX, dldx, dY, dldy, N, Ki, Mi, (double *)h->part.p, &nb));
        CHK(launch_reduce(h, (const double *)h->part.p, nb, Ki * Mi, nullptr, 0, red));
    } else {
        HIPCHK(h, hipMemsetAsync(red, 0, (size_t)plsk::RED_SLICES * K * M * 8, h->stream));
    }
    CHK(do_allreduce(h, red, (i64)plsk::RED_SLICES * K * M));
    hipLaunchKernelGGL(plsk::sum_slices_kernel, dim3((Ki * Mi + plsk::WG - 1) / plsk::WG), dim3(plsk::WG), 0, h->stream,
                       (const double *)red, Ki * Mi, XYd);
    LAUNCH_CHECK(h);
    CHK(cv_share_test_rows<T>(h, dX, dldx, dY, dldy, N, row0, Ki, Mi, ts, num_folds, fchunk));
    const i64 ne = nobs * A * M;
    HIPCHK(h, hipMemsetAsync(dE, 0, (size_t)ne * 8, h->stream));
    if (nfold > 0) {
        Scope s(h, PLS_HIP_FAM_SMALL, (i64)nfold * A * ((i64)K * K + 4 * K) * 8);
        hipLaunchKernelGGL(plsk::cv_folds_kernel, dim3((unsigned)nfold), dim3(plsk::UPD_THREADS), (size_t)A * 8, h->stream,
                           (const double *)XX, (const double *)XYd, (const double *)h->cvx.p, (const double *)h->cvy.p, Ki, Mi,
                           Ai, ts, (double *)h->cvws.p, dE, (int)h->opt_power_iters, fold0, nobs);
        LAUNCH_CHECK(h);
    }
    double *cr = (double *)h->cvred.p;
    for (i64 o = 0; o < ne; o += CV_MSG_CAP) {  // each entry of E has exactly one producer
        const int len = (int)std::min(CV_MSG_CAP, ne - o);
        const dim3 g((unsigned)((len + plsk::WG - 1) / plsk::WG));
        hipLaunchKernelGGL(plsk::fill_slices_kernel, g, dim3(plsk::WG), 0, h->stream, (const double *)dE + o, len, cr);
        LAUNCH_CHECK(h);
        CHK(do_allreduce(h, cr, (i64)plsk::RED_SLICES * len));
        hipLaunchKernelGGL(plsk::sum_slices_kernel, g, dim3(plsk::WG), 0, h->stream, (const double *)cr, len, dE + o);
        LAUNCH_CHECK(h);
    }
    return PLS_HIP_OK;
}

// Refit route: per fold, every rank gathers ITS rows outside the fold's test set (possibly none) and takes part in one sharded
// fit on them; the residuals of the held-out rows (on every rank) under that fit's R, Q (identical on every rank) need no message.
template <typename T>
int cv_folds_sharded_refit(pls_hip_context *h, const T *dX, i64 dldx, const T *dY, i64 dldy, i64 N, i64 row0, int Ki, int Mi,
                           int Ai, const int64_t *test_idx, int ts, i64 num_folds, i64 fchunk, double *dE) {
    const i64 nobs = num_folds * ts;
    const i64 K = Ki, M = Mi, A = Ai;
    const i64 ldtr = std::max<i64>(4, (N + 3) & ~(i64)3);
    double *Wf = (double *)h->cvm.p, *Pf = Wf + K * A, *Rf = Pf + K * A, *Qf = Rf + K * A, *us = Qf + M * A;
    CHK(cv_share_test_rows<T>(h, dX, dldx, dY, dldy, N, row0, Ki, Mi, ts, num_folds, fchunk));
    const double *saved_xx = h->pre_xx, *saved_xy = h->pre_xy;
    h->pre_xx = h->pre_xy = nullptr;
    std::vector<char> held(std::max<i64>(N, 1), 0);
    std::vector<int64_t> keep(std::max<i64>(N, 1));
    int rc = PLS_HIP_OK;
    for (i64 f = 0; f < num_folds && rc == PLS_HIP_OK; ++f) {
        for (int i = 0; i < ts; ++i) {
            const i64 r = test_idx[f * ts + i] - row0;
            if (r >= 0 && r < N) held[r] = 1;
        }
        i64 ntr = 0;
        for (i64 r = 0; r < N; ++r)
            if (!held[r]) keep[ntr++] = r;
        for (i64 r = 0; r < N; ++r) held[r] = 0;
        if (ntr > 0) {
            if (hipMemcpyAsync(h->cvkeep.p, keep.data(), (size_t)ntr * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
                rc = fail(h, PLS_HIP_ERR_DEVICE, "cv_folds: upload of the training row list failed");
                break;
            }
            const unsigned gx = (unsigned)((ntr + plsk::WG - 1) / plsk::WG);
            hipLaunchKernelGGL((plsk::gather_rows_kernel<T>), dim3(gx, (unsigned)std::min<i64>(K, 1024)), dim3(plsk::WG), 0, h->stream,
                               dX, dldx, (const i64 *)h->cvkeep.p, ntr, Ki, (T *)h->cvtx.p, ldtr);
            hipLaunchKernelGGL((plsk::gather_rows_kernel<T>), dim3(gx, (unsigned)std::min<i64>(M, 1024)), dim3(plsk::WG), 0, h->stream,
                               dY, dldy, (const i64 *)h->cvkeep.p, ntr, Mi, (T *)h->cvty.p, ldtr);
        }
        rc = fit_device<T>(h, (const T *)h->cvtx.p, ldtr, (const T *)h->cvty.p, ldtr, ntr, Ki, Mi, Ai, PLS_HIP_KERNEL_TYPE1,
                           Wf, Pf, Qf, Rf, (T *)h->cvtt.p, ldtr, nullptr);
        if (rc != PLS_HIP_OK) break;
        hipLaunchKernelGGL(plsk::cv_refit_residuals_kernel, dim3((unsigned)ts), dim3(plsk::WG), 0, h->stream,
                           (const double *)h->cvx.p + f * ts * K, (const double *)h->cvy.p + f * ts * M, (const double *)Rf,
                           (const double *)Qf, Ki, Mi, Ai, ts, f, nobs, us, dE);
        // `keep` is rewritten for the next fold: its copy must have been consumed
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
            rc = fail(h, PLS_HIP_ERR_DEVICE, "cv_folds: a fold's refit failed on the device");
    }
    h->pre_xx = saved_xx;
    h->pre_xy = saved_xy;
    return rc;
}

// The partition: one message of RED_SLICES * nranks values, this rank's row count in slot `rank` of slice 0 -- or -1 when this
// rank could not prepare its part of the call, which every rank then learns before any collective that would need it.
int cv_partition(pls_hip_context *h, i64 N, bool ready, i64 *row0, i64 *n_total, bool *all_ready) {
    const int n = h->nranks;
    CHK(ensure(h, h->guard, (size_t)plsk::RED_SLICES * std::max(n, 8) * 8));
    double *g = (double *)h->guard.p;
    hipLaunchKernelGGL(plsk::cv_slot_kernel, dim3(1), dim3(plsk::WG), 0, h->stream, g, n, h->rank, ready ? (double)N : -1.0);
    LAUNCH_CHECK(h);
    CHK(do_allreduce(h, g, (i64)plsk::RED_SLICES * n));
    std::vector<double> v((size_t)plsk::RED_SLICES * n);
    HIPCHK(h, hipMemcpyAsync(v.data(), g, v.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *row0 = *n_total = 0;
    *all_ready = true;
    for (int r = 0; r < n; ++r) {
        double s = 0.0;
        for (int i = 0; i < plsk::RED_SLICES; ++i) s += v[(size_t)i * n + r];
        if (!(s >= 0.0)) { *all_ready = false; continue; }
        if (r < h->rank) *row0 += (i64)s;
        *n_total += (i64)s;
    }
    return PLS_HIP_OK;
}

// pls_hip_cv_folds on a handle with a reducer: local checks done by the caller; X, Y are this rank's N rows (N may be 0)
int cv_folds_sharded(pls_hip_context *h, const void *X, i64 ldx, const void *Y, i64 ldy, i64 N, i64 K, i64 M, i64 A,
                     const int64_t *test_idx, i64 ts, i64 num_folds, int dtype, int mem, double *E) {
    const i64 nobs = num_folds * ts;
    const size_t es = esize(dtype);
    const bool batched = cv_batched_covers(h, K, M, A);  // (the env switch PLS_HIP_CV_REFIT must be the same on every rank)
    const int fold0 = (int)(num_folds * h->rank / h->nranks), nfold = (int)(num_folds * (h->rank + 1) / h->nranks) - fold0;
    const i64 fchunk = std::max<i64>(1, std::min<i64>(num_folds, CV_MSG_CAP / (ts * (K + M))));
    const i64 echunk = batched ? std::min<i64>(CV_MSG_CAP, nobs * A * M) : 0;
    const void *dX = X, *dY = Y;
    double *dE = E;
    i64 dldx = ldx, dldy = ldy;
    HostCall hc(h, mem);
    // Phase 1, local: stage host data and size every workspace of the call.  A failure is carried by the partition message,
    // so that no rank is left waiting in a collective its peers never reach.
    const int local = [&]() -> int {
        const i64 ldn = ld_quad(N);
        CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
        CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
        CHK(hc.out_flat(dE, E, h->cve, (size_t)nobs * A * M * 8));
        CHK(ensure(h, h->cvidx, (size_t)nobs * 8));
        CHK(ensure(h, h->cvx, (size_t)nobs * K * 8));
        CHK(ensure(h, h->cvy, (size_t)nobs * M * 8));
        CHK(ensure(h, h->cvred, (size_t)plsk::RED_SLICES * std::max(fchunk * ts * (K + M), echunk) * 8));
        if (batched) {
            const plsk::CvLayout L((int)K, (int)M, (int)A, (int)ts);
            CHK(ensure(h, h->xx, (size_t)K * K * 8));
            CHK(ensure(h, h->xy, (size_t)K * M * 8));
            CHK(ensure(h, h->red, (size_t)plsk::RED_SLICES * std::max<i64>(K * M, K + 1) * 8));
            CHK(ensure(h, h->red2, (size_t)plsk::RED_SLICES * K * K * 8));
            CHK(ensure(h, h->cvws, (size_t)std::max(nfold, 1) * (size_t)L.total * 8));
            if (N > 0) CHK(ensure(h, h->part, (size_t)max_partial_rows(h, N, (int)K) * (size_t)(K * M) * 8));
        } else {
            const i64 ldtr = std::max<i64>(4, (N + 3) & ~(i64)3);
            CHK(ensure(h, h->cvkeep, (size_t)std::max<i64>(N, 1) * 8));
            CHK(ensure(h, h->cvtx, (size_t)ldtr * K * es));
            CHK(ensure(h, h->cvty, (size_t)ldtr * M * es));
            CHK(ensure(h, h->cvtt, (size_t)ldtr * A * es));
            CHK(ensure(h, h->cvm, (size_t)(3 * K * A + M * A + ts * A) * 8));
        }
        return PLS_HIP_OK;
    }();
    i64 row0 = 0, n_total = 0;
    bool all_ready = false;
    CHK(cv_partition(h, N, local == PLS_HIP_OK, &row0, &n_total, &all_ready));
    if (local != PLS_HIP_OK) return local;
    if (!all_ready) return fail(h, PLS_HIP_ERR_ALLOC, "cv_folds: another rank could not prepare its part of the call");
    // Phase 2: the checks on global data -- every rank holds the same, so every rank reaches the same verdict
    if (n_total < 2) return fail(h, PLS_HIP_ERR_INVALID, "bad cv_folds arguments: fewer than 2 rows over all ranks");
    if (ts >= n_total)
        return fail(h, PLS_HIP_ERR_INVALID, "cv_folds: test_size >= n_total -- a fold would leave no training rows");
    CHK(check_test_idx(h, test_idx, nobs, n_total, "cv_folds"));
    HIPCHK(h, hipMemcpyAsync(h->cvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    const int Ki = (int)K, Mi = (int)M, Ai = (int)A, tsi = (int)ts;
    const int rc = by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (batched)
            return cv_folds_sharded_batched<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, row0, Ki, Mi, Ai, tsi, num_folds, fold0, nfold,
                                               fchunk, dE);
        return cv_folds_sharded_refit<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, row0, Ki, Mi, Ai, test_idx, tsi, num_folds, fchunk,
                                         dE);
    });
    if (rc != PLS_HIP_OK) return rc;
    return hc.finish(true, true);  // (the replica guard of the refit route's fits; a timed-out device-side exchange)
}

}  // namespace
