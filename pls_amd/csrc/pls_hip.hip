// pls_hip.hip -- the C-ABI of include/pls_hip.h over the gfx950 kernels in this directory.
// Host side of the library: argument checks, workspace, launch geometry, the A-loop of
// Model::plsr (src/pls.cpp:390-437) enqueued on one HIP stream with no host round trip,
// the injected all-reduce for row-sharded fits, HIP-event profiling.
#include <dlfcn.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pls_hip.h"
#include "fused_kernels.hpp"
#include "defer_kernels.hpp"
#include "small_kernels.hpp"
#include "coop_update.hpp"
#include "wide1_update.hpp"
#include "largem_kernels.hpp"
#include "tiny_kernels.hpp"
#include "resident_kernels.hpp"
#include "resident_gram.hpp"
#include "stream_kernels.hpp"
#include "xb_mfma4.hpp"
#include "xb_mfma4w.hpp"
#include "syrk_kernels.hpp"
#include "cv_kernels.hpp"
#include "validation_kernels.hpp"
#include "xdiag_kernels.hpp"
#include "vardiag_kernels.hpp"
#include "batch_kernels.hpp"
#include "dual_kernels.hpp"
#include "dual_cv_kernels.hpp"
#include "dual_batch_kernels.hpp"
#include "dual_cvbatch_kernels.hpp"
#include "resample_kernels.hpp"
#include "synth_kernels.hpp"
#include "missing_kernels.hpp"
#include "missing_cv_kernels.hpp"
#include "xdiag_missing_kernels.hpp"
#include "host_pipeline.hpp"
#include "exchange_kernels.hpp"

using plsk::i64;

#include "ctx.hpp"
#include "xb_route.hpp"
#include "launch_products.hpp"
#include "plan_common.hpp"
#include "launch_update.hpp"
#include "plan_dual.hpp"
#include "plan_fit_single.hpp"
#include "plan_fit.hpp"
#include "host_entry.hpp"
#include "fit_graph.hpp"
#include "plan_validation.hpp"
#include "plan_xdiag.hpp"
#include "plan_vardiag.hpp"
#include "plan_stats.hpp"
#include "plan_cv.hpp"
#include "dual_round.hpp"
#include "plan_dual_cv.hpp"
#include "plan_dual_batch.hpp"
#include "plan_batch.hpp"
#include "plan_resample.hpp"
#include "plan_dual_cvbatch.hpp"
#include "plan_missing.hpp"
#include "plan_missing_cv.hpp"
#include "plan_xdiag_missing.hpp"
#include "xchg_ipc.hpp"
#include "group_impl.hpp"

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int pls_hip_abi_version(void) { return PLS_HIP_ABI_VERSION; }

#ifdef PLS_HIP_TESTING
// testing/libpls_hip.so only (not in include/pls_hip.h): 4 wall-clock stamps per workgroup of the fused passes that follow go
// to `buf` (device memory, 64 bytes per workgroup (4 stamps, XCC_ID, HW_ID); nullptr: off)
__attribute__((visibility("default"))) int pls_hip_test_set_pass_stamps(void *buf) {
    unsigned long long *p = (unsigned long long *)buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(plsk::g_pass_stamps), &p, sizeof(p)) == hipSuccess ? 0 : 1;
}
// out[4] = {descending, positions per edge, tiles, grid} of the last storing deflating pass that was launched
__attribute__((visibility("default"))) int pls_hip_test_last_turn(int *out) {
    if (!out) return 1;
    out[0] = plsk::g_test_turn.rev; out[1] = plsk::g_test_turn.edge; out[2] = plsk::g_test_turn.ntiles; out[3] = plsk::g_test_turn.grid;
    return 0;
}
// Fills every scratch workspace of the handle that is allocated (ctx.hpp, PLS_HIP_WORKSPACES; behind the leading bytes a stateful
// entry keeps) with `byte` and returns the number of bytes filled, -1 on an error.  also_new != 0: until a call with
// also_new == 0, ensure() fills every fresh allocation with `byte` as well.
__attribute__((visibility("default"))) long long pls_hip_test_poison_workspace(pls_hip_handle h, int byte, int also_new) {
    if (!h || hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    long long filled = 0;
    bool ok = true;
    for_each_workspace(h, [&](DevBuf &b, size_t keep) {
        if (!b.p || keep >= b.bytes) return;
        ok = ok && hipMemsetAsync((char *)b.p + keep, byte & 0xFF, b.bytes - keep, h->stream) == hipSuccess;
        filled += (long long)(b.bytes - keep);
    });
    h->poison_new = also_new ? (byte & 0xFF) : -1;
    return ok && hipStreamSynchronize(h->stream) == hipSuccess ? filled : -1;
}
#endif

int pls_hip_create(pls_hip_handle *out, int device, void *stream) {
    if (!out) return PLS_HIP_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return PLS_HIP_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PLS_HIP_ERR_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PLS_HIP_ERR_DEVICE;  // no other target
    pls_hip_context *c = new (std::nothrow) pls_hip_context();
    if (!c) return PLS_HIP_ERR_ALLOC;
    pls_hip_context::read_env(c->env);
    c->device = device;
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipSetDevice(device) != hipSuccess) { delete c; return PLS_HIP_ERR_DEVICE; }
    c->stream = (hipStream_t)stream;  // NULL = the device's default (null) stream
    *out = c;
    return PLS_HIP_OK;
}

int pls_hip_destroy(pls_hip_handle h) {
    if (!h) return PLS_HIP_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for_each_workspace(h, [](DevBuf &b, size_t) {  // (the one list of ctx.hpp)
        if (b.p) (void)hipFree(b.p);
    });
    for (void *q : h->graveyard) (void)hipFree(q);
    if (h->xchg) xchg_release(h);
    if (h->diverged) (void)hipHostFree(h->diverged);
    if (h->mconv_host) (void)hipHostFree(h->mconv_host);
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    h->stager.release();
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    delete h;
    return PLS_HIP_OK;
}

int pls_hip_set_stream(pls_hip_handle h, void *stream) {
    CHK(check_handle(h));
    CHK(set_device(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = (hipStream_t)stream;
    return PLS_HIP_OK;
}

int pls_hip_set_option(pls_hip_handle h, int option, int64_t value) {
    CHK(check_handle(h));
    switch (option) {
        case PLS_HIP_OPT_ALGO:
            if (value != PLS_HIP_ALGO_KERNEL && value != PLS_HIP_ALGO_NIPALS && value != PLS_HIP_ALGO_GRAM &&
                value != PLS_HIP_ALGO_AUTO && value != PLS_HIP_ALGO_DUAL)
                return fail(h, PLS_HIP_ERR_INVALID, "unknown algo");
            h->opt_algo = value;
            return PLS_HIP_OK;
        case PLS_HIP_OPT_FUSE: h->opt_fuse = value ? 1 : 0; return PLS_HIP_OK;
        case PLS_HIP_OPT_PROFILE: h->opt_profile = value < 0 ? 0 : (value > 2 ? 2 : value); return PLS_HIP_OK;
        case PLS_HIP_OPT_POWER_ITERS:
            if (value < 1 || value > 4096) return fail(h, PLS_HIP_ERR_INVALID, "power iters out of range");
            h->opt_power_iters = value;
            return PLS_HIP_OK;
        case PLS_HIP_OPT_FUSED_GRID:
            if (value < 0 || value > (1 << 20)) return fail(h, PLS_HIP_ERR_INVALID, "fused grid out of range");
            h->opt_fused_grid = value;
            return PLS_HIP_OK;
        case PLS_HIP_OPT_WORK_LAYOUT: h->opt_work_layout = value ? 1 : 0; return PLS_HIP_OK;
        case PLS_HIP_OPT_DEFER:
            if (value < 1 || value > plsk::DEFER_MAX) return fail(h, PLS_HIP_ERR_INVALID, "defer out of range");
            h->opt_defer = value;
            return PLS_HIP_OK;
        case PLS_HIP_OPT_GRAPH: h->opt_graph = value ? 1 : 0; return PLS_HIP_OK;
        case PLS_HIP_OPT_VALIDATION_LDS_ROWS:
            if (value < 0 || value > val_lds_rows_device(h)) return fail(h, PLS_HIP_ERR_INVALID, "validation LDS rows out of range");
            h->opt_val_lds_rows = value;
            return PLS_HIP_OK;
        case PLS_HIP_OPT_MISSING_ITERS:
            if (value < 1 || value > (1 << 20)) return fail(h, PLS_HIP_ERR_INVALID, "missing iters out of range");
            h->opt_missing_iters = value;
            return PLS_HIP_OK;
        default: return fail(h, PLS_HIP_ERR_INVALID, "unknown option");
    }
}

int pls_hip_get_option(pls_hip_handle h, int option, int64_t *value) {
    CHK(check_handle(h));
    if (!value) return PLS_HIP_ERR_INVALID;
    switch (option) {
        case PLS_HIP_OPT_ALGO: *value = h->opt_algo; return PLS_HIP_OK;
        case PLS_HIP_OPT_FUSE: *value = h->opt_fuse; return PLS_HIP_OK;
        case PLS_HIP_OPT_PROFILE: *value = h->opt_profile; return PLS_HIP_OK;
        case PLS_HIP_OPT_POWER_ITERS: *value = h->opt_power_iters; return PLS_HIP_OK;
        case PLS_HIP_OPT_FUSED_GRID: *value = h->opt_fused_grid; return PLS_HIP_OK;
        case PLS_HIP_OPT_GRAPH: *value = h->opt_graph; return PLS_HIP_OK;
        case PLS_HIP_OPT_WORK_LAYOUT: *value = h->opt_work_layout; return PLS_HIP_OK;
        case PLS_HIP_OPT_DEFER: *value = h->opt_defer; return PLS_HIP_OK;
        case PLS_HIP_OPT_VALIDATION_LDS_ROWS: *value = h->opt_val_lds_rows >= 0 ? h->opt_val_lds_rows : val_lds_rows_device(h); return PLS_HIP_OK;
        case PLS_HIP_OPT_MISSING_ITERS: *value = h->opt_missing_iters; return PLS_HIP_OK;
        default: return fail(h, PLS_HIP_ERR_INVALID, "unknown option");
    }
}

int pls_hip_set_reducer(pls_hip_handle h, pls_hip_allreduce_fn fn, void *user, int rank, int nranks) {
    CHK(check_handle(h));
    if (nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !fn))
        return fail(h, PLS_HIP_ERR_INVALID, "bad reducer arguments");
    h->reducer = fn;
    h->reducer_user = user;
    h->rank = rank;
    h->nranks = nranks;
    return PLS_HIP_OK;
}

int pls_hip_get_reducer(pls_hip_handle h, int *installed, int *rank, int *nranks) {
    CHK(check_handle(h));
    if (installed) *installed = h->reducer ? 1 : 0;
    if (rank) *rank = h->rank;
    if (nranks) *nranks = h->nranks;
    return PLS_HIP_OK;
}

int pls_hip_set_reduce_buffer(pls_hip_handle h, void *buf, int64_t count) {
    CHK(check_handle(h));
    if ((buf && count <= 0) || (!buf && count != 0)) return fail(h, PLS_HIP_ERR_INVALID, "bad reduce buffer");
    h->user_red = (double *)buf;
    h->user_red_count = count;
    return PLS_HIP_OK;
}

int pls_hip_synchronize(pls_hip_handle h) {
    CHK(check_handle(h));
    CHK(set_device(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return check_diverged(h);
}

const char *pls_hip_last_error(pls_hip_handle h) { return h ? h->err.c_str() : "null handle"; }

int pls_hip_get_timing(pls_hip_handle h, pls_hip_timing *out) {
    CHK(check_handle(h));
    if (!out) return PLS_HIP_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    CHK(set_device(h));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (const Launch &l : h->fits) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, l.e0, l.e1));
        out->fit_ms += ms;
        out->fits += 1;
    }
    for (const Launch &l : h->launches) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, l.e0, l.e1));
        out->fam_ms[l.fam] += ms;
        out->fam_launches[l.fam] += 1;
        out->fam_bytes[l.fam] += l.bytes;
    }
    h->launches.clear();  // harvested: recycle the event pool
    h->fits.clear();
    h->ev_used = 0;
    return PLS_HIP_OK;
}

int pls_hip_fit(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                int64_t K, int64_t M, int64_t A, int method, int dtype, int mem, double *W, double *P,
                double *Q, double *R, void *T, int64_t ldt, double *B) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (method != PLS_HIP_KERNEL_TYPE1 && method != PLS_HIP_KERNEL_TYPE2)
        return fail(h, PLS_HIP_ERR_INVALID, "bad method");
    const bool sharded = h->nranks > 1;
    if (N < 0 || (N == 0 && !sharded) || K < 1 || M < 1 || A < 1 || A > K)
        return fail(h, PLS_HIP_ERR_INVALID, "bad shape: need N>=1, K>=1, M>=1, 1<=A<=K");
    if (K > (1 << 30) || M > plsk::LM_MAX)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses (or K > 2^30) not supported on the device");
    if (N > 0 && (!X || !Y || (!T && method == PLS_HIP_KERNEL_TYPE1))) return fail(h, PLS_HIP_ERR_INVALID, "null X/Y/T");
    if ((method == PLS_HIP_KERNEL_TYPE2 || h->opt_algo == PLS_HIP_ALGO_GRAM) && K > 32768)  // (AUTO never picks GRAM there)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "KERNEL_TYPE2 keeps a K x K matrix and 8 reduction slices of it (77 GB at K = 32768): K <= 32768");
    if (!W || !P || !Q || !R) return fail(h, PLS_HIP_ERR_INVALID, "null W/P/Q/R");
    if (ldx < std::max<i64>(N, 1) || ldy < std::max<i64>(N, 1) || (T && ldt < std::max<i64>(N, 1)))
        return fail(h, PLS_HIP_ERR_INVALID, "leading dimension smaller than N");
    // the sample-space plan refuses what it cannot take before anything is written (plan_dual.hpp)
    const bool dual = method == PLS_HIP_KERNEL_TYPE1 && h->opt_algo == PLS_HIP_ALGO_DUAL;
    if (dual)
        if (const char *why = dual_refusal(h, N, M)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, why);
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const int Ki = (int)K, Mi = (int)M, Ai = (int)A;

    // staging (host_entry.hpp); X last: once pre_xx / pre_xy point at its sums, nothing returns before they are cleared
    const void *dX = X, *dY = Y;
    void *dT = T;
    double *dW = W, *dP = P, *dQ = Q, *dR = R, *dB = B;
    i64 dldx = ldx, dldy = ldy, dldt = ldt;
    const i64 ldn = ld_even(N);
    HostCall hc(h, mem);
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(hc.out(dW, W, h->hW, K, A));
    CHK(hc.out(dP, P, h->hP, K, A));
    CHK(hc.out(dR, R, h->hR, K, A));
    CHK(hc.out(dQ, Q, h->hQ, M, A));
    CHK(hc.out(dB, B, h->hB, K, M));
    CHK(hc.place(dT, dldt, h->hT, A, es, ldn));  // (KERNEL_TYPE2 has no scores: nothing to copy back)
    if (method == PLS_HIP_KERNEL_TYPE1) CHK(hc.back(T, ldt, dT, dldt, N, A, es));
    CHK(hc.place(dX, dldx, h->hX, K, es, ldn));
    if (hc.host) CHK(upload_fit_x(h, const_cast<void *>(dX), dY, ldn, X, ldx, N, Ki, Mi, Ai, method, dtype));
    // graph replay (fit_graph.hpp) around the A-loop
    FitGraph g;
    CHK(fit_graph_begin(h, g, X, ldx, Y, ldy, N, K, M, A, method, dtype, mem, W, P, Q, R, T, ldt, B, dual));
    if (g.replayed) return PLS_HIP_OK;
    begin_fit_timing(h);
    int rc = by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return fit_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, Ki, Mi, Ai, method, dW, dP, dQ, dR, (Tx *)dT, dldt, dB);
    });
    end_fit_timing(h);
    rc = fit_graph_end(h, g, rc);
    if (hc.host) h->pre_xx = h->pre_xy = nullptr;
    if (rc != PLS_HIP_OK) return rc;
    return hc.finish(true);
}

int pls_hip_coefficients(pls_hip_handle h, const double *R, const double *Q, int64_t K, int64_t M,
                         int64_t A, int64_t cc, int mem, double *B) {
    CHK(check_handle(h));
    if (!R || !Q || !B || K < 1 || M < 1 || A < 1 || cc < 0 || cc > A || K > (1 << 30))
        return fail(h, PLS_HIP_ERR_INVALID, "bad coefficients arguments");  // comp <= A: src/pls.cpp:445
    CHK(set_device(h));
    CHK(check_mem(h, mem));
    const double *dR = R, *dQ = Q;
    double *dB = B;
    HostCall hc(h, mem);
    CHK(hc.in(dR, R, h->hR, K, A));
    CHK(hc.in(dQ, Q, h->hQ, M, A));
    CHK(hc.out(dB, B, h->hB, K, M));
    const int nblk = (int)((K * M + plsk::WG - 1) / plsk::WG);
    hipLaunchKernelGGL(plsk::coefficients_kernel, dim3(nblk), dim3(plsk::WG), 0, h->stream, dR, dQ,
                       (int)K, (int)M, (int)cc, dB);
    LAUNCH_CHECK(h);
    return hc.finish();
}

int pls_hip_xb(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, const double *Bm,
               int64_t ldb, int64_t C, int dtype, int mem, void *out, int64_t ldo) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (N < 0 || K < 1 || C < 1 || K > (1 << 30) || C > (1 << 20) || ldb < K ||
        ldx < std::max<i64>(N, 1) || ldo < std::max<i64>(N, 1) || !Bm || (N > 0 && (!X || !out)))
        return fail(h, PLS_HIP_ERR_INVALID, "bad xb arguments");
    if (N == 0) return PLS_HIP_OK;
    CHK(set_device(h));
    CHK(check_mem(h, mem));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dBm = Bm;
    void *dO = out;
    i64 dldx = ldx, dldo = ldo, dldb = ldb;
    const i64 ldn = ld_even(N);
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ldn));
    CHK(hc.in(dBm, dldb, Bm, ldb, h->hB, K, C, 8, K));
    CHK(hc.out(dO, dldo, out, ldo, h->hOut, N, C, es, ldn));
    int nss = 0;
    CHK(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_xb<T>(h, (const T *)dX, dldx, N, (int)K, dBm, dldb, (int)C, (T *)dO, dldo, nullptr, &nss);
    }));
    return hc.finish();
}

int pls_hip_xty(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                int64_t K, int64_t M, int dtype, double *XY) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (N < 1 || K < 1 || M < 1 || K > (1 << 30) || M > (1 << 20) || !X || !Y || !XY || ldx < N || ldy < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad xty arguments");
    CHK(set_device(h));
    CHK(ensure(h, h->part, (size_t)max_partial_rows(h, N, (int)K) * (size_t)(K * M) * 8));
    int nb = 0;
    CHK(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_xty<T>(h, (const T *)X, ldx, (const T *)Y, ldy, N, (int)K, (int)M, (double *)h->part.p, &nb);
    }));
    CHK(ensure(h, h->red, (size_t)plsk::RED_SLICES * (size_t)(K * M) * 8));
    CHK(launch_reduce(h, (const double *)h->part.p, nb, (int)(K * M), nullptr, 0, (double *)h->red.p));
    const int nblk = (int)((K * M + plsk::WG - 1) / plsk::WG);
    hipLaunchKernelGGL(plsk::sum_slices_kernel, dim3(nblk), dim3(plsk::WG), 0, h->stream,
                       (const double *)h->red.p, (int)(K * M), XY);
    LAUNCH_CHECK(h);
    return PLS_HIP_OK;
}

int pls_hip_deflate(pls_hip_handle h, const void *src, int64_t lds, void *dst, int64_t ldd, int64_t N,
                    int64_t K, const void *t, const double *p, int dtype) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (N < 1 || K < 1 || K > (1 << 30) || !src || !dst || !t || !p || lds < N || ldd < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad deflate arguments");
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return launch_deflate<T>(h, (const T *)src, lds, (T *)dst, ldd, N, (int)K, (const T *)t, p);
    });
}

int pls_hip_colwise_z_scores(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t n_total,
                             int64_t K, int dtype, void *Z, int64_t ldz, double *mean, double *sd) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (N < 0 || n_total < N || n_total < 1 || K < 1 || K > (1 << 30) || !mean || !sd || (N > 0 && !X) ||
        ldx < std::max<i64>(N, 1) || (Z && ldz < std::max<i64>(N, 1)))
        return fail(h, PLS_HIP_ERR_INVALID, "bad z-score arguments");
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return zscores_device<T>(h, (const T *)X, ldx, N, n_total, (int)K, (T *)Z, ldz, mean, sd);
    });
}

int pls_hip_sse_by_components(pls_hip_handle h, const void *S, int64_t lds, const void *Y, int64_t ldy,
                              int64_t N, int64_t A, int64_t M, const double *Q, int dtype, double *SSE) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (N < 1 || A < 1 || M < 1 || M > 1024 || A > (1 << 20) || !S || !Y || !Q || !SSE || lds < N || ldy < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad sse arguments");
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return sse_device<T>(h, (const T *)S, lds, (const T *)Y, ldy, N, (int)A, (int)M, Q, SSE);
    });
}

int pls_hip_cv_folds(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                     int64_t K, int64_t M, int64_t A, const int64_t *test_idx, int64_t test_size,
                     int64_t num_folds, int dtype, int mem, double *E) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (h->reducer) {  // a collective: local checks here, the ones on global data after the partition message
        if (N < 0 || K < 1 || M < 1 || A < 1 || A > K || K > (1 << 30) || (N > 0 && (!X || !Y)) || !test_idx || !E ||
            test_size < 1 || num_folds < 1 || ldx < std::max<i64>(N, 1) || ldy < std::max<i64>(N, 1) ||
            num_folds > (1 << 22) || test_size > (1 << 20))
            return fail(h, PLS_HIP_ERR_INVALID, "bad cv_folds arguments");
        if (M > plsk::LM_MAX) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses not supported on the device");
        CHK(set_device(h));
        return cv_folds_sharded(h, X, ldx, Y, ldy, N, K, M, A, test_idx, test_size, num_folds, dtype, mem, E);
    }
    if (N < 2 || K < 1 || M < 1 || A < 1 || A > K || K > (1 << 30) || !X || !Y ||
        !test_idx || !E || test_size < 1 || test_size >= N || num_folds < 1 || ldx < N || ldy < N ||
        num_folds > (1 << 22) || test_size > (1 << 20))
        return fail(h, PLS_HIP_ERR_INVALID, "bad cv_folds arguments");
    if (M > plsk::LM_MAX) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses not supported on the device");
    const i64 nobs = num_folds * test_size;
    CHK(check_test_idx(h, test_idx, nobs, N, "cv_folds"));
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X, *dY = Y;
    double *dE = E;
    i64 dldx = ldx, dldy = ldy;
    const i64 ldn = ld_quad(N);
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(ensure(h, h->cve, (size_t)nobs * A * M * 8));  // (for device memory too, as ever)
    CHK(hc.out_flat(dE, E, h->cve, (size_t)nobs * A * M * 8));
    int rc = PLS_HIP_ERR_ALLOC;
    const bool tiny = M == 1 && plsk::tiny_fit_covers(N, (int)K, 1, (int)A, dldx, es) && !h->env.cv_refit && h->env.tiny;
    const bool tiny_m = plsk::tiny_fit_m_covers(N, (int)K, (int)M, (int)A, dldx, es) && !h->env.cv_refit && h->env.tiny;
    const bool micro = plsk::micro_fit_covers(N, (int)K, (int)M, (int)A, dldx, es) && !h->env.cv_refit && h->env.tiny;
    if (cv_dual_covers(h, N, M)) {  // the sample-space plan, an explicit opt-in: every fold from one X X^T
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_folds_dual<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, (int)N, (int)K, (int)M, (int)A, test_idx, (int)test_size,
                                    num_folds, dE);
        });
        if (rc == PLS_HIP_ERR_ALLOC) h->err.clear();  // its workspace does not fit: the routes below
    }
    if (rc != PLS_HIP_ERR_ALLOC) {
        // (the sample-space route took the call)
    } else if (micro || tiny || tiny_m) {  // a single-launch fit per fold, in this order of preference
        const FoldKernel kind = micro ? FoldKernel::micro : tiny ? FoldKernel::tiny : FoldKernel::tiny_m;
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_folds_single_launch<T>(h, kind, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, test_idx,
                                             (int)test_size, num_folds, dE);
        });
    } else if (cv_batched_covers(h, K, M, A)) {
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_folds_device<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, test_idx, (int)test_size,
                                      num_folds, dE);
        });
    }
    if (rc == PLS_HIP_ERR_ALLOC) {  // declined, or the per-fold workspaces of the batched form do not fit: one refit per fold
        h->err.clear();
        rc = by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return cv_folds_refit<T>(h, (const T *)dX, dldx, (const T *)dY, dldy, N, (int)K, (int)M, (int)A, test_idx, (int)test_size,
                                     num_folds, dE);
        });
    }
    if (rc != PLS_HIP_OK) return rc;
    // the index list is host memory of the caller: the work must have consumed it before we return, whatever `mem` is
    return hc.finish(false, true);
}

int pls_hip_fit_batch(pls_hip_handle h, const void *X, int64_t ldx, const void *Ys, int64_t ldy, int64_t N, int64_t K, int64_t M,
                      int64_t A, int64_t nprob, int dtype, int mem, double *R, double *Q, double *tt, double *B, double *ssy) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    const bool empty_member = (N == 0 && h->nranks > 1);  // an empty shard still takes part in the messages
    const i64 n1 = std::max<i64>(N, 1);
    if (N < 0 || (N == 0 && !empty_member) || K < 1 || M < 1 || A < 1 || A > K || nprob < 1 || K > (1 << 30) || M > (1 << 20) ||
        nprob > (1 << 24) || nprob * M > (1 << 30) || (N > 0 && (!X || !Ys)) || ldx < n1 || ldy < n1)
        return fail(h, PLS_HIP_ERR_INVALID, "bad fit_batch arguments: need N>=1, 1<=A<=K, M>=1, nprob>=1, ld>=N, X and Ys");
    CHK(set_device(h));
    return fit_batch_impl(h, X, ldx, Ys, ldy, N, K, M, A, nprob, dtype, mem, R, Q, tt, B, ssy);
}

int pls_hip_fit_resampled(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N, int64_t K, int64_t M,
                          int64_t A, const double *Wt, int64_t ldw, int64_t nrep, int dtype, int mem, double *Q, double *tt, double *B,
                          double *B0, double *Bmean, double *Bm2) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 1 || K < 1 || M < 1 || A < 1 || A > K || nrep < 1 || K > (1 << 30) || M > (1 << 20) || nrep > (1 << 24) ||
        nrep * M > (1 << 30) || !X || !Y || !Wt || ldx < N || ldy < N || ldw < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad fit_resampled arguments: need N>=1, 1<=A<=K, M>=1, nrep>=1, ld>=N, X, Y and Wt");
    CHK(check_unsharded(h, "fit_resampled needs every row of X on one handle: not on a row-sharded handle"));
    // what the general route's pls_hip_fit would refuse, before anything is written
    if (!resample_dual_covers(h, N, M)) {
        if (M > plsk::LM_MAX) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses not supported on the device");
        if (h->opt_algo == PLS_HIP_ALGO_DUAL)
            if (const char *why = dual_refusal(h, N, M)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, why);
    }
    CHK(set_device(h));
    return fit_resampled_impl(h, X, ldx, Y, ldy, N, K, M, A, Wt, ldw, nrep, dtype, mem, Q, tt, B, B0, Bmean, Bm2);
}

int pls_hip_cv_press_batch(pls_hip_handle h, const void *X, int64_t ldx, const void *Ys, int64_t ldy, int64_t N, int64_t K, int64_t M,
                           int64_t A, int64_t nprob, const int64_t *test_idx, int64_t test_size, int64_t num_folds, int dtype, int mem,
                           double *PRESS, double *ssy, double *E) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 2 || K < 1 || M < 1 || A < 1 || A > K || K > (1 << 30) || nprob < 1 || nprob > (1 << 24) || nprob * M > (1 << 30) || !X ||
        !Ys || !test_idx || test_size < 1 || test_size >= N || num_folds < 1 || ldx < N || ldy < N || num_folds > (1 << 22) ||
        test_size > (1 << 20))
        return fail(h, PLS_HIP_ERR_INVALID, "bad cv_press_batch arguments: need N>=2, 1<=A<=K, M>=1, nprob>=1, 1<=test_size<N, ld>=N, X, Ys and test_idx");
    CHK(check_test_idx(h, test_idx, num_folds * test_size, N, "cv_press_batch"));
    CHK(check_unsharded(h, "cv_press_batch needs every row of X on one handle: not on a row-sharded handle"));
    if (M > plsk::LM_MAX) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses not supported on the device");
    CHK(set_device(h));
    return cv_press_batch_impl(h, X, ldx, Ys, ldy, N, K, M, A, nprob, test_idx, test_size, num_folds, dtype, mem, PRESS, ssy, E);
}

int pls_hip_model_sse(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                      int64_t K, int64_t M, int64_t A, const double *R, const double *Q, int dtype, int mem,
                      double *SSE) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    const bool empty_member = (N == 0 && h->nranks > 1);  // an empty shard still takes part in the reduction
    if (N < 0 || (N == 0 && !empty_member) || K < 1 || M < 1 || A < 1 || M > 1024 || A > (1 << 20) || K > (1 << 30) ||
        (N > 0 && (!X || !Y)) || !R || !Q || !SSE || ldx < std::max<i64>(N, 1) || ldy < std::max<i64>(N, 1))
        return fail(h, PLS_HIP_ERR_INVALID, "bad model_sse arguments");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const i64 ldn = ld_even(N);  // (of the scores for device memory too)
    const void *dX = X, *dY = Y;
    const double *dR = R, *dQ = Q;
    double *dE = SSE;
    i64 dldx = ldx, dldy = ldy;
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(hc.in(dR, R, h->hR, K, A));
    CHK(hc.in(dQ, Q, h->hQ, M, A));
    CHK(hc.out(dE, SSE, h->hB, M, A));
    CHK(ensure(h, h->hOut, (size_t)ldn * A * es));  // the scores S = X R stay on the device
    int nss = 0;
    CHK(by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (N > 0) CHK(launch_xb<T>(h, (const T *)dX, dldx, N, (int)K, dR, K, (int)A, (T *)h->hOut.p, ldn, nullptr, &nss));
        return sse_device<T>(h, (const T *)h->hOut.p, ldn, (const T *)dY, dldy, N, (int)A, (int)M, dQ, dE);
    }));
    return hc.finish();
}

int pls_hip_validation(pls_hip_handle h, const double *E, int64_t nobs, int64_t A, int64_t M, int mem, double *PRESS, double *D,
                       double *probw, int64_t *ref) {
    CHK(check_handle(h));
    CHK(check_mem(h, mem));
    if (!E || nobs < 1 || A < 1 || M < 1) return fail(h, PLS_HIP_ERR_INVALID, "bad validation arguments");
    if (nobs > ((i64)1 << 31) - 1 || A > (1 << 20) || M > (1 << 20) || M * A > (1 << 24) ||
        ((nobs + plsk::VAL_CH - 1) / plsk::VAL_CH) * M * A > ((i64)1 << 31) - 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "validation: nobs < 2^31, M A <= 2^24, M A ceil(nobs / 4096) < 2^31");
    CHK(set_device(h));
    // (local on a row-sharded handle: every rank holds the same E, nothing is exchanged)
    return validation_impl(h, E, nobs, (int)A, (int)M, mem, PRESS, D, probw, ref);
}

int pls_hip_x_diagnostics(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t n_total, int64_t K, int64_t A,
                          const double *R, const double *P, const double *tvar, int dtype, int mem, double *Qres, int64_t ldq,
                          double *T2, int64_t ldt2, void *S, int64_t lds, double *ssx, double *sst) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    const bool empty_member = (N == 0 && h->nranks > 1);  // an empty shard still takes part in the message
    const i64 n1 = std::max<i64>(N, 1);
    if (N < 0 || (N == 0 && !empty_member) || n_total < N || n_total < 1 || K < 1 || A < 1 || A > K || A > (1 << 20) ||
        K > (1 << 30) || (N > 0 && !X) || !R || !P || ldx < n1 || (Qres && ldq < n1) || (T2 && ldt2 < n1) || (S && lds < n1))
        return fail(h, PLS_HIP_ERR_INVALID, "bad x_diagnostics arguments");
    if (T2 && !tvar && n_total < 2) return fail(h, PLS_HIP_ERR_INVALID, "x_diagnostics: T2 from the call's own scores needs n_total >= 2");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dR = R, *dP = P, *dtv = tvar;
    double *dQ = Qres, *dT2 = T2, *dssx = ssx, *dsst = sst;
    void *dS = S;
    i64 dldx = ldx, dldq = ldq, dldt2 = ldt2, dlds = lds;
    const i64 ldn = ld_even(N);
    const size_t small = (size_t)(3 * A + 1) * 8;  // xdsmall = [tvar (A), ssx (A + 1), sst (A)]
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ldn));
    CHK(hc.in(dR, R, h->hR, K, A));
    CHK(hc.in(dP, P, h->hP, K, A));
    if (tvar) CHK(hc.in(dtv, tvar, h->xdsmall, A, 1, 8, small, 0));
    CHK(hc.out(dQ, dldq, Qres, ldq, h->xdoQ, N, A, 8, ldn));
    CHK(hc.out(dT2, dldt2, T2, ldt2, h->xdoT, N, A, 8, ldn));
    CHK(hc.out(dS, dlds, S, lds, h->xdoS, N, A, es, ldn));
    CHK(hc.out(dssx, ssx, h->xdsmall, A + 1, 1, 8, small, (size_t)A * 8));
    CHK(hc.out(dsst, sst, h->xdsmall, A, 1, 8, small, (size_t)(2 * A + 1) * 8));
    if (hc.host) dldq = dldt2 = dlds = ldn;  // (of an output that is not asked for as well)
    CHK(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return xdiag_device<T>(h, (const T *)dX, dldx, N, n_total, (int)K, (int)A, dR, dP, dtv, dQ, dldq, dT2, dldt2, (T *)dS, dlds, dssx,
                               dsst);
    }));
    return hc.finish();
}

int pls_hip_var_diagnostics(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t M, int64_t A, const double *W,
                            const double *R, const double *P, const double *Q, const double *tt, int dtype, double *ssxk, int64_t ldk,
                            double *VIP, int64_t ldv, double *sst) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    const bool need_x = ssxk || sst || (VIP && !tt);  // (the same on every rank of a sharded handle: it decides the message)
    const bool empty_member = (N == 0 && h->nranks > 1);  // an empty shard still takes part in the message
    if (K < 1 || A < 1 || A > K || A > (1 << 20) || K > (1 << 30))
        return fail(h, PLS_HIP_ERR_INVALID, "bad var_diagnostics arguments: need 1 <= A <= K, A <= 2^20, K <= 2^30");
    if (need_x && (N < 0 || (N == 0 && !empty_member) || (N > 0 && !X) || ldx < std::max<i64>(N, 1) || !R))
        return fail(h, PLS_HIP_ERR_INVALID, "var_diagnostics: ssxk, sst and VIP without tt need X (N >= 1, ldx >= N) and R");
    if (ssxk && (!P || ldk < K)) return fail(h, PLS_HIP_ERR_INVALID, "var_diagnostics: ssxk needs P and ldk >= K");
    if (VIP && (!W || !Q || M < 1 || ldv < K)) return fail(h, PLS_HIP_ERR_INVALID, "var_diagnostics: VIP needs W, Q, M >= 1 and ldv >= K");
    if (!need_x && !VIP) return PLS_HIP_OK;
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return vardiag_device<T>(h, (const T *)X, ldx, need_x ? N : 0, K, M, (int)A, W, R, P, Q, tt, ssxk, ldk, VIP, ldv, sst);
    });
}

int pls_hip_fit_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N, int64_t K, int64_t M,
                        int64_t A, int dtype, int mem, double *W, double *P, double *Q, double *R, void *T, int64_t ldt, double *B,
                        int64_t *iters) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 1 || K < 1 || M < 1 || A < 1 || A > K || !X || !Y || !W || !P || !Q || !R || !T || ldx < N || ldy < N || ldt < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad fit_missing arguments: need N>=1, 1<=A<=K, M>=1, ld>=N, X, Y, W, P, Q, R and T");
    if (K > (((i64)1 << 31) - 1) || M > plsk::MISS_MAX_M)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "fit_missing takes at most 32 responses (and K < 2^31)");
    CHK(check_unsharded(h, "fit_missing needs every row of X on one handle: not on a row-sharded handle"));
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X, *dY = Y;
    void *dT = T;
    double *dW = W, *dP = P, *dQ = Q, *dR = R, *dB = B;
    long long *dit = (long long *)iters;
    i64 dldx = ldx, dldy = ldy, dldt = ldt;
    const i64 ldn = ld_quad(N);
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(hc.out(dW, W, h->hW, K, A));
    CHK(hc.out(dP, P, h->hP, K, A));
    CHK(hc.out(dR, R, h->hR, K, A));
    CHK(hc.out(dQ, Q, h->hQ, M, A));
    CHK(hc.out(dB, B, h->hB, K, M));
    CHK(hc.out(dT, dldt, T, ldt, h->hT, N, A, es, ldn));
    CHK(hc.out(dit, iters, h->mit, A, 1));
    begin_fit_timing(h);
    const int rc = by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return fit_missing_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, (int)K, (int)M, (int)A, dW, dP, dQ, dR, (Tx *)dT, dldt,
                                      dB, dit);
    });
    end_fit_timing(h);
    if (rc != PLS_HIP_OK) return rc;
    return hc.finish();
}

int pls_hip_cv_folds_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N, int64_t K, int64_t M,
                             int64_t A, const int64_t *test_idx, int64_t test_size, int64_t num_folds, int dtype, int mem, double *E,
                             int64_t *iters) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 2 || K < 1 || M < 1 || A < 1 || A > K || !X || !Y || !test_idx || !E || test_size < 1 || test_size >= N || num_folds < 1 ||
        ldx < N || ldy < N || num_folds > (1 << 22) || test_size > (1 << 20))
        return fail(h, PLS_HIP_ERR_INVALID, "bad cv_folds_missing arguments: need N>=2, 1<=A<=K, M>=1, ld>=N, 1<=test_size<N, X, Y, test_idx and E");
    if (K > (((i64)1 << 31) - 1) || M > plsk::MISS_MAX_M)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "cv_folds_missing takes at most 32 responses (and K < 2^31)");
    CHK(check_unsharded(h, "cv_folds_missing needs every row of X on one handle: not on a row-sharded handle"));
    const i64 nobs = num_folds * test_size;
    {
        std::unique_ptr<i64[]> fold_of(new (std::nothrow) i64[(size_t)N]);  // the last fold that held a row out
        if (!fold_of) return fail(h, PLS_HIP_ERR_ALLOC, "cv_folds_missing: no host memory for the index check");
        std::fill_n(fold_of.get(), N, (i64)-1);
        for (i64 f = 0; f < num_folds; ++f)
            for (i64 j = f * test_size; j < (f + 1) * test_size; ++j) {
                if (test_idx[j] < 0 || test_idx[j] >= N) return fail(h, PLS_HIP_ERR_INVALID, "cv_folds_missing: test index out of range");
                if (fold_of[test_idx[j]] == f) return fail(h, PLS_HIP_ERR_INVALID, "cv_folds_missing: a fold holds a row out twice");
                fold_of[test_idx[j]] = f;
            }
    }
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X, *dY = Y;
    double *dE = E;
    long long *dit = (long long *)iters;
    i64 dldx = ldx, dldy = ldy;
    const i64 ldn = ld_quad(N);
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hX, N, K, es, ldn));
    CHK(hc.in(dY, dldy, Y, ldy, h->hY, N, M, es, ldn));
    CHK(hc.out_flat(dE, E, h->cve, (size_t)nobs * A * M * 8));
    CHK(hc.out_flat(dit, iters, h->mit, (size_t)num_folds * A * 8));
    CHK(ensure(h, h->mcvidx, (size_t)nobs * 8));
    HIPCHK(h, hipMemcpyAsync(h->mcvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return cv_folds_missing_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, (int)K, (int)M, (int)A,
                                           (const long long *)h->mcvidx.p, (int)test_size, num_folds, dE, dit);
    }));
    return hc.finish();
}

int pls_hip_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t A, const double *W, const double *P,
                           int dtype, int mem, void *S, int64_t lds) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 1 || K < 1 || A < 1 || A > K || !X || !W || !P || !S || ldx < N || lds < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad scores_missing arguments: need N>=1, 1<=A<=K, ld>=N, X, W, P and S");
    if (K > (((i64)1 << 31) - 1)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "scores_missing: K < 2^31");
    CHK(check_unsharded(h, "scores_missing: not on a row-sharded handle"));
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dW = W, *dP = P;
    void *dS = S;
    i64 dldx = ldx, dlds = lds;
    const i64 ldn = ld_quad(N);
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ldn));
    CHK(hc.in(dW, W, h->hW, K, A));
    CHK(hc.in(dP, P, h->hP, K, A));
    CHK(hc.out(dS, dlds, S, lds, h->hOut, N, A, es, ldn));
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return scores_missing_device<Tx>(h, (const Tx *)dX, dldx, N, (int)K, (int)A, dW, dP, (Tx *)dS, dlds);
    }));
    return hc.finish();
}

int pls_hip_x_diagnostics_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t A, const double *W,
                                  const double *P, const double *tvar, int dtype, int mem, double *Qres, int64_t ldq, double *T2,
                                  int64_t ldt2, void *S, int64_t lds, double *ssx, double *sst, int64_t *nobs) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 1 || K < 1 || A < 1 || A > K || !X || !W || !P || ldx < N || (Qres && ldq < N) || (T2 && ldt2 < N) || (S && lds < N))
        return fail(h, PLS_HIP_ERR_INVALID, "bad x_diagnostics_missing arguments: need N>=1, 1<=A<=K, ld>=N, X, W and P");
    if (T2 && !tvar && N < 2)
        return fail(h, PLS_HIP_ERR_INVALID, "x_diagnostics_missing: T2 from the call's own scores needs N >= 2");
    if (K > (((i64)1 << 31) - 1) || A > (1 << 20)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "x_diagnostics_missing: K < 2^31, A <= 2^20");
    CHK(check_unsharded(h, "x_diagnostics_missing: not on a row-sharded handle"));
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dW = W, *dP = P, *dtv = tvar;
    double *dQ = Qres, *dT2 = T2, *dssx = ssx, *dsst = sst;
    void *dS = S;
    long long *dn = (long long *)nobs;
    i64 dldx = ldx, dldq = ldq, dldt2 = ldt2, dlds = lds;
    const i64 ldn = ld_quad(N);
    const size_t small = (size_t)(3 * A + 1) * 8;  // xdsmall = [tvar (A), ssx (A + 1), sst (A)]
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ldn));
    CHK(hc.in(dW, W, h->hW, K, A));
    CHK(hc.in(dP, P, h->hP, K, A));
    if (tvar) CHK(hc.in(dtv, tvar, h->xdsmall, A, 1, 8, small, 0));
    CHK(hc.out(dQ, dldq, Qres, ldq, h->xdoQ, N, A, 8, ldn));
    CHK(hc.out(dT2, dldt2, T2, ldt2, h->xdoT, N, A, 8, ldn));
    CHK(hc.out(dS, dlds, S, lds, h->xdoS, N, A, es, ldn));
    CHK(hc.out(dssx, ssx, h->xdsmall, A + 1, 1, 8, small, (size_t)A * 8));
    CHK(hc.out(dsst, sst, h->xdsmall, A, 1, 8, small, (size_t)(2 * A + 1) * 8));
    CHK(hc.out(dn, nobs, h->xmon, N, 1));
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return xdiag_missing_device<Tx>(h, (const Tx *)dX, dldx, N, (int)K, (int)A, dW, dP, dtv, dQ, dldq, dT2, dldt2, (Tx *)dS, dlds, dssx,
                                        dsst, dn);
    }));
    return hc.finish();
}

int pls_hip_colwise_z_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int dtype, int mem, void *Z,
                                     int64_t ldz, double *mean, double *sd, int64_t *nobs) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    CHK(check_mem(h, mem));
    if (N < 1 || K < 1 || !X || !mean || !sd || ldx < N || (Z && ldz < N))
        return fail(h, PLS_HIP_ERR_INVALID, "bad z_scores_missing arguments: need N>=1, K>=1, ld>=N, X, mean and sd");
    if (K > (((i64)1 << 31) - 1)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "z_scores_missing: K < 2^31");
    CHK(check_unsharded(h, "z_scores_missing: single rank only, not on a row-sharded handle"));
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    void *dZ = Z;
    double *dmean = mean, *dsd = sd;
    long long *dn = (long long *)nobs;
    i64 dldx = ldx, dldz = ldz;
    const size_t small = (size_t)K * 3 * 8;  // mzo = [mean, sd, nobs]
    HostCall hc(h, mem);
    CHK(hc.in(dX, dldx, X, ldx, h->hIn, N, K, es, ld_exact(N)));
    if (hc.host) {  // scaled in place in the staging copy
        dZ = Z ? const_cast<void *>(dX) : nullptr;
        dldz = dldx;
        CHK(hc.back(Z, ldz, dZ, dldz, N, K, es));
    }
    CHK(hc.out(dmean, mean, h->mzo, K, 1, 8, small, 0));
    CHK(hc.out(dsd, sd, h->mzo, K, 1, 8, small, (size_t)K * 8));
    CHK(hc.out(dn, nobs, h->mzo, K, 1, 8, small, (size_t)K * 16));
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return zscores_missing_device<Tx>(h, (const Tx *)dX, dldx, N, (int)K, (Tx *)dZ, dldz, dmean, dsd, dn);
    }));
    return hc.finish();
}

int pls_hip_synth_x(pls_hip_handle h, void *X, int64_t ldx, int64_t row0, int64_t nrows, int64_t K,
                    uint64_t seed, int dtype) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (nrows < 0 || row0 < 0 || K < 1 || K > (1 << 28) || (nrows > 0 && !X) || ldx < std::max<i64>(nrows, 1))
        return fail(h, PLS_HIP_ERR_INVALID, "bad synth_x arguments");
    if (nrows == 0) return PLS_HIP_OK;
    CHK(set_device(h));
    CHK(ensure(h, h->tab, (size_t)K * (plsk::SYN_F + 1) * 8));
    const uint64_t sE = plsk::mix64(seed), sZ = plsk::mix64(seed + 1), sL = plsk::mix64(seed + 2);
    const int ntab = (int)((K * plsk::SYN_F + plsk::WG - 1) / plsk::WG);
    hipLaunchKernelGGL(plsk::synth_table_kernel, dim3(ntab), dim3(plsk::WG), 0, h->stream,
                       (double *)h->tab.p, (int)K, sL, 0, plsk::mix64(seed + 5));
    LAUNCH_CHECK(h);
    constexpr int KC = 64;
    const dim3 grid((unsigned)((nrows + plsk::WG - 1) / plsk::WG), (unsigned)((K + KC - 1) / KC));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((plsk::synth_x_kernel<T, KC>), grid, dim3(plsk::WG), 0, h->stream, (T *)X, ldx, row0, nrows, (int)K, sE, sZ,
                           (const double *)h->tab.p);
    });
    LAUNCH_CHECK(h);
    return PLS_HIP_OK;
}

int pls_hip_synth_y(pls_hip_handle h, void *Y, int64_t ldy, int64_t row0, int64_t nrows, int64_t M,
                    uint64_t seed, int dtype) {
    CHK(check_handle(h));
    CHK(check_dtype(h, dtype));
    if (nrows < 0 || row0 < 0 || M < 1 || M > (1 << 20) || (nrows > 0 && !Y) || ldy < std::max<i64>(nrows, 1))
        return fail(h, PLS_HIP_ERR_INVALID, "bad synth_y arguments");
    if (nrows == 0) return PLS_HIP_OK;
    CHK(set_device(h));
    // the Y table shares the workspace with the X table: generate Y before or after X, both
    // are stream-ordered
    CHK(ensure(h, h->tab, (size_t)std::max<i64>(M, 1) * plsk::SYN_F * 8));
    const uint64_t sZ = plsk::mix64(seed + 1), sC = plsk::mix64(seed + 3), sN = plsk::mix64(seed + 4);
    const int ntab = (int)((M * plsk::SYN_F + plsk::WG - 1) / plsk::WG);
    hipLaunchKernelGGL(plsk::synth_table_kernel, dim3(ntab), dim3(plsk::WG), 0, h->stream,
                       (double *)h->tab.p, (int)M, sC, 1, (uint64_t)0);
    LAUNCH_CHECK(h);
    const dim3 grid((unsigned)((nrows + plsk::WG - 1) / plsk::WG));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((plsk::synth_y_kernel<T>), grid, dim3(plsk::WG), 0, h->stream, (T *)Y, ldy, row0, nrows, (int)M, sZ, sN,
                           (const double *)h->tab.p);
    });
    LAUNCH_CHECK(h);
    return PLS_HIP_OK;
}

}  // extern "C"
