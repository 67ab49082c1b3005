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
#include "batch_kernels.hpp"
#include "dual_kernels.hpp"
#include "dual_cv_kernels.hpp"
#include "dual_batch_kernels.hpp"
#include "dual_cvbatch_kernels.hpp"
#include "resample_kernels.hpp"
#include "synth_kernels.hpp"
#include "missing_kernels.hpp"
#include "missing_cv_kernels.hpp"
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
#include "plan_validation.hpp"
#include "plan_xdiag.hpp"

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
    {
        auto off = [](const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; };
        auto on = [](const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; };
        c->env.tiny = !off("PLS_HIP_TINY");
        c->env.cv_refit = on("PLS_HIP_CV_REFIT");
        c->env.batch_refit = on("PLS_HIP_BATCH_REFIT");
        if (const char *e = getenv("PLS_HIP_BATCH_ROUND")) c->env.batch_round = atoll(e);
        if (const char *e = getenv("PLS_HIP_DUALCV_ROUND")) c->env.dualcv_round = atoll(e);
        if (const char *e = getenv("PLS_HIP_DUALBATCH_ROUND")) c->env.dualbatch_round = atoll(e);
        if (const char *e = getenv("PLS_HIP_RESAMPLE_ROUND")) c->env.resample_round = atoll(e);
        c->env.resample_refit = on("PLS_HIP_RESAMPLE_REFIT");
        c->env.dualbatch_sweeps = on("PLS_HIP_DUALBATCH_SWEEPS");
        c->env.cvbatch_refit = on("PLS_HIP_CVBATCH_REFIT");
        if (const char *e = getenv("PLS_HIP_DUALCVB_ROUND")) c->env.dualcvb_round = atoll(e);
        if (const char *e = getenv("PLS_HIP_MISSCV_ROUND")) c->env.misscv_round = atoll(e);
        c->env.tail = !off("PLS_HIP_TAIL");
        {
            const char *e = getenv("PLS_HIP_TAIL");
            c->env.tail_update = e ? (atoi(e) >= 2 ? 2 : 0) : 1;
        }
        c->env.replica_guard = !off("PLS_HIP_REPLICA_GUARD");
        c->env.resident = !off("PLS_HIP_RESIDENT");
        c->env.turnaround = !off("PLS_HIP_TURNAROUND");
#ifdef PLS_HIP_TESTING
        if (const char *e = getenv("PLS_HIP_TEST_TURN_EDGE_BYTES")) c->env.turn_edge_bytes = atoll(e);  // (small matrices with a bulk, tests only)
#endif
        if (const char *e = getenv("PLS_HIP_XB4")) c->env.xb4 = atoi(e);
        if (const char *e = getenv("PLS_HIP_RESIDENT_GRAM")) c->env.resident_gram = atoi(e);
    }
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
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

    const void *dX = X, *dY = Y;
    void *dT = T;
    double *dW = W, *dP = P, *dQ = Q, *dR = R, *dB = B;
    i64 dldx = ldx, dldy = ldy, dldt = ldt;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = std::max<i64>(N, 1) + (std::max<i64>(N, 1) & 1);  // even ld keeps 16-B columns
        CHK(ensure(h, h->hX, (size_t)ldn * K * es));
        CHK(ensure(h, h->hY, (size_t)ldn * M * es));
        CHK(ensure(h, h->hT, (size_t)ldn * A * es));
        CHK(ensure(h, h->hW, (size_t)K * A * 8));
        CHK(ensure(h, h->hP, (size_t)K * A * 8));
        CHK(ensure(h, h->hR, (size_t)K * A * 8));
        CHK(ensure(h, h->hQ, (size_t)M * A * 8));
        CHK(ensure(h, h->hB, (size_t)K * M * 8));
        CHK(h2d(h, h->hY.p, ldn, Y, ldy, N, M, es));
        // A plan that works from X^T X (AUTO, GRAM, KERNEL_TYPE2) gets it for free: accumulated on the matrix cores
        // row block by row block while X crosses PCIe (upload_accumulate).  Single rank only: the ranks of a sharded
        // fit must not differ in their plan.
        bool pre = false;
        const bool wants_gram = h->opt_algo == PLS_HIP_ALGO_AUTO || h->opt_algo == PLS_HIP_ALGO_GRAM || method == PLS_HIP_KERNEL_TYPE2;
        const bool single_launch = method == PLS_HIP_KERNEL_TYPE1 && h->opt_algo == PLS_HIP_ALGO_AUTO && h->opt_fuse &&
                                   (plsk::tiny_fit_covers(N, Ki, Mi, Ai, ldn, es) || plsk::tiny_fit_m_covers(N, Ki, Mi, Ai, ldn, es) ||
                                    plsk::micro_fit_covers(N, Ki, Mi, Ai, ldn, es));  // (no use for X^T X there)
        if (wants_gram && !single_launch && !h->reducer && N > 0 && K <= 4096 && ensure(h, h->gxx, (size_t)K * K * 8) == PLS_HIP_OK &&
            ensure(h, h->gxy, (size_t)K * M * 8) == PLS_HIP_OK) {
            CHK(by_dtype(dtype, [&](auto t) {
                using Tx = decltype(t);
                return upload_accumulate<Tx>(h, (Tx *)h->hX.p, ldn, (const Tx *)X, ldx, N, Ki, (const Tx *)h->hY.p, ldn, Mi, (double *)h->gxx.p,
                                            (double *)h->gxy.p, &pre);
            }));
        } else {
            h->err.clear();
            CHK(h2d(h, h->hX.p, ldn, X, ldx, N, K, es));
        }
        if (pre) {
            h->pre_xx = (const double *)h->gxx.p;
            h->pre_xy = (const double *)h->gxy.p;
        }
        dX = h->hX.p; dY = h->hY.p; dT = h->hT.p;
        dW = (double *)h->hW.p; dP = (double *)h->hP.p; dQ = (double *)h->hQ.p; dR = (double *)h->hR.p;
        dB = B ? (double *)h->hB.p : nullptr;
        dldx = dldy = dldt = ldn;
    }
    // PLS_HIP_OPT_GRAPH: a repeated device-memory fit is replayed as one graph launch.  First occurrence of a call: eager (it
    // also sizes every workspace); second: the same enqueue sequence under stream capture (nothing allocates any more),
    // instantiated and launched; from the third on: hipGraphLaunch.  The kernel arguments are baked into the graph, so the key
    // is everything they derive from.
    // (a DUAL fit is never captured: it simply runs)
    const bool graphable = h->opt_graph && mem == PLS_HIP_MEM_DEVICE && !h->reducer && h->opt_profile == 0 && !h->user_red &&
                           h->stream != nullptr && !dual;  // (the legacy default stream cannot be captured)
    std::vector<uint64_t> key;
    if (graphable) {
        key = {(uint64_t)(uintptr_t)X, (uint64_t)ldx, (uint64_t)(uintptr_t)Y, (uint64_t)ldy, (uint64_t)N, (uint64_t)K, (uint64_t)M,
               (uint64_t)A, (uint64_t)method, (uint64_t)dtype, (uint64_t)(uintptr_t)W, (uint64_t)(uintptr_t)P, (uint64_t)(uintptr_t)Q,
               (uint64_t)(uintptr_t)R, (uint64_t)(uintptr_t)T, (uint64_t)ldt, (uint64_t)(uintptr_t)B, (uint64_t)h->opt_algo,
               (uint64_t)h->opt_fuse, (uint64_t)h->opt_power_iters, (uint64_t)h->opt_fused_grid, (uint64_t)h->opt_work_layout,
               (uint64_t)h->opt_defer, (uint64_t)(uintptr_t)h->stream, (uint64_t)(uintptr_t)h->pre_xx, (uint64_t)(uintptr_t)h->pre_xy};
        if (h->graph_exec && key == h->graph_key) {
            HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));
            return PLS_HIP_OK;
        }
    }
    const bool capture = graphable && key == h->graph_seen;
    if (capture) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; h->graph_key.clear(); }
        HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    }
    begin_fit_timing(h);
    const int rc = by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return fit_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, Ki, Mi, Ai, method, dW, dP, dQ, dR, (Tx *)dT, dldt, dB);
    });
    end_fit_timing(h);
    if (capture) {
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(h->stream, &graph);
        if (rc == PLS_HIP_OK && ce == hipSuccess && graph && hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            h->graph_key = key;
            (void)hipGraphDestroy(graph);
            HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));  // this call's work
        } else {
            if (graph) (void)hipGraphDestroy(graph);
            h->graph_exec = nullptr;
            h->graph_seen.clear();
            (void)hipGetLastError();
            if (rc != PLS_HIP_OK) return rc;
            return fail(h, PLS_HIP_ERR_DEVICE, "stream capture of the fit failed");
        }
    } else if (graphable) {
        h->graph_seen = key;
    }
    if (mem == PLS_HIP_MEM_HOST) h->pre_xx = h->pre_xy = nullptr;
    if (rc != PLS_HIP_OK) return rc;
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, W, K, dW, K, K, A, 8));
        CHK(d2h(h, P, K, dP, K, K, A, 8));
        CHK(d2h(h, R, K, dR, K, K, A, 8));
        CHK(d2h(h, Q, M, dQ, M, M, A, 8));
        if (B) CHK(d2h(h, B, K, dB, K, K, M, 8));
        if (method == PLS_HIP_KERNEL_TYPE1) CHK(d2h(h, T, ldt, dT, dldt, N, A, es));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        CHK(check_diverged(h));
    }
    return PLS_HIP_OK;
}

int pls_hip_coefficients(pls_hip_handle h, const double *R, const double *Q, int64_t K, int64_t M,
                         int64_t A, int64_t cc, int mem, double *B) {
    CHK(check_handle(h));
    if (!R || !Q || !B || K < 1 || M < 1 || A < 1 || cc < 0 || cc > A || K > (1 << 30))
        return fail(h, PLS_HIP_ERR_INVALID, "bad coefficients arguments");  // comp <= A: src/pls.cpp:445
    CHK(set_device(h));
    const double *dR = R, *dQ = Q;
    double *dB = B;
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(ensure(h, h->hR, (size_t)K * A * 8));
        CHK(ensure(h, h->hQ, (size_t)M * A * 8));
        CHK(ensure(h, h->hB, (size_t)K * M * 8));
        CHK(h2d(h, h->hR.p, K, R, K, K, A, 8));
        CHK(h2d(h, h->hQ.p, M, Q, M, M, A, 8));
        dR = (double *)h->hR.p; dQ = (double *)h->hQ.p; dB = (double *)h->hB.p;
    } else if (mem != PLS_HIP_MEM_DEVICE) {
        return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    }
    const int nblk = (int)((K * M + plsk::WG - 1) / plsk::WG);
    hipLaunchKernelGGL(plsk::coefficients_kernel, dim3(nblk), dim3(plsk::WG), 0, h->stream, dR, dQ,
                       (int)K, (int)M, (int)cc, dB);
    LAUNCH_CHECK(h);
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, B, K, dB, K, K, M, 8));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_xb(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, const double *Bm,
               int64_t ldb, int64_t C, int dtype, int mem, void *out, int64_t ldo) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (N < 0 || K < 1 || C < 1 || K > (1 << 30) || C > (1 << 20) || ldb < K ||
        ldx < std::max<i64>(N, 1) || ldo < std::max<i64>(N, 1) || !Bm || (N > 0 && (!X || !out)))
        return fail(h, PLS_HIP_ERR_INVALID, "bad xb arguments");
    if (N == 0) return PLS_HIP_OK;
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dBm = Bm;
    void *dO = out;
    i64 dldx = ldx, dldo = ldo, dldb = ldb;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + (N & 1);
        CHK(ensure(h, h->hIn, (size_t)ldn * K * es));
        CHK(ensure(h, h->hOut, (size_t)ldn * C * es));
        CHK(ensure(h, h->hB, (size_t)K * C * 8));
        CHK(h2d(h, h->hIn.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hB.p, K, Bm, ldb, K, C, 8));
        dX = h->hIn.p; dO = h->hOut.p; dBm = (const double *)h->hB.p;
        dldx = dldo = ldn; dldb = K;
    } else if (mem != PLS_HIP_MEM_DEVICE) {
        return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    }
    int nss = 0;
    CHK(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_xb<T>(h, (const T *)dX, dldx, N, (int)K, dBm, dldb, (int)C, (T *)dO, dldo, nullptr, &nss);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, out, ldo, dO, dldo, N, C, es));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_xty(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                int64_t K, int64_t M, int dtype, double *XY) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (N < 1 || K < 1 || K > (1 << 30) || !src || !dst || !t || !p || lds < N || ldd < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad deflate arguments");
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        return launch_deflate<T>(h, (const T *)src, lds, (T *)dst, ldd, N, (int)K, (const T *)t, p);
    });
}

}  // extern "C"

#include "plan_stats.hpp"


extern "C" {

int pls_hip_colwise_z_scores(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t n_total,
                             int64_t K, int dtype, void *Z, int64_t ldz, double *mean, double *sd) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (N < 1 || A < 1 || M < 1 || M > 1024 || A > (1 << 20) || !S || !Y || !Q || !SSE || lds < N || ldy < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad sse arguments");
    CHK(set_device(h));
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return sse_device<T>(h, (const T *)S, lds, (const T *)Y, ldy, N, (int)A, (int)M, Q, SSE);
    });
}

}  // extern "C"

#include "plan_cv.hpp"
#include "dual_round.hpp"
#include "plan_dual_cv.hpp"
#include "plan_dual_batch.hpp"
#include "plan_batch.hpp"
#include "plan_resample.hpp"
#include "plan_dual_cvbatch.hpp"
#include "plan_missing.hpp"
#include "plan_missing_cv.hpp"


extern "C" {

int pls_hip_cv_folds(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                     int64_t K, int64_t M, int64_t A, const int64_t *test_idx, int64_t test_size,
                     int64_t num_folds, int dtype, int mem, double *E) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
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
    for (i64 j = 0; j < nobs; ++j)
        if (test_idx[j] < 0 || test_idx[j] >= N) return fail(h, PLS_HIP_ERR_INVALID, "cv_folds: test index out of range");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X, *dY = Y;
    i64 dldx = ldx, dldy = ldy;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + ((-N) & 3);  // 16-byte columns for either type
        CHK(ensure(h, h->hX, (size_t)ldn * K * es));
        CHK(ensure(h, h->hY, (size_t)ldn * M * es));
        CHK(h2d(h, h->hX.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hY.p, ldn, Y, ldy, N, M, es));
        dX = h->hX.p; dY = h->hY.p;
        dldx = dldy = ldn;
    }
    CHK(ensure(h, h->cve, (size_t)nobs * A * M * 8));
    double *dE = (mem == PLS_HIP_MEM_HOST) ? (double *)h->cve.p : E;
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
    if (mem == PLS_HIP_MEM_HOST)
        HIPCHK(h, hipMemcpyAsync(E, dE, (size_t)nobs * A * M * 8, hipMemcpyDeviceToHost, h->stream));
    // the index list is host memory of the caller: the copy above must have consumed it before we return
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PLS_HIP_OK;
}

int pls_hip_fit_batch(pls_hip_handle h, const void *X, int64_t ldx, const void *Ys, int64_t ldy, int64_t N, int64_t K, int64_t M,
                      int64_t A, int64_t nprob, int dtype, int mem, double *R, double *Q, double *tt, double *B, double *ssy) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 1 || K < 1 || M < 1 || A < 1 || A > K || nrep < 1 || K > (1 << 30) || M > (1 << 20) || nrep > (1 << 24) ||
        nrep * M > (1 << 30) || !X || !Y || !Wt || ldx < N || ldy < N || ldw < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad fit_resampled arguments: need N>=1, 1<=A<=K, M>=1, nrep>=1, ld>=N, X, Y and Wt");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "fit_resampled needs every row of X on one handle: not on a row-sharded handle");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 2 || K < 1 || M < 1 || A < 1 || A > K || K > (1 << 30) || nprob < 1 || nprob > (1 << 24) || nprob * M > (1 << 30) || !X ||
        !Ys || !test_idx || test_size < 1 || test_size >= N || num_folds < 1 || ldx < N || ldy < N || num_folds > (1 << 22) ||
        test_size > (1 << 20))
        return fail(h, PLS_HIP_ERR_INVALID, "bad cv_press_batch arguments: need N>=2, 1<=A<=K, M>=1, nprob>=1, 1<=test_size<N, ld>=N, X, Ys and test_idx");
    const i64 nobs = num_folds * test_size;
    for (i64 j = 0; j < nobs; ++j)
        if (test_idx[j] < 0 || test_idx[j] >= N) return fail(h, PLS_HIP_ERR_INVALID, "cv_press_batch: test index out of range");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "cv_press_batch needs every row of X on one handle: not on a row-sharded handle");
    if (M > plsk::LM_MAX) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "more than 1024 responses not supported on the device");
    CHK(set_device(h));
    return cv_press_batch_impl(h, X, ldx, Ys, ldy, N, K, M, A, nprob, test_idx, test_size, num_folds, dtype, mem, PRESS, ssy, E);
}

int pls_hip_model_sse(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N,
                      int64_t K, int64_t M, int64_t A, const double *R, const double *Q, int dtype, int mem,
                      double *SSE) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    const bool empty_member = (N == 0 && h->nranks > 1);  // an empty shard still takes part in the reduction
    if (N < 0 || (N == 0 && !empty_member) || K < 1 || M < 1 || A < 1 || M > 1024 || A > (1 << 20) || K > (1 << 30) ||
        (N > 0 && (!X || !Y)) || !R || !Q || !SSE || ldx < std::max<i64>(N, 1) || ldy < std::max<i64>(N, 1))
        return fail(h, PLS_HIP_ERR_INVALID, "bad model_sse arguments");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const i64 ldn = std::max<i64>(N, 1) + (std::max<i64>(N, 1) & 1);
    const void *dX = X, *dY = Y;
    const double *dR = R, *dQ = Q;
    double *dE = SSE;
    i64 dldx = ldx, dldy = ldy;
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(ensure(h, h->hIn, (size_t)ldn * K * es));
        CHK(ensure(h, h->hY, (size_t)ldn * M * es));
        CHK(ensure(h, h->hR, (size_t)K * A * 8));
        CHK(ensure(h, h->hQ, (size_t)M * A * 8));
        CHK(ensure(h, h->hB, (size_t)M * A * 8));
        CHK(h2d(h, h->hIn.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hY.p, ldn, Y, ldy, N, M, es));
        CHK(h2d(h, h->hR.p, K, R, K, K, A, 8));
        CHK(h2d(h, h->hQ.p, M, Q, M, M, A, 8));
        dX = h->hIn.p; dY = h->hY.p; dR = (const double *)h->hR.p; dQ = (const double *)h->hQ.p;
        dE = (double *)h->hB.p;
        dldx = dldy = ldn;
    }
    CHK(ensure(h, h->hOut, (size_t)ldn * A * es));  // the scores S = X R stay on the device
    int nss = 0;
    CHK(by_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (N > 0) CHK(launch_xb<T>(h, (const T *)dX, dldx, N, (int)K, dR, K, (int)A, (T *)h->hOut.p, ldn, nullptr, &nss));
        return sse_device<T>(h, (const T *)h->hOut.p, ldn, (const T *)dY, dldy, N, (int)A, (int)M, dQ, dE);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, SSE, M, dE, M, M, A, 8));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_validation(pls_hip_handle h, const double *E, int64_t nobs, int64_t A, int64_t M, int mem, double *PRESS, double *D,
                       double *probw, int64_t *ref) {
    CHK(check_handle(h));
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
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
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = n1 + (n1 & 1);
        CHK(ensure(h, h->hIn, (size_t)ldn * K * es));
        CHK(ensure(h, h->hR, (size_t)K * A * 8));
        CHK(ensure(h, h->hP, (size_t)K * A * 8));
        CHK(ensure(h, h->xdsmall, (size_t)(3 * A + 1) * 8));  // [tvar (A), ssx (A + 1), sst (A)]
        if (Qres) CHK(ensure(h, h->xdoQ, (size_t)ldn * A * 8));
        if (T2) CHK(ensure(h, h->xdoT, (size_t)ldn * A * 8));
        if (S) CHK(ensure(h, h->xdoS, (size_t)ldn * A * es));
        CHK(h2d(h, h->hIn.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hR.p, K, R, K, K, A, 8));
        CHK(h2d(h, h->hP.p, K, P, K, K, A, 8));
        double *small = (double *)h->xdsmall.p;
        if (tvar) CHK(h2d(h, small, A, tvar, A, A, 1, 8));
        dX = h->hIn.p; dR = (const double *)h->hR.p; dP = (const double *)h->hP.p;
        dtv = tvar ? small : nullptr;
        dQ = Qres ? (double *)h->xdoQ.p : nullptr;
        dT2 = T2 ? (double *)h->xdoT.p : nullptr;
        dS = S ? h->xdoS.p : nullptr;
        dssx = ssx ? small + A : nullptr;
        dsst = sst ? small + 2 * A + 1 : nullptr;
        dldx = dldq = dldt2 = dlds = ldn;
    }
    CHK(by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return xdiag_device<T>(h, (const T *)dX, dldx, N, n_total, (int)K, (int)A, dR, dP, dtv, dQ, dldq, dT2, dldt2, (T *)dS, dlds, dssx,
                               dsst);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        if (Qres) CHK(d2h(h, Qres, ldq, dQ, dldq, N, A, 8));
        if (T2) CHK(d2h(h, T2, ldt2, dT2, dldt2, N, A, 8));
        if (S) CHK(d2h(h, S, lds, dS, dlds, N, A, es));
        if (ssx) CHK(d2h(h, ssx, A + 1, dssx, A + 1, A + 1, 1, 8));
        if (sst) CHK(d2h(h, sst, A, dsst, A, A, 1, 8));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_fit_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N, int64_t K, int64_t M,
                        int64_t A, int dtype, int mem, double *W, double *P, double *Q, double *R, void *T, int64_t ldt, double *B,
                        int64_t *iters) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 1 || K < 1 || M < 1 || A < 1 || A > K || !X || !Y || !W || !P || !Q || !R || !T || ldx < N || ldy < N || ldt < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad fit_missing arguments: need N>=1, 1<=A<=K, M>=1, ld>=N, X, Y, W, P, Q, R and T");
    if (K > (((i64)1 << 31) - 1) || M > plsk::MISS_MAX_M)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "fit_missing takes at most 32 responses (and K < 2^31)");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "fit_missing needs every row of X on one handle: not on a row-sharded handle");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X, *dY = Y;
    void *dT = T;
    double *dW = W, *dP = P, *dQ = Q, *dR = R, *dB = B;
    long long *dit = (long long *)iters;
    i64 dldx = ldx, dldy = ldy, dldt = ldt;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + ((-N) & 3);  // 16-byte columns for either type
        CHK(ensure(h, h->hX, (size_t)ldn * K * es));
        CHK(ensure(h, h->hY, (size_t)ldn * M * es));
        CHK(ensure(h, h->hT, (size_t)ldn * A * es));
        CHK(ensure(h, h->hW, (size_t)K * A * 8));
        CHK(ensure(h, h->hP, (size_t)K * A * 8));
        CHK(ensure(h, h->hR, (size_t)K * A * 8));
        CHK(ensure(h, h->hQ, (size_t)M * A * 8));
        if (B) CHK(ensure(h, h->hB, (size_t)K * M * 8));
        if (iters) CHK(ensure(h, h->mit, (size_t)A * 8));
        CHK(h2d(h, h->hX.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hY.p, ldn, Y, ldy, N, M, es));
        dX = h->hX.p; dY = h->hY.p; dT = h->hT.p;
        dW = (double *)h->hW.p; dP = (double *)h->hP.p; dQ = (double *)h->hQ.p; dR = (double *)h->hR.p;
        dB = B ? (double *)h->hB.p : nullptr;
        dit = iters ? (long long *)h->mit.p : nullptr;
        dldx = dldy = dldt = ldn;
    }
    begin_fit_timing(h);
    const int rc = by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return fit_missing_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, (int)K, (int)M, (int)A, dW, dP, dQ, dR, (Tx *)dT, dldt,
                                      dB, dit);
    });
    end_fit_timing(h);
    if (rc != PLS_HIP_OK) return rc;
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, W, K, dW, K, K, A, 8));
        CHK(d2h(h, P, K, dP, K, K, A, 8));
        CHK(d2h(h, R, K, dR, K, K, A, 8));
        CHK(d2h(h, Q, M, dQ, M, M, A, 8));
        if (B) CHK(d2h(h, B, K, dB, K, K, M, 8));
        CHK(d2h(h, T, ldt, dT, dldt, N, A, es));
        if (iters) CHK(d2h(h, iters, A, dit, A, A, 1, 8));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_cv_folds_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int64_t N, int64_t K, int64_t M,
                             int64_t A, const int64_t *test_idx, int64_t test_size, int64_t num_folds, int dtype, int mem, double *E,
                             int64_t *iters) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 2 || K < 1 || M < 1 || A < 1 || A > K || !X || !Y || !test_idx || !E || test_size < 1 || test_size >= N || num_folds < 1 ||
        ldx < N || ldy < N || num_folds > (1 << 22) || test_size > (1 << 20))
        return fail(h, PLS_HIP_ERR_INVALID, "bad cv_folds_missing arguments: need N>=2, 1<=A<=K, M>=1, ld>=N, 1<=test_size<N, X, Y, test_idx and E");
    if (K > (((i64)1 << 31) - 1) || M > plsk::MISS_MAX_M)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "cv_folds_missing takes at most 32 responses (and K < 2^31)");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "cv_folds_missing needs every row of X on one handle: not on a row-sharded handle");
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
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + ((-N) & 3);  // 16-byte columns for either type
        CHK(ensure(h, h->hX, (size_t)ldn * K * es));
        CHK(ensure(h, h->hY, (size_t)ldn * M * es));
        CHK(ensure(h, h->cve, (size_t)nobs * A * M * 8));
        if (iters) CHK(ensure(h, h->mit, (size_t)num_folds * A * 8));
        CHK(h2d(h, h->hX.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hY.p, ldn, Y, ldy, N, M, es));
        dX = h->hX.p; dY = h->hY.p; dE = (double *)h->cve.p;
        dit = iters ? (long long *)h->mit.p : nullptr;
        dldx = dldy = ldn;
    }
    CHK(ensure(h, h->mcvidx, (size_t)nobs * 8));
    HIPCHK(h, hipMemcpyAsync(h->mcvidx.p, test_idx, (size_t)nobs * 8, hipMemcpyHostToDevice, h->stream));
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return cv_folds_missing_device<Tx>(h, (const Tx *)dX, dldx, (const Tx *)dY, dldy, N, (int)K, (int)M, (int)A,
                                           (const long long *)h->mcvidx.p, (int)test_size, num_folds, dE, dit);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        HIPCHK(h, hipMemcpyAsync(E, dE, (size_t)nobs * A * M * 8, hipMemcpyDeviceToHost, h->stream));
        if (iters) HIPCHK(h, hipMemcpyAsync(iters, dit, (size_t)num_folds * A * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t A, const double *W, const double *P,
                           int dtype, int mem, void *S, int64_t lds) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 1 || K < 1 || A < 1 || A > K || !X || !W || !P || !S || ldx < N || lds < N)
        return fail(h, PLS_HIP_ERR_INVALID, "bad scores_missing arguments: need N>=1, 1<=A<=K, ld>=N, X, W, P and S");
    if (K > (((i64)1 << 31) - 1)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "scores_missing: K < 2^31");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "scores_missing: not on a row-sharded handle");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    const double *dW = W, *dP = P;
    void *dS = S;
    i64 dldx = ldx, dlds = lds;
    if (mem == PLS_HIP_MEM_HOST) {
        const i64 ldn = N + ((-N) & 3);
        CHK(ensure(h, h->hIn, (size_t)ldn * K * es));
        CHK(ensure(h, h->hOut, (size_t)ldn * A * es));
        CHK(ensure(h, h->hW, (size_t)K * A * 8));
        CHK(ensure(h, h->hP, (size_t)K * A * 8));
        CHK(h2d(h, h->hIn.p, ldn, X, ldx, N, K, es));
        CHK(h2d(h, h->hW.p, K, W, K, K, A, 8));
        CHK(h2d(h, h->hP.p, K, P, K, K, A, 8));
        dX = h->hIn.p; dS = h->hOut.p; dW = (const double *)h->hW.p; dP = (const double *)h->hP.p;
        dldx = dlds = ldn;
    }
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return scores_missing_device<Tx>(h, (const Tx *)dX, dldx, N, (int)K, (int)A, dW, dP, (Tx *)dS, dlds);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(d2h(h, S, lds, dS, dlds, N, A, es));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_colwise_z_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int dtype, int mem, void *Z,
                                     int64_t ldz, double *mean, double *sd, int64_t *nobs) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
    if (mem != PLS_HIP_MEM_HOST && mem != PLS_HIP_MEM_DEVICE) return fail(h, PLS_HIP_ERR_INVALID, "bad mem kind");
    if (N < 1 || K < 1 || !X || !mean || !sd || ldx < N || (Z && ldz < N))
        return fail(h, PLS_HIP_ERR_INVALID, "bad z_scores_missing arguments: need N>=1, K>=1, ld>=N, X, mean and sd");
    if (K > (((i64)1 << 31) - 1)) return fail(h, PLS_HIP_ERR_UNSUPPORTED, "z_scores_missing: K < 2^31");
    if (h->reducer || h->nranks > 1)
        return fail(h, PLS_HIP_ERR_UNSUPPORTED, "z_scores_missing: single rank only, not on a row-sharded handle");
    CHK(set_device(h));
    const size_t es = esize(dtype);
    const void *dX = X;
    void *dZ = Z;
    double *dmean = mean, *dsd = sd;
    long long *dn = (long long *)nobs;
    i64 dldx = ldx, dldz = ldz;
    if (mem == PLS_HIP_MEM_HOST) {
        CHK(ensure(h, h->hIn, (size_t)N * K * es));
        CHK(ensure(h, h->mzo, (size_t)K * 3 * 8));  // [mean, sd, nobs]
        CHK(h2d(h, h->hIn.p, N, X, ldx, N, K, es));
        dX = h->hIn.p; dZ = Z ? h->hIn.p : nullptr;  // scaled in place in the staging copy
        dmean = (double *)h->mzo.p; dsd = dmean + K; dn = nobs ? (long long *)(dsd + K) : nullptr;
        dldx = dldz = N;
    }
    CHK(by_dtype(dtype, [&](auto t) {
        using Tx = decltype(t);
        return zscores_missing_device<Tx>(h, (const Tx *)dX, dldx, N, (int)K, (Tx *)dZ, dldz, dmean, dsd, dn);
    }));
    if (mem == PLS_HIP_MEM_HOST) {
        if (Z) CHK(d2h(h, Z, ldz, dZ, dldz, N, K, es));
        CHK(d2h(h, mean, K, dmean, K, K, 1, 8));
        CHK(d2h(h, sd, K, dsd, K, K, 1, 8));
        if (nobs) CHK(d2h(h, nobs, K, dn, K, K, 1, 8));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PLS_HIP_OK;
}

int pls_hip_synth_x(pls_hip_handle h, void *X, int64_t ldx, int64_t row0, int64_t nrows, int64_t K,
                    uint64_t seed, int dtype) {
    CHK(check_handle(h));
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
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
    if (dtype != PLS_HIP_F64 && dtype != PLS_HIP_F32) return fail(h, PLS_HIP_ERR_INVALID, "bad dtype");
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

#include "xchg_ipc.hpp"

#include "group_impl.hpp"
