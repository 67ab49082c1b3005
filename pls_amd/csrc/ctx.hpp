// ctx.hpp -- the handle (pls_hip_context), its workspace buffers, status / launch-check macros, HIP-event and roctx brackets.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct Launch {
    int fam;
    i64 bytes;
    hipEvent_t e0, e1;
};

}  // namespace

struct pls_hip_context {
    int device = 0;
    hipStream_t stream = nullptr;
    pls_hip_allreduce_fn reducer = nullptr;
    void *reducer_user = nullptr;
    int rank = 0, nranks = 1;
    double *user_red = nullptr;
    i64 user_red_count = 0;
    i64 opt_algo = PLS_HIP_ALGO_KERNEL, opt_fuse = 1, opt_profile = 0, opt_power_iters = 48;
    i64 opt_fused_grid = 0, opt_work_layout = 1, opt_defer = 1, opt_graph = 0;
    // PLS_HIP_OPT_GRAPH: the last repeated device-memory fit as an executable graph (one entry: a loop of identical fits)
    std::vector<uint64_t> graph_key, graph_seen;
    hipGraphExec_t graph_exec = nullptr;
    DevBuf zeros, part, sspart, xbpart, wide1, red, red2, xx, xyp, praw, xy, v, cs, coop, lm, gxx, gxy, tab, work, cvidx, cvx, cvy, cvws, cve, cvtx, cvty, cvtt, cvm, cvkeep, cvred, hX, hY, hT, hW, hP, hQ, hR, hB, hIn, hOut;
    DevBuf valout, valpart, vale, valacc, valkeys, valhist;  // pls_hip_validation (plan_validation.hpp)
    DevBuf xdS, xdQ, xdPT, xdred, xdtv, xdoQ, xdoT, xdoS, xdsmall;  // pls_hip_x_diagnostics (plan_xdiag.hpp): scores, column-block sums, the message, tvar, host staging
    DevBuf bws, bv, bred, bmsg, bssy, bY, boR, boQ, bott, boB, bossy;  // pls_hip_fit_batch (plan_batch.hpp): per-problem workspace, V and r columns, the sliced product, the message, host staging
    DevBuf dG, dpart, dV, dT, dY, dZ, dC, dscr;  // PLS_HIP_ALGO_DUAL (plan_dual.hpp): X X^T, its split partials, [U | T / tt], the fp64 scores, Y_a, G Y_a, C, small vectors
    DevBuf dcv;  // its cross-validation folds (plan_dual_cv.hpp): the state of a round's folds
    DevBuf dbat;  // its batched fits (plan_dual_batch.hpp): the state of a round's problems
    DevBuf dcvb, cvbpos, cvbidx, cvbo, cvboE;  // pls_hip_cv_press_batch (plan_dual_cvbatch.hpp): the state of a round's items, pos of every fold, the test rows, host staging of [PRESS | ssy] and of E
    DevBuf rsw, rsB, rsacc, rsX, rsY, rsW, rsoS;  // pls_hip_fit_resampled (plan_resample.hpp): the state of a round's replicates (general route: of one fit), a round's B, [s1, s2, B0], the row-scaled work copies, host staging of the weights and of [B0, Bmean, Bm2]
    DevBuf mX, mws, mit, mzo;  // pls_hip_fit_missing and its companions (plan_missing.hpp): the work copy of X, vectors and partials, host staging of iters and of [mean, sd, nobs]
    DevBuf mcv, mcvidx;  // pls_hip_cv_folds_missing (plan_missing_cv.hpp): the slabs of a round's folds (miss_layout.hpp) and the round's word, the test rows (iters are staged in mit)
    DevBuf xmws, xmon;  // pls_hip_x_diagnostics_missing (plan_xdiag_missing.hpp): scores, Q columns, range partials and slices (xdiagmiss_layout.hpp), host staging of nobs
    DevBuf vdST, vdpart, vdred, vdsm;  // pls_hip_var_diagnostics (plan_vardiag.hpp): the row-contiguous scores, the row splits' partials of a range, the message, [||w||^2 | ssy | sst]
    i64 opt_missing_iters = 500;  // PLS_HIP_OPT_MISSING_ITERS
    int *mconv_host = nullptr;    // pinned: where the host reads the convergence word of the M > 1 loop
    i64 opt_val_lds_rows = -1;  // PLS_HIP_OPT_VALIDATION_LDS_ROWS; -1 = the device's own limit
    i64 val_lds_rows_dev = -1;  // that limit, found on first use
    std::string err;
    // profiling
    std::vector<hipEvent_t> ev_pool;  // grows until pls_hip_get_timing harvests and recycles it
    size_t ev_used = 0;
    std::vector<Launch> launches;     // every bracketed launch since the last harvest
    std::vector<Launch> fits;         // one bracket per pls_hip_fit since the last harvest
    Launch cur_fit{};
    bool fit_timed = false;
    int num_cu = 256;
    // host <-> device staging (host_pipeline.hpp): pinned double buffer + copy threads, created on first large transfer
    plsh::Stager stager;
    int copy_threads = 0;  // 0 = default (PLS_HIP_COPY_THREADS or min(16, cores/2))
    hipStream_t copy_stream = nullptr;  // transfers that run beside kernels of `stream` (upload_accumulate)
    // X^T X (K x K) and X^T Y (K x M) of THIS member's rows, already formed while the rows were uploaded
    // (upload_accumulate): a fit that may use the Gram plan takes them instead of two passes over X
    const double *pre_xx = nullptr, *pre_xy = nullptr;
    // Members of a group: workspace that has to grow is not freed on the spot -- hipFree waits for the whole DEVICE, and a
    // member that shares its GPU with others (virtual shards) would wait for a peer's exchange kernel that in turn waits for
    // this member's next collective.  The old blocks are released when no member is running (run_members).
    bool defer_free = false;
    std::vector<void *> graveyard;
    // cross-process device-side exchange (pls_hip_xchg_*, exchange_kernels.hpp)
    struct XchgIpc *xchg = nullptr;
    // This member's view of the device-side exchange it belongs to, whoever owns the inboxes (XchgIpc: one process per
    // GPU; pls_hip_group: the members of one process).  With it the per-component collective of a fused fit is not a
    // call of the reducer: the push rides in the tail of the pass, the gather is the prologue of the component update.
    struct XchgEndpoint {
        bool on = false;
        int n = 0, rank = 0;
        double *const *inbox = nullptr;             // [n] the members' inboxes (peer-visible addresses)
        unsigned long long *const *flags = nullptr;  // [n] their flags
        unsigned long long *seq = nullptr;           // this member's running collective number
        int *status = nullptr, *host_status = nullptr;
        const long long *limit = nullptr;
    } xep;
    DevBuf tailcnt;  // arrival counters of slice_tail (fused_kernels.hpp)
    DevBuf resident;  // resident_fit_kernel: two arrival counters (256 bytes) + [2][G][LP] partial vectors
    DevBuf rgflags;   // resident_gram_fit_kernel: one arrival word per workgroup (1 KB), values grow from launch to launch
    unsigned rg_epoch = 0;
    unsigned long long resident_launches = 0;
    // The environment switches of the library, read ONCE when the handle is created (INTEGRATION.md lists them):
    //   PLS_HIP_TINY=0           small fits on the general plan instead of the single-launch kernels (tests compare the two)
    //   PLS_HIP_CV_REFIT=1       pls_hip_cv_folds as one device refit per fold (the general form; tests compare)
    //   PLS_HIP_TAIL=0           partial rows summed by reduce_partials_kernel behind the pass, sharded collectives through
    //                            the reducer call (the launches of round 3; A/B measurements)
    //   PLS_HIP_TAIL=1 / 2       the one-response update as the last act of the tail -- ONE launch per component, sharded over
    //                            the device-side exchange as well (push, wait for the peers, update) -- never (1) / behind every
    //                            pass (2).  Default (unset): behind READ-ONLY passes only; behind a deflating sweep the tail's loads
    //                            queue behind the write drain and the update is faster as a launch of its own
    //                            (profiles/r5/tail_ab.txt)
    //   PLS_HIP_BATCH_REFIT=1    pls_hip_fit_batch as one KERNEL_TYPE2 fit per problem (the general form; tests compare)
    //   PLS_HIP_BATCH_ROUND=n    at most n problems per round of pls_hip_fit_batch's batched route (tests: several rounds)
    //   PLS_HIP_DUALCV_ROUND=n   at most n folds per round of pls_hip_cv_folds under PLS_HIP_ALGO_DUAL (tests: several rounds)
    //   PLS_HIP_DUALBATCH_ROUND=n  at most n problems per round of pls_hip_fit_batch under PLS_HIP_ALGO_DUAL (tests: several rounds)
    //   PLS_HIP_DUALBATCH_SWEEPS=1 its back-projection beyond 64 columns as one sweep of dual_xtv_kernel per 64 columns instead
    //                            of one launch of dual_xtvb_kernel (A/B measurements; tests compare)
    //   PLS_HIP_RESAMPLE_REFIT=1 pls_hip_fit_resampled as one KERNEL_TYPE1 fit per replicate on row-scaled copies (the general form;
    //                            tests compare)
    //   PLS_HIP_RESAMPLE_ROUND=n at most n replicates per round of pls_hip_fit_resampled under PLS_HIP_ALGO_DUAL (tests: several rounds)
    //   PLS_HIP_CVBATCH_REFIT=1  pls_hip_cv_press_batch as one pls_hip_cv_folds plus the PRESS kernels of pls_hip_validation per
    //                            problem (the general form; tests compare)
    //   PLS_HIP_DUALCVB_ROUND=n  at most n (problem, fold) pairs per round of pls_hip_cv_press_batch under PLS_HIP_ALGO_DUAL
    //                            (tests: several rounds)
    //   PLS_HIP_MISSCV_ROUND=n   at most n folds per round of pls_hip_cv_folds_missing (tests: several rounds)
    //   PLS_HIP_XDIAGMISS_ROUTE=stream  pls_hip_x_diagnostics_missing on its streaming route whatever the shape (the cross-check of
    //                            the row-resident route; tests compare)
    //   PLS_HIP_RESIDENT=0       mid-size single-response fits on the general plan instead of the one-launch resident fit
    //   PLS_HIP_REPLICA_GUARD=0  no replica-divergence check after a sharded fit (must be the same on every rank)
    //   PLS_HIP_TURNAROUND=0     every fused pass walks ascending with the nt policy throughout (A/B measurements; must be the
    //                            same on every rank)
    struct Env {
        bool turnaround = true;
        i64 turn_edge_bytes = plsk::TURN_EDGE_BYTES;  // (testing build: PLS_HIP_TEST_TURN_EDGE_BYTES)
        bool batch_refit = false;
        i64 batch_round = 0;
        i64 dualcv_round = 0;
        i64 dualbatch_round = 0;
        i64 resample_round = 0;
        bool resample_refit = false;
        bool dualbatch_sweeps = false;
        bool cvbatch_refit = false;
        i64 dualcvb_round = 0;
        i64 misscv_round = 0;
        bool xdiagmiss_stream = false;
        bool tiny = true, cv_refit = false, tail = true, replica_guard = true, resident = true;
        int tail_update = 1;  // 0: never, 1: in the tail of READ-ONLY passes (default), 2: of every pass
        int xb4 = 1;          // PLS_HIP_XB4=0: X B with 5..32 columns on the older kernels
        int resident_gram = 1;  // PLS_HIP_RESIDENT_GRAM=0: AUTO's mid-size fits on the per-component resident kernels; 2: also under KERNEL (measurements); 4: the row form of its first phase everywhere
    };
    static void read_env(Env &env) {  // (pls_hip_create)
        auto off = [](const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; };
        auto on = [](const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; };
        auto num = [](const char *name, i64 &v) { if (const char *e = getenv(name)) v = atoll(e); };
        env.tiny = !off("PLS_HIP_TINY");
        env.cv_refit = on("PLS_HIP_CV_REFIT");
        env.batch_refit = on("PLS_HIP_BATCH_REFIT");
        num("PLS_HIP_BATCH_ROUND", env.batch_round);
        num("PLS_HIP_DUALCV_ROUND", env.dualcv_round);
        num("PLS_HIP_DUALBATCH_ROUND", env.dualbatch_round);
        num("PLS_HIP_RESAMPLE_ROUND", env.resample_round);
        env.resample_refit = on("PLS_HIP_RESAMPLE_REFIT");
        env.dualbatch_sweeps = on("PLS_HIP_DUALBATCH_SWEEPS");
        env.cvbatch_refit = on("PLS_HIP_CVBATCH_REFIT");
        num("PLS_HIP_DUALCVB_ROUND", env.dualcvb_round);
        num("PLS_HIP_MISSCV_ROUND", env.misscv_round);
        if (const char *e = getenv("PLS_HIP_XDIAGMISS_ROUTE")) env.xdiagmiss_stream = std::strcmp(e, "stream") == 0;
        env.tail = !off("PLS_HIP_TAIL");
        const char *tail = getenv("PLS_HIP_TAIL");
        env.tail_update = tail ? (atoi(tail) >= 2 ? 2 : 0) : 1;
        env.replica_guard = !off("PLS_HIP_REPLICA_GUARD");
        env.resident = !off("PLS_HIP_RESIDENT");
        env.turnaround = !off("PLS_HIP_TURNAROUND");
#ifdef PLS_HIP_TESTING
        num("PLS_HIP_TEST_TURN_EDGE_BYTES", env.turn_edge_bytes);  // (small matrices with a bulk, tests only)
#endif
        if (const char *e = getenv("PLS_HIP_XB4")) env.xb4 = atoi(e);
        if (const char *e = getenv("PLS_HIP_RESIDENT_GRAM")) env.resident_gram = atoi(e);
    }
    Env env;
    // replica guard of sharded fits (small_kernels.hpp): host-mapped flag "the ranks derived different W/P/Q/R/B"
    int *diverged = nullptr, *diverged_dev = nullptr;
    DevBuf guard;
#ifdef PLS_HIP_TESTING
    int poison_new = -1;  // testing/libpls_hip.so: ensure() fills every fresh block with this byte (pls_hip_test_poison_workspace); -1: off
#endif
};

// ---- the workspaces of a handle: ONE list -------------------------------------------------------------------------------------
// Every DevBuf member of pls_hip_context, once (tests/test_workspace_list.py holds the struct and the list to each other).
// pls_hip_destroy frees from this list, pls_hip_test_poison_workspace of the testing build fills from it.
//   SCRATCH(name)                 nothing in it outlives the call that wrote it: a call writes whatever it reads, so the bits it
//                                 returns cannot depend on what an earlier call left there (tests/test_gpu_history.py fills these
//                                 with 0xFF / 0x7F / 0x01 between calls)
//   STATEFUL(name, keep, reason)  the first `keep` bytes (WS_ALL: the whole buffer; an expression of the handle c) carry state
//                                 from call to call ON PURPOSE, for the reason given; INTEGRATION.md section K repeats the reasons
#define PLS_HIP_WORKSPACES(SCRATCH, STATEFUL)                                                                                        \
    STATEFUL(zeros, WS_ALL, "256 zero bytes, cleared once when first used and only read afterwards: the source of out-of-range rows of the LDS-DMA panels") \
    STATEFUL(resident, 256, "two arrival counters of the resident fits, used in alternating parity (resident_launches): each launch zeroes the counter of the next; the payload behind the 256 bytes is scratch") \
    STATEFUL(rgflags, WS_ALL, "one arrival word per workgroup of resident_gram_fit_kernel: values only grow, a launch waits for words beyond rg_epoch, which the host advances by 4 per launch") \
    STATEFUL(gxx, c->pre_xx ? WS_ALL : 0, "X^T X accumulated during an upload, only while pre_xx points into it: from upload_accumulate to the end of the same host-memory fit") \
    STATEFUL(gxy, c->pre_xy ? WS_ALL : 0, "X^T Y accumulated during an upload, only while pre_xy points into it: from upload_accumulate to the end of the same host-memory fit") \
    SCRATCH(tailcnt) SCRATCH(part) SCRATCH(sspart) SCRATCH(xbpart) SCRATCH(wide1) SCRATCH(red) SCRATCH(red2) SCRATCH(xx) SCRATCH(xyp)  \
    SCRATCH(praw) SCRATCH(xy) SCRATCH(v) SCRATCH(cs) SCRATCH(coop) SCRATCH(lm) SCRATCH(tab) SCRATCH(work)                              \
    SCRATCH(cvidx) SCRATCH(cvx) SCRATCH(cvy) SCRATCH(cvws) SCRATCH(cve) SCRATCH(cvtx) SCRATCH(cvty) SCRATCH(cvtt) SCRATCH(cvm)         \
    SCRATCH(cvkeep) SCRATCH(cvred)                                                                                                     \
    SCRATCH(hX) SCRATCH(hY) SCRATCH(hT) SCRATCH(hW) SCRATCH(hP) SCRATCH(hQ) SCRATCH(hR) SCRATCH(hB) SCRATCH(hIn) SCRATCH(hOut)         \
    SCRATCH(valout) SCRATCH(valpart) SCRATCH(vale) SCRATCH(valacc) SCRATCH(valkeys) SCRATCH(valhist)                                   \
    SCRATCH(xdS) SCRATCH(xdQ) SCRATCH(xdPT) SCRATCH(xdred) SCRATCH(xdtv) SCRATCH(xdoQ) SCRATCH(xdoT) SCRATCH(xdoS) SCRATCH(xdsmall)    \
    SCRATCH(bws) SCRATCH(bv) SCRATCH(bred) SCRATCH(bmsg) SCRATCH(bssy) SCRATCH(bY) SCRATCH(boR) SCRATCH(boQ) SCRATCH(bott)             \
    SCRATCH(boB) SCRATCH(bossy)                                                                                                        \
    SCRATCH(dG) SCRATCH(dpart) SCRATCH(dV) SCRATCH(dT) SCRATCH(dY) SCRATCH(dZ) SCRATCH(dC) SCRATCH(dscr) SCRATCH(dcv) SCRATCH(dbat)    \
    SCRATCH(dcvb) SCRATCH(cvbpos) SCRATCH(cvbidx) SCRATCH(cvbo) SCRATCH(cvboE)                                                         \
    SCRATCH(rsw) SCRATCH(rsB) SCRATCH(rsacc) SCRATCH(rsX) SCRATCH(rsY) SCRATCH(rsW) SCRATCH(rsoS)                                      \
    SCRATCH(mX) SCRATCH(mws) SCRATCH(mit) SCRATCH(mzo) SCRATCH(mcv) SCRATCH(mcvidx)                                                    \
    SCRATCH(xmws) SCRATCH(xmon)                                                                                                        \
    SCRATCH(vdST) SCRATCH(vdpart) SCRATCH(vdred) SCRATCH(vdsm)                                                                         \
    SCRATCH(guard)

namespace {

constexpr size_t WS_ALL = ~(size_t)0;

// f(DevBuf &, keep) for every workspace of the list; keep = the leading bytes that carry state (0 for scratch)
template <typename F>
void for_each_workspace(pls_hip_context *c, F &&f) {
#define PLS_HIP_WS_SCRATCH(name) f(c->name, (size_t)0);
#define PLS_HIP_WS_STATEFUL(name, keep, reason) f(c->name, (size_t)(keep));
    PLS_HIP_WORKSPACES(PLS_HIP_WS_SCRATCH, PLS_HIP_WS_STATEFUL)
#undef PLS_HIP_WS_SCRATCH
#undef PLS_HIP_WS_STATEFUL
}

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);               \
            return PLS_HIP_ERR_DEVICE;                                                     \
        }                                                                                  \
    } while (0)

#define CHK(expr)                      \
    do {                               \
        int rc__ = (expr);             \
        if (rc__ != PLS_HIP_OK) return rc__; \
    } while (0)

int fail(pls_hip_context *c, int code, const std::string &msg) {
    c->err = msg;
    return code;
}

int ensure(pls_hip_context *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.bytes && b.p) return PLS_HIP_OK;
    if (b.p) {
        if (c->defer_free) {
            c->graveyard.push_back(b.p);
        } else {
            HIPCHK(c, hipStreamSynchronize(c->stream));  // earlier launches may still read it
            HIPCHK(c, hipFree(b.p));
        }
        b.p = nullptr;
        b.bytes = 0;
    }
    bytes = std::max<size_t>(bytes, 256);
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(c, PLS_HIP_ERR_ALLOC, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    b.bytes = bytes;
#ifdef PLS_HIP_TESTING
    if (c->poison_new >= 0) {  // a fresh block is arbitrary and usually zero: the tests want it as hostile as a stale one
        HIPCHK(c, hipMemsetAsync(b.p, c->poison_new, bytes, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (the block may be written next from the copy stream)
    }
#endif
    return PLS_HIP_OK;
}

size_t esize(int dtype) { return dtype == PLS_HIP_F64 ? 8 : 4; }

// ---- profiling ------------------------------------------------------------------------
hipEvent_t take_event(pls_hip_context *c) {
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_used++];
}
struct Scope {  // brackets one launch with events when profiling is on
    pls_hip_context *c;
    Launch l{};
    bool on;
    // profile level 1 brackets only the streaming kernels over X (the K-sized bookkeeping kernels
    // run unbracketed, so that event records do not widen the gaps of the A-loop); level 2: all
    Scope(pls_hip_context *ctx, int fam, i64 bytes)
        : c(ctx), on(ctx->opt_profile >= 2 || (ctx->opt_profile == 1 && fam != PLS_HIP_FAM_SMALL)) {
        if (!on) return;
        l.fam = fam;
        l.bytes = bytes;
        l.e0 = take_event(c);
        l.e1 = take_event(c);
        if (!l.e0 || !l.e1) { on = false; return; }
        (void)hipEventRecord(l.e0, c->stream);
    }
    ~Scope() {
        if (!on) return;
        (void)hipEventRecord(l.e1, c->stream);
        c->launches.push_back(l);
    }
};

// ---- tracing: roctx ranges around the phases of a fit -----------------------------------------------------
// The reference has no tracing.  With PLS_HIP_ROCTX=1 in the environment every fit is wrapped
// in roctx ranges -- "pls_hip_fit", "X^T Y", "X^T X (SYRK)", "component a", "upload" -- which `rocprofv3 --marker-trace`
// shows next to the kernels.  The marker library (librocprofiler-sdk-roctx.so) is looked up at run time: the product
// has no link-time dependency on it and the ranges cost nothing when the switch is off.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char *e = getenv("PLS_HIP_ROCTX");
        if (!e || atoi(e) == 0) return;
        void *lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return;
        push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        if (!push || !pop) push = nullptr;
    }
};
inline Roctx &roctx() {
    static Roctx r;
    return r;
}
struct Range {  // RAII range; `text` must outlive the call only
    bool on;
    explicit Range(const char *text) : on(roctx().push != nullptr) {
        if (on) roctx().push(text);
    }
    Range(const char *prefix, int n) : on(roctx().push != nullptr) {
        if (on) {
            char buf[64];
            std::snprintf(buf, sizeof(buf), "%s %d", prefix, n);
            roctx().push(buf);
        }
    }
    ~Range() {
        if (on) roctx().pop();
    }
};

#define LAUNCH_CHECK(ctx)                                                           \
    do {                                                                            \
        hipError_t e__ = hipGetLastError();                                         \
        if (e__ != hipSuccess) {                                                    \
            (ctx)->err = std::string("kernel launch: ") + hipGetErrorString(e__);   \
            return PLS_HIP_ERR_DEVICE;                                              \
        }                                                                           \
    } while (0)

}  // namespace
