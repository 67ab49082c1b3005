// host_entry.hpp -- argument checks the entries share, fit timing brackets, host <-> device staging (h2d, d2h, the leading-dimension
// rules, HostCall and the table of what every entry stages where) and the upload that accumulates X^T X / X^T Y on the way.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

int check_handle(pls_hip_handle h) { return h ? PLS_HIP_OK : PLS_HIP_ERR_INVALID; }
int check_dtype(pls_hip_context *c, int dtype) {
    return dtype == PLS_HIP_F64 || dtype == PLS_HIP_F32 ? PLS_HIP_OK : fail(c, PLS_HIP_ERR_INVALID, "bad dtype");
}
int check_mem(pls_hip_context *c, int mem) {
    return mem == PLS_HIP_MEM_HOST || mem == PLS_HIP_MEM_DEVICE ? PLS_HIP_OK : fail(c, PLS_HIP_ERR_INVALID, "bad mem kind");
}
// an entry that needs every row of X on one handle; `why` is its own wording of that
int check_unsharded(pls_hip_context *c, const char *why) {
    return c->reducer || c->nranks > 1 ? fail(c, PLS_HIP_ERR_UNSUPPORTED, why) : PLS_HIP_OK;
}
// the held-out rows of the cv entries: every one of the n indices in [0, rows)
int check_test_idx(pls_hip_context *c, const int64_t *test_idx, i64 n, i64 rows, const char *entry) {
    for (i64 j = 0; j < n; ++j)
        if (test_idx[j] < 0 || test_idx[j] >= rows) return fail(c, PLS_HIP_ERR_INVALID, std::string(entry) + ": test index out of range");
    return PLS_HIP_OK;
}

int set_device(pls_hip_context *c) {
    HIPCHK(c, hipSetDevice(c->device));
    return PLS_HIP_OK;
}

void begin_fit_timing(pls_hip_context *c) {
    c->fit_timed = false;
    if (!c->opt_profile) return;
    c->cur_fit.e0 = take_event(c);
    c->cur_fit.e1 = take_event(c);
    if (c->cur_fit.e0 && c->cur_fit.e1) {
        (void)hipEventRecord(c->cur_fit.e0, c->stream);
        c->fit_timed = true;
    }
}
void end_fit_timing(pls_hip_context *c) {
    if (!c->fit_timed) return;
    (void)hipEventRecord(c->cur_fit.e1, c->stream);
    c->fits.push_back(c->cur_fit);
    c->fit_timed = false;
}

// host <-> device staging of a column-major matrix with leading dimension.  Matrices of a few MB and more go
// through the pinned double-buffer pipeline of host_pipeline.hpp (the caller's pageable memory is repacked by host
// threads while the DMA engine moves the previous tile); small ones are one plain copy.
constexpr size_t PIPELINE_MIN_BYTES = (size_t)4 << 20;
int h2d(pls_hip_context *c, void *dst, i64 ldd, const void *src, i64 lds, i64 rows, i64 cols, size_t es) {
    if (rows == 0 || cols == 0) return PLS_HIP_OK;
    if ((size_t)rows * (size_t)cols * es >= PIPELINE_MIN_BYTES) {
        HIPCHK(c, c->stager.ensure(c->copy_threads > 0 ? c->copy_threads : plsh::default_copy_threads(), c->device));
        HIPCHK(c, plsh::upload(c->stager, c->stream, dst, ldd, src, lds, rows, cols, es));
        return PLS_HIP_OK;
    }
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)ldd * es, src, (size_t)lds * es, (size_t)rows * es,
                               (size_t)cols, hipMemcpyHostToDevice, c->stream));
    return PLS_HIP_OK;
}
int d2h(pls_hip_context *c, void *dst, i64 ldd, const void *src, i64 lds, i64 rows, i64 cols, size_t es) {
    if (rows == 0 || cols == 0) return PLS_HIP_OK;
    if ((size_t)rows * (size_t)cols * es >= PIPELINE_MIN_BYTES) {
        HIPCHK(c, c->stager.ensure(c->copy_threads > 0 ? c->copy_threads : plsh::default_copy_threads(), c->device));
        HIPCHK(c, plsh::download(c->stager, c->stream, dst, ldd, src, lds, rows, cols, es));
        return PLS_HIP_OK;
    }
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)ldd * es, src, (size_t)lds * es, (size_t)rows * es,
                               (size_t)cols, hipMemcpyDeviceToHost, c->stream));
    return PLS_HIP_OK;
}

// ---- staging of a host-memory call ------------------------------------------------------------------------------------------
// The leading dimension a matrix of n rows is staged with.  The rule feeds vec_ok / cols_aligned of the routes and through them
// the kernel and the bits, so every entry keeps the rule it was written with:
i64 ld_even(i64 n) { n = std::max<i64>(n, 1); return n + (n & 1); }      // 16-byte columns of fp64
i64 ld_quad(i64 n) { n = std::max<i64>(n, 1); return n + ((-n) & 3); }   // 16-byte columns of either type
i64 ld_exact(i64 n) { return n; }                                         // packed
//
//   entry                      rule   staged inputs                      staged outputs                              guard
//   pls_hip_fit                even   hX hY                              hW hP hR hQ hB hT                           yes
//   pls_hip_coefficients       -      hR hQ                              hB                                          no
//   pls_hip_xb                 even   hIn hB                             hOut                                        no
//   pls_hip_model_sse          even   hIn hY hR hQ                       hB (SSE; the scores stay in hOut)           no
//   pls_hip_x_diagnostics      even   hIn hR hP xdsmall[tvar]            xdoQ xdoT xdoS xdsmall[ssx | sst]           no
//   pls_hip_cv_folds           quad   hX hY                              cve (flat)                                  no, sync for device memory too
//   cv_folds_sharded           quad   hX hY                              cve (flat)                                  yes, for device memory too
//   fit_batch_impl             quad   hX bY                              boR boQ bott boB bossy                      yes
//   fit_resampled_impl         quad   hX hY rsW (exact)                  boQ bott boB rsoS[B0 | Bmean | Bm2]         yes
//   cv_press_batch_impl        quad   hX bY                              cvbo[PRESS | ssy] cvboE                     no, sync for device memory too
//   validation_impl            -      vale (its own piecewise upload)    valout[PRESS | D | probw | ref] (flat)      no
//   pls_hip_fit_missing        quad   hX hY                              hW hP hR hQ hB hT mit                       no
//   pls_hip_cv_folds_missing   quad   hX hY                              cve mit (flat)                              no (its plan synchronises for either memory)
//   pls_hip_scores_missing     quad   hIn hW hP                          hOut                                        no
//   pls_hip_x_diagnostics_missing  quad  hIn hW hP xdsmall[tvar]      xdoQ xdoT xdoS xdsmall[ssx | sst] xmon      no
//   pls_hip_colwise_z_scores_missing  exact  hIn                         hIn (Z, in place) mzo[mean | sd | nobs]     no
//
// guard = check_diverged() behind the synchronisation.  The index list of the cv entries is the caller's host memory for either
// kind of `mem`, which is why they synchronise always.  The buffer names are an interface: a device-memory call leaves every one
// of them alone (but hOut, the scores of pls_hip_model_sse, and cve, which pls_hip_cv_folds sizes for either memory), and
// group_impl.hpp relies on that -- pls_hip_group_xb stages B in hB, pls_hip_group_model_sse R, Q and the SSE in hR, hQ, hB, the
// fit of a group has its members write W .. B to hW .. hB -- around device-memory calls of the entries above.
//
// HostCall: in() per staged input, out() per staged output in the order the copies back are to be issued, finish() behind the work.
// With device memory every call leaves the pointers as they are.  A matrix may share its buffer with others: `total` bytes for
// all of them (0: the matrix alone), this one `off` bytes into it.
struct HostCall {
    pls_hip_context *c;
    const bool host;
    struct Copy {
        void *dst;
        const void *src;
        i64 ldd, lds, rows, cols;  // flat: rows = bytes
        size_t es;                 // 0: flat, one hipMemcpyAsync
    };
    static constexpr int MAX_COPIES = 8;
    Copy copies[MAX_COPIES];
    int n = 0;
    HostCall(pls_hip_context *ctx, int mem) : c(ctx), host(mem == PLS_HIP_MEM_HOST) {}

    // dev, ldd = where a matrix of `cols` columns is staged (nothing is copied)
    template <typename P>
    int place(P *&dev, i64 &ldd, DevBuf &buf, i64 cols, size_t es, i64 ld_staged, size_t total = 0, size_t off = 0) {
        if (!host) return PLS_HIP_OK;
        CHK(ensure(c, buf, total ? total : (size_t)ld_staged * cols * es));
        dev = (P *)((char *)buf.p + off);
        ldd = ld_staged;
        return PLS_HIP_OK;
    }
    // input: rows x cols of `es` bytes at `src` (leading dimension lds), uploaded by h2d
    template <typename P>
    int in(P *&dev, i64 &ldd, const void *src, i64 lds, DevBuf &buf, i64 rows, i64 cols, size_t es, i64 ld_staged, size_t total = 0,
           size_t off = 0) {
        if (!host) return PLS_HIP_OK;
        CHK(place(dev, ldd, buf, cols, es, ld_staged, total, off));
        return h2d(c, (void *)dev, ldd, src, lds, rows, cols, es);
    }
    template <typename P>  // ... packed on both sides
    int in(P *&dev, const void *src, DevBuf &buf, i64 rows, i64 cols, size_t es = 8, size_t total = 0, size_t off = 0) {
        i64 ld = rows;
        return in(dev, ld, src, rows, buf, rows, cols, es, rows, total, off);
    }
    // records the copy back of rows x cols from dev to dst (null: not asked for), by d2h
    int back(void *dst, i64 ldd, const void *dev, i64 lds, i64 rows, i64 cols, size_t es) {
        if (!host || !dst) return PLS_HIP_OK;
        if (n == MAX_COPIES) return fail(c, PLS_HIP_ERR_INVALID, "internal: more staged outputs than HostCall holds");
        copies[n++] = {dst, dev, ldd, lds, rows, cols, es};
        return PLS_HIP_OK;
    }
    // output: dev = where the kernels write it (null: dst is null, not asked for), copied back by finish()
    template <typename P>
    int out(P *&dev, i64 &ldd, void *dst, i64 ld_dst, DevBuf &buf, i64 rows, i64 cols, size_t es, i64 ld_staged, size_t total = 0,
            size_t off = 0) {
        if (!host) return PLS_HIP_OK;
        dev = nullptr;
        if (!dst) return PLS_HIP_OK;
        CHK(place(dev, ldd, buf, cols, es, ld_staged, total, off));
        return back(dst, ld_dst, dev, ldd, rows, cols, es);
    }
    template <typename P>  // ... packed on both sides
    int out(P *&dev, void *dst, DevBuf &buf, i64 rows, i64 cols, size_t es = 8, size_t total = 0, size_t off = 0) {
        i64 ld = rows;
        return out(dev, ld, dst, rows, buf, rows, cols, es, rows, total, off);
    }
    // the flat flavour: `bytes` in one hipMemcpyAsync, for what never went through the pipeline of d2h
    int back_flat(void *dst, const void *dev, size_t bytes) { return back(dst, 0, dev, 0, (i64)bytes, 1, 0); }
    template <typename P>
    int out_flat(P *&dev, void *dst, DevBuf &buf, size_t bytes) {
        if (!host) return PLS_HIP_OK;
        dev = nullptr;
        if (!dst) return PLS_HIP_OK;
        CHK(ensure(c, buf, bytes));
        dev = (P *)buf.p;
        return back_flat(dst, dev, bytes);
    }
    // Behind the work, and only when it succeeded: the copies back in the order recorded, the synchronisation of a host-memory call
    // (sync_device: of a device-memory call too), then, where asked, the replica-divergence flag
    int finish(bool check_guard = false, bool sync_device = false) {
        for (int i = 0; i < n; ++i) {
            const Copy &o = copies[i];
            if (o.es)
                CHK(d2h(c, o.dst, o.ldd, o.src, o.lds, o.rows, o.cols, o.es));
            else
                HIPCHK(c, hipMemcpyAsync(o.dst, o.src, (size_t)o.rows, hipMemcpyDeviceToHost, c->stream));
        }
        if (!host && !sync_device) return PLS_HIP_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return check_guard ? check_diverged(c) : PLS_HIP_OK;
    }
};

// Upload of X (host, rows x K) in ROW blocks with X^T X and X^T Y accumulated block by block on the compute stream
// while the DMA engine already moves the next block: the matrix-core SYRK of a block (2 rb K^2 flops) takes a
// fraction of the block's PCIe time (K * 2e-4 of it), so by the time the last rows have arrived the Gram matrix of
// the whole shard is complete and a Gram-plan fit needs no further pass over X for its component loop.
// dY: the member's rows of Y, already on the device.  *ok = false: the layout does not allow it (plain upload done).
template <typename T>
int upload_accumulate(pls_hip_context *c, T *dX, i64 ldd, const T *hX, i64 ldx, i64 N, int K, const T *dY, i64 ldy,
                      int M, double *XXacc, double *XYacc, bool *ok) {
    constexpr int FV = 16 / sizeof(T);
    const size_t es = sizeof(T);
    *ok = false;
    const i64 KK = (i64)K * K, L0 = (i64)K * M;
    i64 rb = (i64)(plsh::STAGE_BYTES / ((size_t)K * es)) & ~(i64)63;
    const int nbk = (K + plsk::SYRK_TB - 1) / plsk::SYRK_TB;
    const i64 S = std::max<i64>(1, (2 * (i64)c->num_cu) / (nbk * (nbk + 1) / 2));
    if (N < 1 || K > 4096 || M > plsk::LM_MAX || rb < 64 || !plsk::vec_ok((uintptr_t)dX, ldd, sizeof(T), FV) || !plsk::vec_ok((uintptr_t)dY, ldy, sizeof(T), FV) ||
        ensure(c, c->red2, (size_t)plsk::RED_SLICES * KK * 8) != PLS_HIP_OK ||
        ensure(c, c->part, std::max<size_t>((size_t)S * KK, (size_t)max_partial_rows(c, rb, K) * L0) * 8) != PLS_HIP_OK ||
        ensure(c, c->red, (size_t)plsk::RED_SLICES * std::max<i64>(L0, K + 1) * 8) != PLS_HIP_OK) {
        c->err.clear();
        return h2d(c, dX, ldd, hX, ldx, N, K, es);
    }
    HIPCHK(c, c->stager.ensure(c->copy_threads > 0 ? c->copy_threads : plsh::default_copy_threads(), c->device));
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->zeros.p) {
        CHK(ensure(c, c->zeros, 256));
        HIPCHK(c, hipMemsetAsync(c->zeros.p, 0, 256, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(XXacc, 0, (size_t)KK * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(XYacc, 0, (size_t)L0 * 8, c->stream));
    plsh::Stager &st = c->stager;
    double *part = (double *)c->part.p, *red2 = (double *)c->red2.p, *red = (double *)c->red.p;
    bool acc = true;
    Range r_up("upload + X^T X / X^T Y accumulation");
    for (i64 r0 = 0; r0 < N; r0 += rb) {
        const i64 rbn = std::min(rb, N - r0);
        const int s = st.slot;
        if (st.busy[s]) HIPCHK(c, hipEventSynchronize(st.ev[s]));
        plsh::repack(*st.pool, (char *)st.buf[s], (char *)const_cast<T *>(hX), ldx, r0, 0, rbn, K, es, true);
        HIPCHK(c, hipMemcpy2DAsync(dX + r0, (size_t)ldd * es, st.buf[s], (size_t)rbn * es, (size_t)rbn * es, (size_t)K,
                                   hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipEventRecord(st.ev[s], c->copy_stream));
        st.busy[s] = true;
        st.slot ^= 1;
        HIPCHK(c, hipStreamWaitEvent(c->stream, st.ev[s], 0));  // kernels of this block (and of the fit) after its rows
        if (!acc) continue;
        int nb = 0;
        if (plsk::launch_syrk<T>(c->stream, c->num_cu, dX + r0, ldd, rbn, K, part, S * KK, &nb, c->zeros.p) != 0) {
            acc = false;  // ragged block the matrix-core kernel declines: the fit forms X^T X itself
            continue;
        }
        LAUNCH_CHECK(c);
        CHK(launch_reduce(c, part, nb, (int)KK, nullptr, 0, red2));
        hipLaunchKernelGGL(plsk::accumulate_slices_kernel, dim3((unsigned)((KK + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                           c->stream, (const double *)red2, (int)KK, XXacc);
        LAUNCH_CHECK(c);
        CHK(launch_xty<T>(c, dX + r0, ldd, dY + r0, ldy, rbn, K, M, part, &nb));
        CHK(launch_reduce(c, part, nb, (int)L0, nullptr, 0, red));
        hipLaunchKernelGGL(plsk::accumulate_slices_kernel, dim3((unsigned)((L0 + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                           c->stream, (const double *)red, (int)L0, XYacc);
        LAUNCH_CHECK(c);
    }
    *ok = acc;
    return PLS_HIP_OK;
}

// The upload of X in a host-memory pls_hip_fit, to dX with leading dimension ldn (dY: the staged Y, the same ldn).  A plan that
// works from X^T X (AUTO, GRAM, KERNEL_TYPE2) gets it for free: accumulated on the matrix cores row block by row block while X
// crosses PCIe (upload_accumulate).  Single rank only: the ranks of a sharded fit must not differ in their plan.
// Sets pre_xx / pre_xy when the sums are there; the fit clears them on every way out.
int upload_fit_x(pls_hip_context *h, void *dX, const void *dY, i64 ldn, const void *X, i64 ldx, i64 N, int K, int M, int A, int method,
                 int dtype) {
    const size_t es = esize(dtype);
    bool pre = false;
    const bool wants_gram = h->opt_algo == PLS_HIP_ALGO_AUTO || h->opt_algo == PLS_HIP_ALGO_GRAM || method == PLS_HIP_KERNEL_TYPE2;
    const bool single_launch = method == PLS_HIP_KERNEL_TYPE1 && h->opt_algo == PLS_HIP_ALGO_AUTO && h->opt_fuse &&
                               (plsk::tiny_fit_covers(N, K, M, A, ldn, es) || plsk::tiny_fit_m_covers(N, K, M, A, ldn, es) ||
                                plsk::micro_fit_covers(N, K, M, A, ldn, es));  // (no use for X^T X there)
    if (wants_gram && !single_launch && !h->reducer && N > 0 && K <= 4096 && ensure(h, h->gxx, (size_t)K * K * 8) == PLS_HIP_OK &&
        ensure(h, h->gxy, (size_t)K * M * 8) == PLS_HIP_OK) {
        CHK(by_dtype(dtype, [&](auto t) {
            using Tx = decltype(t);
            return upload_accumulate<Tx>(h, (Tx *)dX, ldn, (const Tx *)X, ldx, N, K, (const Tx *)dY, ldn, M, (double *)h->gxx.p,
                                        (double *)h->gxy.p, &pre);
        }));
    } else {
        h->err.clear();
        CHK(h2d(h, dX, ldn, X, ldx, N, K, es));
    }
    if (pre) {
        h->pre_xx = (const double *)h->gxx.p;
        h->pre_xy = (const double *)h->gxy.p;
    }
    return PLS_HIP_OK;
}

}  // namespace
