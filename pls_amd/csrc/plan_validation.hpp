// plan_validation.hpp -- pls_hip_validation: PRESS, reference column, signed-rank sums and p-values of cross-validation residuals
// (Model::validation / optimal_num_components, src/pls.cpp:235-289) on the device; kernels in validation_kernels.hpp.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// the largest nobs the one-workgroup route can take on this device: VAL_LDS_MAX_ROWS where the kernel's dynamic-LDS limit can
// be raised to the CU's 160 KiB, what fits in the 48 KiB every kernel has otherwise
i64 val_lds_rows_device(pls_hip_context *c) {
    if (c->val_lds_rows_dev >= 0) return c->val_lds_rows_dev;
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return plsk::VAL_LDS_ROWS_48K; }
    const bool big = plsk::raise_dynamic_lds(reinterpret_cast<const void *>(&plsk::signed_rank_lds_kernel),
                                             plsk::VAL_LDS_MAX_ROWS * plsk::VAL_LDS_ROW_BYTES);
    c->val_lds_rows_dev = big ? plsk::VAL_LDS_MAX_ROWS : plsk::VAL_LDS_ROWS_48K;
    return c->val_lds_rows_dev;
}

// workspace of the streaming route for P pairs at once: two key buffers and the per-workgroup digit counts
size_t val_keys_bytes(i64 P, i64 nobs) { return (size_t)P * 2 * (size_t)nobs * 8; }
size_t val_hist_bytes(i64 P, i64 nblk) { return (size_t)P * 256 * (size_t)nblk * 4; }
constexpr size_t VAL_ROUND_BYTES = (size_t)4 << 30;  // pairs are batched up to this much workspace per round

// PRESS partials of a piece of E that is on the device: columns [col0, col0 + ncols), rows [chunk0 VAL_CH, + rows)
int val_press_piece(pls_hip_context *c, const double *dE, i64 ld, i64 rows, i64 ncols, int chunk0, int nchunk_total, i64 col0,
                    double *part) {
    const i64 nchunk = (rows + plsk::VAL_CH - 1) / plsk::VAL_CH;
    Scope s(c, PLS_HIP_FAM_XTY, rows * ncols * 8);
    hipLaunchKernelGGL(plsk::press_partial_kernel, dim3((unsigned)(nchunk * ncols)), dim3(plsk::WG), 0, c->stream, dE, ld, rows,
                       (int)nchunk, chunk0, nchunk_total, col0, part);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

int val_press_finish(pls_hip_context *c, const double *part, int nchunk_total, int A, int M, double *PRESS, long long *ref) {
    Scope s(c, PLS_HIP_FAM_SMALL, (i64)M * A * ((i64)nchunk_total + 1) * 8 + (i64)M * 8);
    hipLaunchKernelGGL(plsk::press_finish_kernel, dim3(M), dim3(plsk::WG), 0, c->stream, part, nchunk_total, A, M, PRESS, ref);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// D and probw of every (m, alt) from E on the device and ref on the device; all launches on the stream, no host round trip
int val_signed_ranks(pls_hip_context *c, const double *dE, i64 nobs, int A, int M, const long long *ref, double *D, double *probw) {
    const i64 MA = (i64)M * A;
    const i64 lds_rows = c->opt_val_lds_rows >= 0 ? c->opt_val_lds_rows : val_lds_rows_device(c);
    if (nobs <= lds_rows) {
        (void)val_lds_rows_device(c);  // (raises the kernel's limit on this device)
        Scope s(c, PLS_HIP_FAM_SMALL, MA * nobs * 8 + 2 * MA * 8);
        hipLaunchKernelGGL(plsk::signed_rank_lds_kernel, dim3((unsigned)MA), dim3(plsk::VAL_LDS_THREADS),
                           (size_t)nobs * plsk::VAL_LDS_ROW_BYTES, c->stream, dE, (int)nobs, A, M, ref, D, probw);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    }
    CHK(ensure(c, c->valacc, (size_t)MA * 8));
    long long *acc = (long long *)c->valacc.p;
    const i64 pairs = (i64)M * (A - 1);
    if (pairs > 0) {
        HIPCHK(c, hipMemsetAsync(acc, 0, (size_t)MA * 8, c->stream));
        const i64 nblk = (nobs + plsk::RADIX_TILE - 1) / plsk::RADIX_TILE;
        const size_t per_pair = val_keys_bytes(1, nobs) + val_hist_bytes(1, nblk);
        i64 P = std::max<i64>(1, std::min<i64>(std::min<i64>(pairs, 65535), (i64)(VAL_ROUND_BYTES / per_pair)));
        // fewer pairs per round when the workspace does not fit
        while (ensure(c, c->valkeys, val_keys_bytes(P, nobs)) != PLS_HIP_OK || ensure(c, c->valhist, val_hist_bytes(P, nblk)) != PLS_HIP_OK) {
            if (P == 1) return PLS_HIP_ERR_ALLOC;
            c->err.clear();
            P = (P + 1) / 2;
        }
        unsigned long long *buf[2] = {(unsigned long long *)c->valkeys.p, (unsigned long long *)c->valkeys.p + P * nobs};
        unsigned *hist = (unsigned *)c->valhist.p;
        for (i64 p0 = 0; p0 < pairs; p0 += P) {
            const unsigned np = (unsigned)std::min(P, pairs - p0);
            const dim3 grid((unsigned)nblk, np);
            for (int pass = 0; pass < plsk::RADIX_PASSES; ++pass) {
                const int shift = 8 * pass;
                const unsigned mask = pass == plsk::RADIX_PASSES - 1 ? 0x7fu : 0xffu;  // bit 63 carries the sign
                const unsigned long long *src = buf[(pass + 1) & 1];
                unsigned long long *dst = buf[pass & 1];
                const bool first = pass == 0, last = pass == plsk::RADIX_PASSES - 1;
                Scope s(c, PLS_HIP_FAM_SMALL, (i64)np * nobs * 8 * ((first ? 4 : 2) + (last ? 0 : 1)));
                if (first)
                    hipLaunchKernelGGL((plsk::radix_hist_kernel<true>), grid, dim3(plsk::WG), 0, c->stream, dE, src, nobs, A, ref, (int)p0,
                                       shift, mask, (int)nblk, hist);
                else
                    hipLaunchKernelGGL((plsk::radix_hist_kernel<false>), grid, dim3(plsk::WG), 0, c->stream, dE, src, nobs, A, ref, (int)p0,
                                       shift, mask, (int)nblk, hist);
                LAUNCH_CHECK(c);
                hipLaunchKernelGGL(plsk::radix_scan_kernel, dim3(np), dim3(1024), 0, c->stream, hist, (int)(256 * nblk), A, ref, (int)p0);
                LAUNCH_CHECK(c);
#define VAL_SCATTER(F_, L_)                                                                                                         \
    hipLaunchKernelGGL((plsk::radix_scatter_kernel<F_, L_>), grid, dim3(plsk::WG), 0, c->stream, dE, src, dst, nobs, A, ref, (int)p0, \
                       shift, mask, (int)nblk, (const unsigned *)hist, acc)
                if (first) VAL_SCATTER(true, false);
                else if (last) VAL_SCATTER(false, true);
                else VAL_SCATTER(false, false);
#undef VAL_SCATTER
                LAUNCH_CHECK(c);
            }
        }
    }
    Scope s(c, PLS_HIP_FAM_SMALL, 3 * MA * 8);
    hipLaunchKernelGGL(plsk::signed_rank_finish_kernel, dim3((unsigned)((MA + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0, c->stream,
                       (const long long *)acc, nobs, A, M, ref, D, probw);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

int validation_impl(pls_hip_context *c, const double *E, i64 nobs, int A, int M, int mem, double *PRESS, double *D, double *probw,
                    int64_t *ref) {
    const i64 MA = (i64)M * A;
    const int nchunk = (int)((nobs + plsk::VAL_CH - 1) / plsk::VAL_CH);
    const bool ranks = D || probw;
    // outputs the caller does not take (and all of them for host memory) live in library scratch: [PRESS | D | probw | ref]
    CHK(ensure(c, c->valout, (size_t)(3 * MA + M) * 8));
    CHK(ensure(c, c->valpart, (size_t)MA * nchunk * 8));
    double *sc = (double *)c->valout.p, *part = (double *)c->valpart.p;
    const bool dev = mem == PLS_HIP_MEM_DEVICE;
    double *dP = dev && PRESS ? PRESS : sc, *dD = dev && D ? D : sc + MA, *dW = dev && probw ? probw : sc + 2 * MA;
    long long *dR = dev && ref ? (long long *)ref : (long long *)(sc + 3 * MA);
    const double *dE = E;
    if (!dev && ranks) {  // the sort reads columns again and again: all of E goes to the device
        CHK(ensure(c, c->vale, (size_t)MA * nobs * 8));
        CHK(h2d(c, c->vale.p, nobs, E, nobs, nobs, MA, 8));
        dE = (const double *)c->vale.p;
    }
    if (dev || ranks) {
        CHK(val_press_piece(c, dE, nobs, nobs, MA, 0, nchunk, 0, part));
    } else {
        // PRESS alone: E crosses in pieces of whole chunks (at most VAL_PIECE_BYTES each) through one staging buffer
        constexpr i64 PIECE = ((i64)64 << 20) / 8;
        const i64 prows = nobs <= PIECE ? nobs : (PIECE / plsk::VAL_CH) * plsk::VAL_CH;
        const i64 pcols = nobs <= PIECE ? std::max<i64>(1, std::min<i64>(MA, PIECE / nobs)) : 1;
        const i64 ldp = prows + (prows & 1);
        CHK(ensure(c, c->vale, (size_t)ldp * pcols * 8));
        for (i64 c0 = 0; c0 < MA; c0 += pcols)
            for (i64 r0 = 0; r0 < nobs; r0 += prows) {
                const i64 nr = std::min(prows, nobs - r0), nc = std::min(pcols, MA - c0);
                CHK(h2d(c, c->vale.p, ldp, E + c0 * nobs + r0, nobs, nr, nc, 8));
                CHK(val_press_piece(c, (const double *)c->vale.p, ldp, nr, nc, (int)(r0 / plsk::VAL_CH), nchunk, c0, part));
            }
    }
    CHK(val_press_finish(c, part, nchunk, A, M, dP, dR));
    if (ranks) CHK(val_signed_ranks(c, dE, nobs, A, M, dR, dD, dW));
    HostCall hc(c, mem);  // (every output has its place in valout already, asked for or not)
    CHK(hc.back_flat(PRESS, dP, (size_t)MA * 8));
    CHK(hc.back_flat(D, dD, (size_t)MA * 8));
    CHK(hc.back_flat(probw, dW, (size_t)MA * 8));
    CHK(hc.back_flat(ref, dR, (size_t)M * 8));
    return hc.finish();
}

}  // namespace
