// plan_missing_cv.hpp -- cross-validation folds of X with missing values (pls_hip_cv_folds_missing): the folds in rounds, every
// kernel of the component loop launched once per round with the fold as a grid dimension (missing_cv_kernels.hpp).  A fold is
// the algorithm of pls_hip_fit_missing on work copies of ALL rows with the training mask entering through N-sized vectors; its
// slab is MissCvLayout (miss_layout.hpp), which both sizes the round and is what the kernels carve.  The sweep geometry is
// miss_geom's, from (N, K, type, CU count) alone: the bits of a fold do not depend on the round it falls into.
// DESIGN.md f13 has the launches and the bytes per round and component.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// All pointers device memory but test_idx (host; idx_dev: its device copy).  Returns after the work has completed.
template <typename T>
int cv_folds_missing_device(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M, int A,
                            const long long *idx_dev, int ts, i64 num_folds, double *E, long long *iters) {
    constexpr int FV = 16 / (int)sizeof(T);
    const MissGeom g = miss_geom<T>(c, N, K);
    plsk::MissCvView v;
    v.l = plsk::miss_cv_layout(N, K, M, A, (int)sizeof(T), c->num_cu);
    // a round: as many folds as 4 GB and half the free memory hold; one fold always, if the allocation succeeds
    const i64 nround = std::max<i64>(1, round_size(v.l.bytes, 65535, c->env.misscv_round, num_folds));
    CHK(ensure(c, c->mcv, (size_t)(nround * v.l.bytes) + 16));
    v.base = (char *)c->mcv.p;
    int *round_word = (int *)(v.base + nround * v.l.bytes);
    const bool multi = M > 1;
    const int max_it = (int)c->opt_missing_iters;
    if (multi && !c->mconv_host) HIPCHK(c, hipHostMalloc((void **)&c->mconv_host, 64, hipHostMallocDefault));
    const i64 nobs = num_folds * ts;
    const bool wide_x = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), FV);
    const dim3 blk(plsk::WG), wave(plsk::WAVE);
    const unsigned nts = (unsigned)((ts + plsk::WG - 1) / plsk::WG);

    for (i64 f0 = 0; f0 < num_folds; f0 += nround) {
        Range r_round("round", (int)(f0 / nround));
        const unsigned nr = (unsigned)std::min<i64>(nround, num_folds - f0);
        const dim3 gN((unsigned)g.nbN, 1, nr), gK((unsigned)g.nbK, 1, nr), gY((unsigned)g.GY, 1, nr), g1(1, 1, nr);
        const dim3 gcol((unsigned)g.nkg, (unsigned)g.G, nr), grow((unsigned)g.nrb, (unsigned)g.S, nr);
        const long long *idx = idx_dev + f0 * ts;
        long long *it_out = iters ? iters + f0 * A : nullptr;

        // the column sweep of the round: [deflate and store] and accumulate against field vf, then the quotient -> field outf
        auto col_sweep = [&](bool first, bool store, bool defl, int vf, int outf, bool want_ss, bool use_stop) -> int {
            const bool wide = !first || wide_x;  // (the work copies have 16-byte columns)
            {
                Scope s(c, store ? PLS_HIP_FAM_DEFLATE : PLS_HIP_FAM_XTY,
                        (i64)nr * ((store ? 2 : 1) * N * (i64)K * (i64)sizeof(T) + (2 * N + 2 * (i64)K) * 8));
#define MISSCV_COL(V_, S_, D_) \
    hipLaunchKernelGGL((plsk::misscv_col_kernel<T, V_, S_, D_, true>), gcol, blk, 0, c->stream, v, first ? X : (const T *)nullptr, ldx, g.ldw, N, K, vf, use_stop)
#define MISSCV_COL_V(S_, D_) do { if (wide) MISSCV_COL(FV, S_, D_); else MISSCV_COL(1, S_, D_); } while (0)
                if (store && defl) MISSCV_COL_V(true, true);
                else if (store) MISSCV_COL_V(true, false);
                else MISSCV_COL_V(false, false);
#undef MISSCV_COL_V
#undef MISSCV_COL
                LAUNCH_CHECK(c);
            }
            Scope s(c, PLS_HIP_FAM_SMALL, (i64)nr * g.G * K * 16);
            hipLaunchKernelGGL(plsk::misscv_col_finish_kernel, gK, blk, 0, c->stream, v, g.G, K, outf, want_ss, use_stop);
            LAUNCH_CHECK(c);
            if (want_ss) {
                hipLaunchKernelGGL(plsk::misscv_normalize_kernel, gK, blk, 0, c->stream, v, K, (int)g.nbK, use_stop);
                LAUNCH_CHECK(c);
            }
            return PLS_HIP_OK;
        };

        hipLaunchKernelGGL(plsk::misscv_mask_kernel, gN, blk, 0, c->stream, v, N);
        LAUNCH_CHECK(c);
        hipLaunchKernelGGL(plsk::misscv_mask_clear_kernel, dim3(nts, 1, nr), blk, 0, c->stream, v, idx, ts);
        LAUNCH_CHECK(c);
        hipLaunchKernelGGL((plsk::misscv_y_init_kernel<T>), gY, blk, 0, c->stream, v, Y, ldy, N, M, multi);
        LAUNCH_CHECK(c);
        for (int a = 0; a < A; ++a) {
            Range r_comp("component", a);
            if (multi) {
                hipLaunchKernelGGL(plsk::misscv_u_pick_kernel, g1, wave, 0, c->stream, v, g.GY, M);
                LAUNCH_CHECK(c);
            }
            hipLaunchKernelGGL(plsk::misscv_u_start_kernel, gN, blk, 0, c->stream, v, N, multi);
            LAUNCH_CHECK(c);
            bool done = false;
            for (int it = 1; !done; ++it) {
                if (it == 1) {
                    // deflate-and-accumulate: reads X_{a-1} (the caller's matrix for a = 0), stores X_a, sums for w with u~
                    CHK(col_sweep(a == 0, true, a > 0, plsk::MCV_U, plsk::MCV_W, true, multi));
                } else {
                    hipLaunchKernelGGL(plsk::misscv_u_kernel, gN, blk, 0, c->stream, v, N, M, a);
                    LAUNCH_CHECK(c);
                    CHK(col_sweep(false, false, false, plsk::MCV_U, plsk::MCV_W, true, multi));
                }
                {
                    Scope s(c, PLS_HIP_FAM_XB, (i64)nr * (N * (i64)K * (i64)sizeof(T) + ((i64)K + N) * 8 + (g.S > 1 ? (i64)g.S * N * 32 : 0)));
                    hipLaunchKernelGGL((plsk::misscv_row_kernel<T, FV>), grow, blk, 0, c->stream, v, g.ldw, N, K, g.lrl, g.kper, g.S > 1, multi);
                    LAUNCH_CHECK(c);
                }
                if (g.S > 1) {
                    hipLaunchKernelGGL(plsk::misscv_row_finish_kernel, dim3((unsigned)((N + plsk::MISS_RF_ROWS - 1) / plsk::MISS_RF_ROWS), 1, nr),
                                       blk, 0, c->stream, v, g.S, N, multi);
                    LAUNCH_CHECK(c);
                }
                hipLaunchKernelGGL(plsk::misscv_tmask_kernel, gN, blk, 0, c->stream, v, N, multi);
                LAUNCH_CHECK(c);
                hipLaunchKernelGGL(plsk::misscv_yt_kernel, gY, blk, 0, c->stream, v, N, M, multi);
                LAUNCH_CHECK(c);
                hipLaunchKernelGGL(plsk::misscv_q_kernel, g1, wave, 0, c->stream, v, g.GY, M, A, a, it, max_it, multi, it_out);
                LAUNCH_CHECK(c);
                if (!multi || it >= max_it) {
                    done = true;
                } else if (it % MISS_BATCH == 0) {  // the host reads "every fold of the round has stopped" through pinned memory
                    hipLaunchKernelGGL(plsk::misscv_round_done_kernel, dim3(1), blk, 0, c->stream, v, (int)nr, round_word);
                    LAUNCH_CHECK(c);
                    HIPCHK(c, hipMemcpyAsync(c->mconv_host, round_word, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    done = *c->mconv_host != 0;
                }
            }
            CHK(col_sweep(false, false, false, plsk::MCV_TM, plsk::MCV_P, false, false));
            hipLaunchKernelGGL(plsk::misscv_y_deflate_kernel, gY, blk, 0, c->stream, v, N, M, a, multi && a + 1 < A);
            LAUNCH_CHECK(c);
            hipLaunchKernelGGL(plsk::misscv_record_kernel, dim3(nts, (unsigned)M, nr), blk, 0, c->stream, v, idx, ts, N, A, nobs, a,
                               E + f0 * ts);
            LAUNCH_CHECK(c);
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PLS_HIP_OK;
}

}  // namespace
