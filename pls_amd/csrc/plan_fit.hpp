// plan_fit.hpp -- fit_device: Model::plsr (src/pls.cpp:390-437) enqueued on one stream.  A dispatcher: the single-launch fits
// (plan_fit_single.hpp), else the plan of fit_plan (fit_route.hpp: every per-fit decision and threshold) executed by fit_workspace,
// fit_xty, and fit_type2 (GRAM / KERNEL_TYPE2) or fit_passes (KERNEL, NIPALS).
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// the workspaces of a general-plan fit and what its prologue left behind
template <typename T>
struct FitWork {
    double *red, *part, *sspart, *XY, *v;
    T *work;
    // The partial rows of a fused pass are summed in the tail of the pass itself (slice_tail: no reduce launch behind it),
    // and with the device-side exchange attached the push of a sharded component rides there too, the gather in front of
    // the update: pass -> update.  PLS_HIP_TAIL=0: the launches of round 3 (A/B measurements).
    plsk::SliceTail tail;
    bool retiled = false;        // the working copy was made in the X^T Y sweep
    bool xx_local_done = false;  // this rank's X^T X slices were formed in the prologue
    int nip;                     // 1: NIPALS
};

// The workspaces in their fixed order (tests/test_gpu_history.py, the stateful-workspace list of ctx.hpp).  The tiled copy of the
// KERNEL plan is optional: refused its memory, the fit is planned again without it.
template <typename T>
int fit_workspace(pls_hip_context *c, const plsk::FitShape &shape, plsk::FitPlan &plan, FitWork<T> &w) {
    CHK(ensure(c, c->part, plan.part_bytes));
    CHK(ensure(c, c->sspart, plan.sspart_bytes));
    CHK(ensure(c, c->xy, (size_t)shape.K * shape.M * 8));
    CHK(ensure(c, c->v, (size_t)shape.K * 8));
    CHK(ensure(c, c->cs, (size_t)shape.A * 8));
    if (c->user_red) {
        if (c->user_red_count < (i64)(plan.red_bytes / 8)) return fail(c, PLS_HIP_ERR_INVALID, "reduce buffer too small");
        w.red = c->user_red;
    } else {
        CHK(ensure(c, c->red, plan.red_bytes));
        w.red = (double *)c->red.p;
    }
    if (plan.retile_fit && ensure(c, c->work, plan.work_bytes) != PLS_HIP_OK) {
        c->err.clear();
        plan = plsk::fit_plan(shape, plsk::FIT_NO_COPY);
    }
    if (plan.work_bytes) CHK(ensure(c, c->work, plan.work_bytes));
    w.part = (double *)c->part.p;
    w.sspart = (double *)c->sspart.p;
    w.XY = (double *)c->xy.p;
    w.v = (double *)c->v.p;
    // (round 5 moved this copy around inside its allocation -- 20 offsets from 256 bytes to 32 MB, profiles/r5/retile_offsets.txt:
    // retile_xty takes the same 1.60-1.63 ms wherever it lies)
    w.work = (T *)c->work.p;
    if (c->env.tail && c->opt_fuse && shape.N > 0) {
        if (!c->tailcnt.p) CHK(ensure(c, c->tailcnt, 256));
        HIPCHK(c, hipMemsetAsync(c->tailcnt.p, 0, 256, c->stream));  // (whatever an earlier, failed fit left behind)
        w.tail.cnt = (unsigned *)c->tailcnt.p;
        w.tail.red = w.red;
    }
    w.nip = plan.algo == plsk::FIT_NIPALS ? 1 : 0;
    return PLS_HIP_OK;
}

// prologue: XY = X^T Y (src/pls.cpp:396), summed over ranks -- and the first component's weights
template <typename T>
int fit_xty(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w) {
    const T *X = f.X;
    const i64 N = f.N, ldx = f.ldx;
    const int K = f.K, M = f.M;
    const i64 L0 = (i64)K * M;
    const bool type2 = p.algo == plsk::FIT_GRAM || p.algo == plsk::FIT_TYPE2;
    Range r_phase("X^T Y");
    if (!p.use_pre && N > 0 && (p.retile_fit || p.nip_copy) && M <= 8) {
        // the copy into tiles and X^T Y in ONE sweep over the caller's matrix (instead of retile_kernel + the X^T Y pass)
        int nb = 0, rc = 1;
        {
            Scope s(c, PLS_HIP_FAM_DEFLATE, 2 * (i64)N * K * sizeof(T) + (i64)N * M * sizeof(T) + L0 * 8);
            // (the source tile is as tall as the copy's for narrow matrices, the 256-byte-segment tile otherwise)
            rc = pick_int<8, 16, 32>(p.fused_mode ? p.tall_cg : 32, [&](auto cg) {
                return plsk::launch_retile_xty<T, decltype(cg)::value>(c->stream, c->num_cu, X, ldx, f.Y, f.ldy, w.work, p.WR, p.WR * (i64)K, (int)p.WR, N, K,
                                                                       M, w.part, (int)p.prow, &nb);
            });
            if (rc != 0) s.on = false;
        }
        if (rc == 0) {
            LAUNCH_CHECK(c);
            CHK(launch_reduce(c, w.part, nb, (int)L0, nullptr, 0, w.red));
            w.retiled = true;
        }
    }
    if (p.wide_only && !w.retiled && N > 0 && M <= 8) return fail(c, PLS_HIP_ERR_DEVICE, "copy into row-pack tiles failed");
    if (w.retiled) {
    } else if (p.use_pre) {
        hipLaunchKernelGGL(plsk::fill_slices_kernel, dim3((unsigned)((L0 + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                           c->stream, c->pre_xy, (int)L0, w.red);
        LAUNCH_CHECK(c);
    } else if (N > 0) {
        // KERNEL_TYPE2 / GRAM: the SYRK's diagonal workgroups form X^T Y on the way (no pass over X of its own); its
        // partial blocks take c->part, so it runs first and `part` is read again afterwards
        bool xy_from_syrk = false;
        if (type2) {
            CHK(compute_xx_local<T>(c, X, ldx, N, K, f.Y, f.ldy, M, w.red, &xy_from_syrk));
            w.xx_local_done = true;
            w.part = (double *)c->part.p;
        }
        if (!xy_from_syrk) {
            int nb = 0;
            CHK(launch_xty<T>(c, X, ldx, f.Y, f.ldy, N, K, M, w.part, &nb));
            CHK(launch_reduce(c, w.part, nb, (int)L0, nullptr, 0, w.red));
        }
    } else {
        HIPCHK(c, hipMemsetAsync(w.red, 0, (size_t)plsk::RED_SLICES * L0 * 8, c->stream));
    }
    CHK(do_allreduce(c, w.red, (i64)plsk::RED_SLICES * L0));
    CHK(launch_update(c, w.red, w.XY, f.W, f.P, f.Q, f.R, w.v, K, M, f.A, -1, w.nip));
    return PLS_HIP_OK;
}

// KERNEL_TYPE2 (src/pls.cpp:398, :422-425): XX = X^T X once, then the A-loop never touches X:
// tt = r^T XX r, p = XX r / tt; T is not computed.  XX is formed in 32-column blocks with the
// same column-reduction kernel as X^T Y (functional; an MFMA SYRK is the planned fast form).
// GRAM: the same loop for a KERNEL_TYPE1 request, then the scores in one pass.
template <typename T>
int fit_type2(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w) {
    const i64 N = f.N;
    const int K = f.K, M = f.M, A = f.A;
    double *red = w.red, *XY = w.XY, *v = w.v, *W = f.W, *P = f.P, *Q = f.Q, *R = f.R;
    CHK(ensure(c, c->xx, (size_t)K * K * 8));
    CHK(ensure(c, c->praw, (size_t)K * 8));
    double *XX = (double *)c->xx.p, *praw = (double *)c->praw.p;
    {
        Range r_phase("X^T X (SYRK)");
        if (p.use_pre) {  // this member's X^T X came with the upload: present it as slice 0, sum over the members
            const i64 KK = (i64)K * K;
            CHK(ensure(c, c->red2, (size_t)plsk::RED_SLICES * KK * 8));
            hipLaunchKernelGGL(plsk::fill_slices_kernel, dim3((unsigned)((KK + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                               c->stream, c->pre_xx, (int)KK, (double *)c->red2.p);
            LAUNCH_CHECK(c);
            CHK(do_allreduce(c, (double *)c->red2.p, (i64)plsk::RED_SLICES * KK));
            hipLaunchKernelGGL(plsk::sum_slices_kernel, dim3((unsigned)((KK + plsk::WG - 1) / plsk::WG)), dim3(plsk::WG), 0,
                               c->stream, (const double *)c->red2.p, (int)KK, XX);
            LAUNCH_CHECK(c);
        } else {
            if (!w.xx_local_done) CHK(compute_xx_local<T>(c, f.X, f.ldx, N, K));  // (an empty shard: zero slices)
            CHK(compute_xx_finish(c, K, XX));
        }
    }
    for (int a = 0; a < A; ++a) {
        Range r_comp("component", a);
        {
            Scope s(c, PLS_HIP_FAM_SMALL, ((i64)K * K + 2 * K) * 8);
            hipLaunchKernelGGL(plsk::symv_kernel, dim3((K + 3) / 4), dim3(plsk::WG), 0, c->stream,
                               (const double *)XX, (const double *)v, K, praw);  // XX symmetric: XX r
            LAUNCH_CHECK(c);
        }
        if (update_is_single(K, M, A, a)) {  // tt = r^T praw and the packing: the prologue of the one-workgroup update
            Scope s(c, PLS_HIP_FAM_SMALL, ((i64)K * M * 3 + (i64)K * (2 * (a + 2)) + 2 * K) * 8);
            hipLaunchKernelGGL(plsk::component_update_type2_kernel, dim3(1), dim3(plsk::UPD_THREADS),
                               (size_t)std::min(A, 4096) * sizeof(double), c->stream, (const double *)praw, (const double *)v, red,
                               XY, W, P, Q, R, v, K, M, A, a, (int)c->opt_power_iters, 0);
            LAUNCH_CHECK(c);
            continue;
        }
        hipLaunchKernelGGL(plsk::type2_pack_kernel, dim3(1), dim3(plsk::UPD_THREADS), 0, c->stream,
                           (const double *)praw, (const double *)v, K, red);
        LAUNCH_CHECK(c);
        CHK(launch_update(c, red, XY, W, P, Q, R, v, K, M, A, a, 0));
    }
    if (f.B) {
        const int nblk = (int)(((i64)K * M + plsk::WG - 1) / plsk::WG);
        hipLaunchKernelGGL(plsk::coefficients_kernel, dim3(nblk), dim3(plsk::WG), 0, c->stream, R, Q, K, M, A, f.B);
        LAUNCH_CHECK(c);
    }
    if (p.algo == plsk::FIT_GRAM && N > 0) {  // T = X R (src/pls.cpp:439-442 applied to the training data)
        Range r_t("T = X R");
        int nss = 0;
        CHK(launch_xb<T>(c, f.X, f.ldx, N, K, R, K, A, f.Tm, f.ldt, nullptr, &nss));
    }
    return replica_guard(c, W, P, Q, R, f.B, K, M, A);
}

// ---- the component loop of the KERNEL and NIPALS plans ------------------------------------------------------------------------
// what the passes of a fit hand from component to component, and what one pass tells the update behind it
template <typename T>
struct PassState {
    const T *Xc;             // the current matrix ...
    i64 ldc, tsc;            // ... its column stride and tile stride
    bool cur_tiled = false;  // Xc is the row-tile-major working copy
    int defer_b = 0;         // deferred write-back: index of the stored matrix X_b
    // of this component:
    bool tail_used, upd_done;
    bool store_x;            // X_a goes back to memory (false: it lives in the pass's registers only)
    plsk::Turn turn;
};
// A pass route answers PLS_HIP_OK (launched: scores, loading sums and t^T t of component a are on their way to `red`),
// PASS_NOT_COVERED (ask the next route) or an error.
constexpr int PASS_NOT_COVERED = -1;

// deferred write-back: the stored matrix is X_b (the caller's X for b = 0, the working copy after the
// first store); apply the a - b pending updates in registers, store X_a when `defer` are pending
template <typename T>
int pass_deferred(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w, PassState<T> &st, int a) {
    if (!(p.fused_mode && p.defer > 1 && a > 0)) return PASS_NOT_COVERED;
    const i64 N = f.N;
    const int K = f.K;
    int nb = 0, nss = 0, rc;
    const int np = a - st.defer_b;
    const bool store = (np == p.defer) && (a + 1 < f.A);
    plsk::PendingUpdates<T> pend{};
    for (int n = 0; n < np; ++n) {
        pend.t[n] = f.Tm + (i64)(st.defer_b + n) * f.ldt;
        pend.p[n] = f.P + (i64)(st.defer_b + n) * K;
    }
    {
        const i64 bytes = (store ? 2 : 1) * (i64)N * K * sizeof(T) + (np + 1) * (i64)N * sizeof(T) +
                          (np + 2) * (i64)K * 8;
        Scope s(c, PLS_HIP_FAM_FUSED, bytes);
        rc = plsk::launch_fused_defer<T>(c->stream, c->num_cu, st.Xc, st.ldc, st.tsc, w.work, p.ldw, p.tsw, N, K, w.v, np, pend,
                                         store, f.Tm + (i64)a * f.ldt, w.part, (int)p.prow, w.sspart, &nb, &nss);
        if (rc != 0) s.on = false;
    }
    if (rc != 0) return fail(c, PLS_HIP_ERR_DEVICE, "deferred fused pass launch failed");
    LAUNCH_CHECK(c);
    if (store) { st.Xc = w.work; st.ldc = p.ldw; st.tsc = p.tsw; st.cur_tiled = true; st.defer_b = a; }
    CHK(launch_reduce(c, w.part, nb, K, w.sspart, nss, w.red));
    return PLS_HIP_OK;
}

// tile-resident pass: [deflate with (t_{a-1}, p_{a-1}) +] t_a = X v, X^T t_a partials
template <typename T>
int pass_tall(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w, PassState<T> &st, int a) {
    if (!(p.fused_mode && !p.retile_fit)) return PASS_NOT_COVERED;
    const i64 N = f.N;
    const int K = f.K;
    const bool nipals = p.algo == plsk::FIT_NIPALS;
    T *work = w.work;
    int nb = 0, nss = 0;
    const T *tprev = (nipals && a > 0) ? f.Tm + (i64)(a - 1) * f.ldt : nullptr;
    const double *pprev = (nipals && a > 0) ? f.P + (i64)(a - 1) * K : nullptr;
    int rc;
    {
        const i64 bytes = ((tprev && st.store_x) ? 2 : 1) * (i64)N * K * sizeof(T) +
                          (tprev ? 2 : 1) * (i64)N * sizeof(T) + (tprev ? 3 : 2) * (i64)K * 8;
        Scope s(c, PLS_HIP_FAM_FUSED, bytes);
        if (p.mid_cg && a >= 2)  // half-height tiles of the working copy, in place
            rc = plsk::launch_fused_pass<T, 64>(c->stream, c->num_cu, work, p.ldw, p.tsw, work, p.ldw, p.tsw, N, K, w.v,
                                                tprev, pprev, f.Tm + (i64)a * f.ldt, w.part, (int)p.prow, w.sspart,
                                                &nb, &nss, (int)c->opt_fused_grid, 0, true, &w.tail, &st.tail_used, &st.upd_done, st.store_x, st.turn);
        else  // (a == 1 with mid_cg: X in 256-byte segments -> half-height tiles; A = 2: nothing is stored, no tile shape)
            rc = pick_int<8, 16, 32>(p.tall_cg, [&](auto cg) {
                return plsk::launch_fused_pass<T, decltype(cg)::value>(
                    c->stream, c->num_cu, st.Xc, st.ldc, st.tsc, (tprev && st.store_x) ? work : nullptr, p.ldw, p.tsw, N, K, w.v, tprev, pprev,
                    f.Tm + (i64)a * f.ldt, w.part, (int)p.prow, w.sspart, &nb, &nss, (int)c->opt_fused_grid,
                    (p.mid_cg && tprev && st.store_x) ? (int)p.WR : 0, st.Xc == work, &w.tail, &st.tail_used, &st.upd_done, st.store_x, st.turn);
            });
        if (rc != 0) s.on = false;  // nothing was launched: drop the event pair
    }
    if (rc != 0) return fail(c, PLS_HIP_ERR_DEVICE, "fused pass launch failed");
    LAUNCH_CHECK(c);
    if (tprev && st.store_x) { st.Xc = work; st.ldc = p.ldw; st.tsc = p.tsw; st.cur_tiled = p.tiled_work; }
    if (!st.tail_used) CHK(launch_reduce(c, w.part, nb, K, w.sspart, nss, w.red));
    return PLS_HIP_OK;
}

// short-tile fused pass on the working copy: NIPALS deflates it in place, KERNEL only reads it
template <typename T>
int pass_short_tile(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w, PassState<T> &st, int a) {
    const bool nipals = p.algo == plsk::FIT_NIPALS;
    if (!(p.wide_cg && (nipals ? (a >= 2 || w.retiled || p.wide_only) : true))) return PASS_NOT_COVERED;
    const i64 N = f.N;
    const int K = f.K;
    T *work = w.work;
    int nb = 0, nss = 0, rc;
    const T *tprev = (nipals && a > 0) ? f.Tm + (i64)(a - 1) * f.ldt : nullptr;
    const double *pprev = (nipals && a > 0) ? f.P + (i64)(a - 1) * K : nullptr;
    if ((!nipals || p.wide_only) && a == 0 && !w.retiled) {  // the one-time copy into short tiles (before the first component: it runs fused, too)
        Scope s(c, PLS_HIP_FAM_DEFLATE, 2 * (i64)N * K * sizeof(T));
        if (plsk::launch_retile<T>(c->stream, c->num_cu, f.X, f.ldx, work, p.ldw, p.tsw, (int)p.WR, N, K) != 0) {
            s.on = false;
            return fail(c, PLS_HIP_ERR_DEVICE, "retile launch failed");
        }
        LAUNCH_CHECK(c);
    }
    {
        const i64 bytes = ((tprev && st.store_x) ? 2 : 1) * (i64)N * K * sizeof(T) + (tprev ? 2 : 1) * (i64)N * sizeof(T) + 3 * (i64)K * 8;
        Scope s(c, PLS_HIP_FAM_FUSED, bytes);
        rc = pick_int<8, 16, 32, 64, 128, 256, 512>(p.wide_cg, [&](auto cg) {
            return plsk::launch_fused_pass<T, decltype(cg)::value>(c->stream, c->num_cu, work, p.ldw, p.tsw, work, p.ldw, p.tsw, N, K, w.v, tprev, pprev,
                                                                   f.Tm + (i64)a * f.ldt, w.part, (int)p.prow, w.sspart, &nb, &nss, (int)c->opt_fused_grid, 0,
                                                                   true, &w.tail, &st.tail_used, &st.upd_done, st.store_x, st.turn);
        });
        if (rc != 0) s.on = false;
    }
    if (rc != 0) return fail(c, PLS_HIP_ERR_DEVICE, "short-tile fused pass launch failed");
    LAUNCH_CHECK(c);
    if (!st.tail_used) CHK(launch_reduce(c, w.part, nb, K, w.sspart, nss, w.red));
    return PLS_HIP_OK;
}

// the one-product kernels: [deflation,] score, loading -- with deflation and score in one sweep on the semi-fused plan.  Covers every fit.
template <typename T>
int pass_unfused(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w, PassState<T> &st, int a) {
    const i64 N = f.N;
    const int K = f.K;
    T *work = w.work;
    int nss = 0, nb = 0;
    bool have_t = false;
    if (p.algo == plsk::FIT_NIPALS && a > 0) {  // X_a = X_{a-1} - t_{a-1} p_{a-1}^T (first one out of place)
        const T *tprev = f.Tm + (i64)(a - 1) * f.ldt;
        const double *pprev = f.P + (i64)(a - 1) * K;
        if (p.semi_fit) {  // wide matrices: deflation and score in one sweep (3NK instead of 4NK)
            const i64 bytes = 2 * (i64)N * K * sizeof(T) + 2 * (i64)N * sizeof(T) + 2 * (i64)K * 8;
            Scope s(c, PLS_HIP_FAM_DEFLATE, bytes);
            const int rc = plsk::launch_deflate_score<T>(c->stream, c->num_cu, st.Xc, st.ldc, st.tsc, work, p.ldw, p.tsw,
                                                         (int)(p.tiled_work ? p.WR : p.TR), N, K, tprev, pprev, w.v,
                                                         f.Tm + (i64)a * f.ldt, w.sspart, (int)p.ssmax, &nss, st.Xc == work);
            if (rc != 0) {
                s.on = false;
                return fail(c, PLS_HIP_ERR_DEVICE, "deflate+score launch failed");
            }
            LAUNCH_CHECK(c);
            have_t = true;
        }
        if (!have_t) CHK(launch_deflate<T>(c, st.Xc, st.ldc, work, p.ldw, N, K, tprev, pprev));
        st.Xc = work;
        st.ldc = p.ldw;
        st.tsc = p.tsw;
        st.cur_tiled = p.tiled_work;
    }
    if (!have_t)
        CHK(launch_xb<T>(c, st.Xc, st.ldc, N, K, w.v, K, 1, f.Tm + (i64)a * f.ldt, f.ldt, w.sspart, &nss));  // :419-420
    if (st.cur_tiled) {  // row-tile-major work buffer: the loading in tile addressing (:421)
        Scope s(c, PLS_HIP_FAM_XTY, (i64)N * K * sizeof(T) + (i64)N * sizeof(T) + (i64)K * 8);
        const T *ta = f.Tm + (i64)a * f.ldt;
        // (the tile of the copy: 64, 128 or 256 column groups; every other copy is read with the 32-group tile)
        const int cg = (p.wide_cg == 64 || p.wide_cg == 128 || p.wide_cg == 256) ? p.wide_cg : 32;
        const int xrc = pick_int<32, 64, 128, 256>(cg, [&](auto g) {
            return plsk::launch_xty_tiled<T, decltype(g)::value>(c->stream, c->num_cu, st.Xc, st.ldc, st.tsc, N, K, ta, w.part, (int)p.prow, &nb);
        });
        if (xrc != 0) {
            s.on = false;
            return fail(c, PLS_HIP_ERR_DEVICE, "tiled loading launch failed");
        }
        LAUNCH_CHECK(c);
    } else {
        CHK(launch_xty<T>(c, st.Xc, st.ldc, f.Tm + (i64)a * f.ldt, f.ldt, N, K, 1, w.part, &nb));  // :421
    }
    CHK(launch_reduce(c, w.part, nb, K, w.sspart, nss, w.red));
    return PLS_HIP_OK;
}

// the gather of collective number `seq` of the device-side exchange: this rank's inbox and flags of that parity
inline plsk::XchgGather exchange_gather(const pls_hip_context *c, unsigned long long seq) {
    const int par = (int)(seq & 1);
    plsk::XchgGather gx;
    gx.inbox = c->xep.inbox[c->xep.rank] + (i64)par * c->xep.n * plsk::XCHG_CAP;
    gx.flags = c->xep.flags[c->xep.rank] + par * c->xep.n;
    gx.n = c->xep.n; gx.cap = plsk::XCHG_CAP; gx.seq = seq;
    gx.status = c->xep.status; gx.host_status = c->xep.host_status; gx.limit = *c->xep.limit;
    return gx;
}

template <typename T>
int fit_passes(pls_hip_context *c, const FitArgs<T> &f, const plsk::FitPlan &p, FitWork<T> &w) {
    const i64 N = f.N;
    const int K = f.K, M = f.M, A = f.A;
    plsk::SliceTail &tail = w.tail;
    PassState<T> st;
    st.Xc = f.X;
    st.ldc = f.ldx;
    st.tsc = p.TR;
    using Route = int (*)(pls_hip_context *, const FitArgs<T> &, const plsk::FitPlan &, FitWork<T> &, PassState<T> &, int);
    const Route routes[] = {pass_deferred<T>, pass_tall<T>, pass_short_tile<T>, pass_unfused<T>};
    for (int a = 0; a < A; ++a) {
        Range r_comp("component", a);
        st.tail_used = st.upd_done = false;
        // sharded over the device-side exchange, the one-workgroup update behind the pass: the pass pushes (if its tail
        // runs), the update gathers.  The collective number is drawn only when the pass did push.
        const bool want_push = tail.cnt && p.xep_ok && update_is_single(K, M, A, a);
        // one response: the update is the last act of the pass's tail (update_m1.hpp) -- ONE launch per component; sharded
        // over the device-side exchange the tail pushes, waits for the peers' pushes and updates (other reducers: a call
        // between the pass and the update, so the update stays a launch of its own)
        const bool defl_pass = w.nip && a > 0;
        // The last deflating pass of a fit stores nothing: X_{A-1} is read by no later launch, and the work buffer is scratch,
        // not an output (after a fit it holds X_{A-2}).  On the three fused routes.  Not on the semi-fused route (the
        // loading launch behind launch_deflate_score reads what that stored: the store is not dead), not on the unfused plan;
        // the deferred plan has always skipped its last store.
        st.store_x = (a + 1 < A);
        // The turn-around: even components descend, odd ones ascend -- a function of the component index alone, so a fit
        // computes the same bits whatever ran before it on the handle and every rank of a sharded fit walks alike.  Only
        // deflating passes turn (the launcher ignores it for a read-only pass): components 0 and 1 ascend, 2 is the first to descend.
        st.turn = plsk::Turn{c->env.turnaround, c->env.turnaround && a % 2 == 0, c->env.turn_edge_bytes};
        const bool want_upd = tail.cnt && (c->env.tail_update == 2 || (c->env.tail_update == 1 && !defl_pass)) && M == 1 &&
                              K <= plsk::UPD1_KMAX && update_is_single(K, M, A, a) && (!c->reducer || want_push);
        tail.npush = 0;
        tail.upd = plsk::TailUpdate();
        tail.gx = plsk::XchgGather();
        if (want_push) {
            const unsigned long long seq = *c->xep.seq + 1;
            const int par = (int)(seq & 1);
            tail.npush = c->xep.n;
            tail.seq = seq;
            for (int j = 0; j < c->xep.n; ++j) {
                tail.peers.slot[j] = c->xep.inbox[j] + ((i64)par * c->xep.n + c->xep.rank) * plsk::XCHG_CAP;
                tail.peers.flag[j] = c->xep.flags[j] + par * c->xep.n + c->xep.rank;
            }
            if (want_upd) tail.gx = exchange_gather(c, seq);
        }
        if (want_upd) {
            tail.upd.XY = w.XY; tail.upd.W = f.W; tail.upd.P = f.P; tail.upd.Q = f.Q; tail.upd.R = f.R; tail.upd.vnext = w.v;
            tail.upd.A = A; tail.upd.a = a; tail.upd.nipals = w.nip;
        }
        if (N > 0) {
            int rc = PASS_NOT_COVERED;
            for (Route route : routes)
                if ((rc = route(c, f, p, w, st, a)) != PASS_NOT_COVERED) break;
            CHK(rc);
        } else {
            HIPCHK(c, hipMemsetAsync(w.red, 0, (size_t)plsk::RED_SLICES * (K + 1) * 8, c->stream));
        }
        if (st.upd_done) {  // the tail of the pass was the update as well (sharded: its push and gather too)
            if (want_push) ++*c->xep.seq;
        } else if (st.tail_used && want_push) {  // pushed from the tail of the pass: gather in the prologue of the update
            const plsk::XchgGather gx = exchange_gather(c, ++*c->xep.seq);
            CHK(launch_update(c, w.red, w.XY, f.W, f.P, f.Q, f.R, w.v, K, M, A, a, w.nip, &gx));
        } else {
            CHK(do_allreduce(c, w.red, (i64)plsk::RED_SLICES * (K + 1)));
            CHK(launch_update(c, w.red, w.XY, f.W, f.P, f.Q, f.R, w.v, K, M, A, a, w.nip));  // :427-433 and :403-416 of a+1
        }
    }
    if (f.B) {
        Scope s(c, PLS_HIP_FAM_SMALL, ((i64)K * A + (i64)M * A + (i64)K * M) * 8);
        const int nblk = (int)(((i64)K * M + plsk::WG - 1) / plsk::WG);
        hipLaunchKernelGGL(plsk::coefficients_kernel, dim3(nblk), dim3(plsk::WG), 0, c->stream, f.R, f.Q,
                           K, M, A, f.B);
        LAUNCH_CHECK(c);
    }
    return replica_guard(c, f.W, f.P, f.Q, f.R, f.B, K, M, A);
}

// ---- the fit on device pointers -----------------------------------------------------------
template <typename T>
int fit_device(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M,
               int A, int method, double *W, double *P, double *Q, double *R, T *Tm, i64 ldt, double *B) {
    // The sample-space plan (opt-in, never AUTO's choice): everything from G = X X^T, two sweeps over X (plan_dual.hpp)
    if (method == PLS_HIP_KERNEL_TYPE1 && c->opt_algo == PLS_HIP_ALGO_DUAL)
        return fit_dual<T>(c, X, ldx, Y, ldy, N, K, M, A, W, P, Q, R, Tm, ldt, B);
    const FitArgs<T> f{X, ldx, Y, ldy, N, K, M, A, method, W, P, Q, R, Tm, ldt, B};
    bool taken = false;
    CHK(fit_single_launch<T>(c, f, &taken));
    if (taken) return PLS_HIP_OK;
    const plsk::FitShape shape{N, K, M, A, (int)sizeof(T), ldx, ldy, ldt, (uintptr_t)X, (uintptr_t)Y, (uintptr_t)Tm, c->num_cu, method,
                               c->opt_algo, c->opt_fuse, c->opt_work_layout, c->opt_defer, c->opt_fused_grid,
                               c->reducer != nullptr, c->pre_xx && c->pre_xy, c->xep.on};
    plsk::FitPlan plan = plsk::fit_plan(shape, 0);
    FitWork<T> w;
    CHK(fit_workspace<T>(c, shape, plan, w));
    Range r_fit("pls_hip_fit");
    CHK(fit_xty<T>(c, f, plan, w));
    if (plan.algo == plsk::FIT_GRAM || plan.algo == plsk::FIT_TYPE2) return fit_type2<T>(c, f, plan, w);
    return fit_passes<T>(c, f, plan, w);
}

}  // namespace
