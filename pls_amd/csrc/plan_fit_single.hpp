// plan_fit_single.hpp -- the single-launch fits: fit_single_launch asks the one-launch routes (tiny, resident X^T X, resident, micro) in their
// fixed order; with the resident fits' turn-taking and workspace.  FitArgs: what a fit is called with.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// The resident fits of one process take turns on a device: a launch waits for the previous one's completion event, whatever
// stream that ran on, and records its own (two such kernels together could each hold CUs the other waits for).
struct ResidentTurn {
    std::mutex mu;
    hipEvent_t ev[64] = {};
    bool have[64] = {};
    hipStream_t last[64] = {};  // the stream of the last resident launch (the same stream again: its own order is enough)
    bool any[64] = {};
};
inline ResidentTurn &resident_turns() {
    static ResidentTurn t;
    return t;
}
inline void resident_turn(pls_hip_context *c) {
    ResidentTurn &t = resident_turns();
    std::lock_guard<std::mutex> lock(t.mu);
    const int d = c->device & 63;
    if (t.have[d] && t.any[d] && t.last[d] != c->stream) (void)hipStreamWaitEvent(c->stream, t.ev[d], 0);
}
inline void resident_done(pls_hip_context *c) {
    ResidentTurn &t = resident_turns();
    std::lock_guard<std::mutex> lock(t.mu);
    const int d = c->device & 63;
    if (!t.have[d]) {
        if (hipEventCreateWithFlags(&t.ev[d], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        t.have[d] = true;
    }
    (void)hipEventRecord(t.ev[d], c->stream);
    t.last[d] = c->stream;
    t.any[d] = true;
}

// The workspace of a resident launch in c->resident: 256 bytes of arrival counters (two, 64 bytes apart, zero before their
// launch), then `payload` bytes; and what its bounded waits report to (resident_kernels.hpp, ResidentSync)
int resident_workspace(pls_hip_context *c, size_t payload, plsk::ResidentSync &sy) {
    if (c->resident.bytes < 256 + payload) {
        CHK(ensure(c, c->resident, 256 + payload));
        HIPCHK(c, hipMemsetAsync(c->resident.p, 0, 256, c->stream));  // both counters start from zero
        c->resident_launches = 0;
    }
    sy.status = c->diverged_dev + 1;
    sy.limit = (long long)(0.05 * 1e8);  // 50 ms of the 100 MHz wall clock
#ifdef PLS_HIP_TESTING
    if (const char *e = getenv("PLS_HIP_TEST_RESIDENT_LIMIT_TICKS")) sy.limit = atoll(e);  // (the time-out path, tests only)
#endif
    return PLS_HIP_OK;
}

// ... of a fit that exchanges once per component: two parities of G partial rows of LP doubles, this launch's counter and the next one's
int resident_sync(pls_hip_context *c, int G, int LP, plsk::ResidentSync &sy) {
    CHK(resident_workspace(c, (size_t)2 * G * LP * 8, sy));
    unsigned *ctr = (unsigned *)c->resident.p;
    sy.bar = ctr + 16 * (c->resident_launches & 1);        // (64 bytes apart)
    sy.bar_next = ctr + 16 * ((c->resident_launches + 1) & 1);
    ++c->resident_launches;
    sy.part = (double *)((char *)c->resident.p + 256);
    sy.LP = LP;
    return PLS_HIP_OK;
}

// ---- the fit on device pointers -----------------------------------------------------------
// what fit_device is called with
template <typename T>
struct FitArgs {
    const T *X;
    i64 ldx;
    const T *Y;
    i64 ldy;
    i64 N;
    int K, M, A, method;
    double *W, *P, *Q, *R;
    T *Tm;
    i64 ldt;
    double *B;
};

// what the single-launch routes share
struct SingleFit {
    bool single_launch;  // what every single-launch route asks for
    bool resident_ok;    // ... and the per-component resident routes on top of it
    size_t fit_lds;      // dynamic LDS of the one-workgroup and the per-component resident kernels
    i64 fit_bytes;
};

// Every route: *taken = true once the fit is this route's (launched, or failed as its own); left alone, the next route is asked.

// A single-response problem small enough for one workgroup's registers: the whole fit in ONE launch (tiny_kernels.hpp) instead of
// three launches per component, whose dispatch latency would be the entire cost.  The reference's sequence, so the
// KERNEL plan and AUTO (also when X^T X came with the upload: one launch beats the K x K loop's sixty);
// an explicit NIPALS or GRAM request keeps its own kernels.
template <typename T>
int single_tiny(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &sf, bool *taken) {
    if (!(sf.single_launch && plsk::tiny_fit_covers(f.N, f.K, f.M, f.A, f.ldx, sizeof(T)) &&
          !plsk::micro_fit_covers(f.N, f.K, f.M, f.A, f.ldx, sizeof(T))))  // (the smallest data: one wave is faster than 1024 threads' barriers, single_micro)
        return PLS_HIP_OK;
    *taken = true;
    if (!plsk::raise_dynamic_lds((const void *)plsk::tiny_fit_kernel<T>, (int)plsk::TINY_LDS_MAX)  /* raised once per device: to the most any fit asks for */)
        return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the single-launch fit could not be raised");
    Range r_fit("pls_hip_fit (single launch)");
    Scope s(c, PLS_HIP_FAM_SMALL, sf.fit_bytes);
    hipLaunchKernelGGL((plsk::tiny_fit_kernel<T>), dim3(1), dim3(plsk::UPD_THREADS), sf.fit_lds, c->stream, f.X, f.ldx, f.Y, (int)f.N, f.K, f.A,
                       f.W, f.P, f.Q, f.R, f.Tm, f.ldt, f.B, (const i64 *)nullptr, 0, (i64)0, (double *)nullptr);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// Mid-size data (1-8 responses) with at most 128 columns under AUTO: ONE launch with three grid-wide hand-offs whatever A -- X^T X and X^T Y on
// the matrix cores, the component loop on XX in ONE workgroup's LDS, the scores at the end (resident_gram.hpp); the resident
// fits below exchange once per component.  An explicit KERNEL request keeps the reference's TYPE1 arithmetic (below).
template <typename T>
int single_resident_gram(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &, bool *taken) {
    const T *X = f.X, *Y = f.Y;
    i64 ldx = f.ldx, ldy = f.ldy, N = f.N, ldt = f.ldt;
    int K = f.K, M = f.M, A = f.A;
    double *W = f.W, *P = f.P, *Q = f.Q, *R = f.R, *B = f.B;
    T *Tm = f.Tm;
    if (!(f.method == PLS_HIP_KERNEL_TYPE1 && (c->opt_algo == PLS_HIP_ALGO_AUTO || c->env.resident_gram == 2) && c->opt_fuse && !c->reducer &&
          c->env.tiny && c->env.resident && c->env.resident_gram && !c->opt_graph && plsk::elem_aligned((uintptr_t)X, sizeof(T)) &&
          plsk::elem_aligned((uintptr_t)Y, sizeof(T)) && Tm && !plsk::single_fit_covers(N, K, M, A, ldx, sizeof(T)) &&
          !plsk::micro_fit_covers(N, K, M, A, ldx, sizeof(T))))
        return PLS_HIP_OK;
    int G = plsk::resident_gram_grid(N, K, M, A, ldx, sizeof(T), c->num_cu);
    if (!(G > 0 && host_flags(c))) return PLS_HIP_OK;
    plsk::ResidentGram rg;
    // the block form of phase 1 where it pays (PLS_HIP_RESIDENT_GRAM=4: the row form everywhere)
    rg.rs = c->env.resident_gram == 4 ? 0
                                      : plsk::resident_gram_splits(N, K, M, c->num_cu, plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), 16 / (int)sizeof(T)) &&
                                                                                           plsk::vec_ok((uintptr_t)Y, ldy, sizeof(T), 16 / (int)sizeof(T)));
    if (rg.rs > 0) {
        const int nb = (K + 15) / 16;
        rg.brows = (int)(((N + rg.rs - 1) / rg.rs + 15) & ~(i64)15);
        rg.rs = (int)((N + rg.brows - 1) / rg.brows);
        G = (nb * (nb + 1) / 2 + nb) * rg.rs;
        rg.rows_per = (int)(((N + G - 1) / G + 3) & ~(i64)3);  // (phase 4: a workgroup beyond N has no rows)
    } else {
        rg.rows_per = (int)(((N + G - 1) / G + 3) & ~(i64)3);
        G = (int)((N + rg.rows_per - 1) / rg.rows_per);
    }
    rg.LP = ((i64)K * K + (i64)K * M + 7) & ~(i64)7;
    rg.big = plsk::resident_gram_big(K);
    {  // many rows per workgroup and room in LDS: twice the rows staged at a time
        const int kp = (K + 15) / 16 * 16 + 16;
        if ((i64)rg.rows_per * kp > rg.big && rg.big < 16384 && 16384 + plsk::RG_SMALL + plsk::resident_gram_extra(K, M, A) <= plsk::RG_LDS_DOUBLES - (M > 1 ? 256 : 0))
            rg.big = 16384;
    }
    CHK(resident_workspace(c, ((size_t)(G + 1) * rg.LP + (size_t)K * A) * 8, rg.sy));
    const size_t lds = ((size_t)rg.big + plsk::RG_SMALL + (size_t)plsk::resident_gram_extra(K, M, A)) * 8;
    const void *fn = rg.rs > 0 ? (M <= 1 ? (const void *)plsk::resident_gram_fit_kernel<T, 1, true> : (const void *)plsk::resident_gram_fit_kernel<T, 2, true>)
                     : M <= 1 ? (const void *)plsk::resident_gram_fit_kernel<T, 1>
                     : M <= 2 ? (const void *)plsk::resident_gram_fit_kernel<T, 2>
                     : M <= 4 ? (const void *)plsk::resident_gram_fit_kernel<T, 4>
                              : (const void *)plsk::resident_gram_fit_kernel<T, 8>;
    if (!plsk::raise_dynamic_lds(fn, (int)lds)) return PLS_HIP_OK;  // (refused: the per-component resident kernels take the fit)
    *taken = true;
    if (!c->rgflags.p) {
        CHK(ensure(c, c->rgflags, (size_t)plsk::RESIDENT_MAX_WG * 4));
        HIPCHK(c, hipMemsetAsync(c->rgflags.p, 0, (size_t)plsk::RESIDENT_MAX_WG * 4, c->stream));
        c->rg_epoch = 0;
    }
    rg.flags = (unsigned *)c->rgflags.p;
    rg.epoch = c->rg_epoch;
    c->rg_epoch += 4;  // (three hand-offs at most; the words wrap with it: the kernel compares signed distances)
    rg.part = (double *)((char *)c->resident.p + 256);
    rg.gred = rg.part + (size_t)G * rg.LP;
    rg.rshare = rg.gred + rg.LP;
    Range r_fit("pls_hip_fit (single launch, resident, X^T X)");
    Scope s(c, PLS_HIP_FAM_SMALL, (2 * (i64)N * K + (i64)N * M + (i64)N * A) * (i64)sizeof(T) + (3 * (i64)K + M) * A * 8);
    resident_turn(c);
    int pit = (int)c->opt_power_iters;
    void *args[] = {(void *)&X, (void *)&ldx, (void *)&Y, (void *)&ldy, (void *)&N, (void *)&K, (void *)&M, (void *)&A, (void *)&pit, (void *)&W,
                    (void *)&P, (void *)&Q, (void *)&R, (void *)&Tm, (void *)&ldt, (void *)&B, (void *)&rg};
    if (hipLaunchKernel(fn, dim3(G), dim3(plsk::UPD_THREADS), args, lds, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, PLS_HIP_ERR_DEVICE, "kernel launch: resident_gram_fit");
    }
    resident_done(c);
    return PLS_HIP_OK;
}

// Mid-size single-response data (beyond one workgroup's 1024 rows, up to ~50 MB): the same single launch on up to 256
// workgroups with one grid-wide exchange per component (resident_kernels.hpp)
template <typename T>
int single_resident(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &sf, bool *taken) {
    if (!(sf.resident_ok && f.M == 1)) return PLS_HIP_OK;
    // (the score columns go out through one buffer descriptor per workgroup: A ld s below 2^31)
    const int wps = (i64)f.A * f.ldt * (i64)sizeof(T) < (1ll << 31) ? plsk::resident_wps(f.N, f.K, f.M, f.A, f.ldx, sizeof(T), c->num_cu) : 0;
    if (!(wps > 0 && host_flags(c))) return PLS_HIP_OK;
    *taken = true;
    const int G = (int)((f.N + (i64)plsk::WAVE * wps - 1) / ((i64)plsk::WAVE * wps));
    if (!plsk::raise_dynamic_lds((const void *)plsk::resident_fit_kernel<T>, (int)plsk::TINY_LDS_MAX))
        return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the resident fit could not be raised");
    plsk::ResidentSync sy;
    CHK(resident_sync(c, G, (f.K + 1 + 7) & ~7, sy));
    Range r_fit("pls_hip_fit (single launch, resident)");
    Scope s(c, PLS_HIP_FAM_SMALL, sf.fit_bytes);
    // all G workgroups must be resident together: the resident fits of ONE process take turns (an event chain per
    // device across its streams); a foreign kernel holding CUs ends in the bounded wait's error, not in a hang
    resident_turn(c);
    hipLaunchKernelGGL((plsk::resident_fit_kernel<T>), dim3(G), dim3(plsk::UPD_THREADS), sf.fit_lds, c->stream, f.X, f.ldx, f.Y,
                       f.N, f.K, f.A, f.W, f.P, f.Q, f.R, f.Tm, f.ldt, f.B, wps, sy);
    LAUNCH_CHECK(c);
    resident_done(c);
    return PLS_HIP_OK;
}

// ... and the same for 2..8 responses (resident_fit_m_kernel)
template <typename T>
int single_resident_m(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &sf, bool *taken) {
    if (!(sf.resident_ok && f.M >= 2)) return PLS_HIP_OK;
    const int wps = plsk::resident_wps(f.N, f.K, f.M, f.A, f.ldx, sizeof(T), c->num_cu);
    if (!(wps > 0 && host_flags(c))) return PLS_HIP_OK;
    *taken = true;
    const int G = (int)((f.N + (i64)plsk::WAVE * wps - 1) / ((i64)plsk::WAVE * wps));
    Range r_fit("pls_hip_fit (single launch, resident)");
    Scope s(c, PLS_HIP_FAM_SMALL, sf.fit_bytes);
    CHK(with_mm(f.M, [&](auto mm) {
        constexpr int MM = decltype(mm)::value;
        // (as in the one-response route: a refusal here leaves the launch counter where it was)
        if (!plsk::raise_dynamic_lds((const void *)plsk::resident_fit_m_kernel<T, MM>, (int)plsk::TINY_LDS_MAX))
            return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the resident fit could not be raised");
        plsk::ResidentSync sy;
        CHK(resident_sync(c, G, (std::max(f.K + 1, std::min(f.K * f.M, (int)plsk::UPD_THREADS)) + 7) & ~7, sy));
        resident_turn(c);
        hipLaunchKernelGGL((plsk::resident_fit_m_kernel<T, MM>), dim3(G), dim3(plsk::UPD_THREADS), sf.fit_lds, c->stream, f.X, f.ldx, f.Y, f.ldy,
                           f.N, f.K, f.M, f.A, (int)c->opt_power_iters, f.W, f.P, f.Q, f.R, f.Tm, f.ldt, f.B, wps, sy);
        return (int)PLS_HIP_OK;
    }));
    LAUNCH_CHECK(c);
    resident_done(c);
    return PLS_HIP_OK;
}

// The smallest problems (N <= 64, K <= 32, 1..8 responses: the reference's README example) as ONE WAVE (micro_fit_kernel)
template <typename T>
int single_micro(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &sf, bool *taken) {
    if (!(sf.single_launch && plsk::micro_fit_covers(f.N, f.K, f.M, f.A, f.ldx, sizeof(T)))) return PLS_HIP_OK;
    *taken = true;
    Range r_fit("pls_hip_fit (single launch, one wave)");
    Scope s(c, PLS_HIP_FAM_SMALL, sf.fit_bytes);
    with_mm(f.M, [&](auto mm) {
        hipLaunchKernelGGL((plsk::micro_fit_kernel<T, decltype(mm)::value>), dim3(1), dim3(plsk::WAVE), 0, c->stream, f.X, f.ldx, f.Y, f.ldy, (int)f.N,
                           f.K, f.M, f.A, (int)c->opt_power_iters, f.W, f.P, f.Q, f.R, f.Tm, f.ldt, f.B, (const i64 *)nullptr, 0, (i64)0, (double *)nullptr);
    });
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// ... and one workgroup for 2..8 responses (tiny_fit_m_kernel: the reference's own example, README.md:23, is such a fit)
template <typename T>
int single_tiny_m(pls_hip_context *c, const FitArgs<T> &f, const SingleFit &sf, bool *taken) {
    if (!(sf.single_launch && plsk::tiny_fit_m_covers(f.N, f.K, f.M, f.A, f.ldx, sizeof(T)))) return PLS_HIP_OK;
    *taken = true;
    Range r_fit("pls_hip_fit (single launch)");
    Scope s(c, PLS_HIP_FAM_SMALL, sf.fit_bytes);
    CHK(with_mm(f.M, [&](auto mm) {
        constexpr int MM = decltype(mm)::value;
        if (!plsk::raise_dynamic_lds((const void *)plsk::tiny_fit_m_kernel<T, MM>, (int)plsk::TINY_LDS_MAX))
            return fail(c, PLS_HIP_ERR_DEVICE, "dynamic LDS limit of the single-launch fit could not be raised");
        hipLaunchKernelGGL((plsk::tiny_fit_m_kernel<T, MM>), dim3(1), dim3(plsk::UPD_THREADS), sf.fit_lds, c->stream, f.X, f.ldx, f.Y, f.ldy, (int)f.N, f.K, f.M,
                           f.A, (int)c->opt_power_iters, f.W, f.P, f.Q, f.R, f.Tm, f.ldt, f.B, (const i64 *)nullptr, 0, (i64)0, (double *)nullptr);
        return (int)PLS_HIP_OK;
    }));
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

// The cascade, in its fixed order; *taken: one of the routes took the fit (the status is then the fit's).
template <typename T>
int fit_single_launch(pls_hip_context *c, const FitArgs<T> &f, bool *taken) {
    SingleFit sf;
    sf.single_launch = f.method == PLS_HIP_KERNEL_TYPE1 && (c->opt_algo == PLS_HIP_ALGO_KERNEL || c->opt_algo == PLS_HIP_ALGO_AUTO) &&
                       c->opt_fuse && !c->reducer && c->env.tiny;
    // (the per-component resident routes: a replayed graph would re-use one launch's arrival counter)
    sf.resident_ok = sf.single_launch && c->env.resident && !c->opt_graph && plsk::elem_aligned((uintptr_t)f.X, sizeof(T)) &&
                     plsk::elem_aligned((uintptr_t)f.Y, sizeof(T)) && f.Tm;
    sf.fit_lds = plsk::single_fit_lds_bytes(f.K, f.M, f.A);
    sf.fit_bytes = ((i64)f.N * f.K + (i64)f.N * f.M + (i64)f.N * f.A) * (i64)sizeof(T) + (3 * (i64)f.K + f.M) * f.A * 8;
    using Route = int (*)(pls_hip_context *, const FitArgs<T> &, const SingleFit &, bool *);
    const Route routes[] = {single_tiny<T>, single_resident_gram<T>, single_resident<T>, single_resident_m<T>, single_micro<T>, single_tiny_m<T>};
    *taken = false;
    for (Route route : routes) {
        CHK(route(c, f, sf, taken));
        if (*taken) return PLS_HIP_OK;
    }
    return PLS_HIP_OK;
}

}  // namespace
