// dual_cvbatch_kernels.hpp -- pls_hip_cv_press_batch under the sample-space plan (plan_dual_cvbatch.hpp): the cross-validation
// folds of MANY response sets from ONE G = X X^T, PRESS reduced on the device.
//
// A (problem, fold) pair is a fold with its own Y: item = b num_folds + f runs the masked recursion of dual_cv_kernels.hpp on
// Y_0 = diag(m_f) Y_b.  The mask depends on the fold alone, so the table `pos` (position of a row in a fold's test set, -1: a
// training row) exists once per FOLD and every problem reads it.  Per component a round of items costs one product
// Z = G [Y_a of every item] and one launch of dual_cvb_step_kernel, a workgroup per item, which also leaves the item's
// partial PRESS: the sum of e^2 over the fold's held-out rows, taken by test position.  PRESS[b][m, c] is the sum of the
// partials of the problem's folds in fold order, wherever the round boundaries fall.
//
//   dual_cvb_pos_kernel      once per call: pos of every fold
//   dual_cvb_init_kernel     per item of a round, straight from the caller's Ys: Y_0 = diag(m_f) Y_b in fp64, the responses of
//                            the held-out rows (yte) and their sums of squares (the item's partial ssy), predictions = 0
//   dual_cvb_step_kernel     one component of every item of the round (dual_step_body<DUAL_CVB>, dual_kernels.hpp)
//   dual_cvb_reduce_kernel   after a round: PRESS and ssy of the round's problems += the items' partials, in item order
//   cvb_ssy_kernel           the general route's ssy: the held-out rows of every problem, by observation
// Every sum is taken in a fixed order, no atomics; nothing waits on another workgroup.
#pragma once
#include "dual_kernels.hpp"

namespace plsk {

// grid = folds of the call, 256 threads.  idx: ts test rows per fold; pos: N per fold.
__global__ __launch_bounds__(WG) void dual_cvb_pos_kernel(const i64 *__restrict__ idx, int N, int ts, int *__restrict__ pos) {
    const i64 f = blockIdx.x;
    int *ps = pos + f * N;
    for (int n = threadIdx.x; n < N; n += WG) ps[n] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < ts; i += WG) {
        const i64 r = idx[f * ts + i];
        if (r >= 0 && r < N) ps[r] = i;
    }
}

// grid = items of the round (item0 + blockIdx.x of the call), 256 threads.  Ya (N x M per item, ld N), pred and yte (ts x M
// per item, ld ts), ssyp (M per item).
template <typename T>
__global__ __launch_bounds__(WG) void dual_cvb_init_kernel(const T *__restrict__ Ys, i64 ldy, const i64 *__restrict__ idx,
                                                           const int *__restrict__ pos, int N, int M, int ts, i64 nfolds, i64 item0,
                                                           double *__restrict__ Ya, double *__restrict__ pred,
                                                           double *__restrict__ yte, double *__restrict__ ssyp) {
    __shared__ double sm[WG / WAVE];
    const i64 it = blockIdx.x, item = item0 + it, b = item / nfolds, f = item % nfolds;
    const int tid = threadIdx.x;
    const T *y = Ys + b * M * ldy;
    const int *ps = pos + f * N;
    const i64 *te = idx + f * ts;
    double *ya = Ya + it * M * N;
    for (int m = 0; m < M; ++m) {
        for (int n = tid; n < N; n += WG) ya[n + (i64)m * N] = ps[n] < 0 ? (double)y[n + m * ldy] : 0.0;
        double s = 0.0;
        for (int i = tid; i < ts; i += WG) {
            const i64 r = te[i];
            const double v = (r >= 0 && r < N) ? (double)y[r + m * ldy] : 0.0;
            yte[(it * M + m) * ts + i] = v;
            pred[(it * M + m) * ts + i] = 0.0;
            s = fma(v, v, s);
        }
        s = block_sum<WG / WAVE>(s, sm);
        if (tid == 0) ssyp[it * M + m] = s;
    }
}

// Component a of every item of the round, one workgroup per item.
__global__ __launch_bounds__(UPD_THREADS) void dual_cvb_step_kernel(const double *__restrict__ Zall, double *__restrict__ Yall,
                                                                    double *__restrict__ Tall, double *__restrict__ ttall,
                                                                    double *__restrict__ scrall, const int *__restrict__ pos,
                                                                    double *__restrict__ predall, const double *__restrict__ yte,
                                                                    double *__restrict__ escr, double *__restrict__ pressp,
                                                                    double *__restrict__ E, int N, int M, int A, int a, int ts,
                                                                    i64 item0, i64 nfolds, i64 nobs, int power_iters) {
    dual_step_body<DUAL_CVB>(Zall, Yall, Tall, ttall, scrall, N, M, A, a, power_iters, nullptr, nullptr, nullptr, pos, predall, yte, E,
                             ts, item0, nobs, nullptr, nullptr, nfolds, escr, pressp);
}

// The round's items [item0, item0 + nb) into the outputs of their problems: blockIdx.x / nblk is the problem counted from the
// round's first, the rest of the index the entry -- e < MA of PRESS (M x A, ld M), MA <= e < MA + M of ssy.  A problem whose
// first fold lies in the round starts from zero, one that began in an earlier round continues its running sum.
// PRESS, ssy: null = not asked for.
__global__ __launch_bounds__(WG) void dual_cvb_reduce_kernel(const double *__restrict__ pressp, const double *__restrict__ ssyp,
                                                             i64 item0, i64 nb, i64 nfolds, int MA, int M, int nblk,
                                                             double *__restrict__ PRESS, double *__restrict__ ssy) {
    const i64 b = item0 / nfolds + blockIdx.x / nblk;
    const int e = (int)(blockIdx.x % nblk) * WG + threadIdx.x;
    if (e >= MA + M) return;
    const i64 lo = max(item0, b * nfolds), hi = min(item0 + nb, (b + 1) * nfolds);
    const bool press = e < MA;
    double *o = press ? PRESS : ssy;
    if (!o || lo >= hi) return;
    o += press ? b * MA + e : b * M + (e - MA);
    const double *p = press ? pressp + e : ssyp + (e - MA);
    const i64 stride = press ? MA : M;
    double s = lo == b * nfolds ? 0.0 : *o;
    for (i64 item = lo; item < hi; ++item) s += p[(item - item0) * stride];
    *o = s;
}

// ssy[b M + m] = sum over the nobs observations o, in a fixed order, of Ys[idx[o], b M + m]^2.  grid = nprob M, 256 threads.
template <typename T>
__global__ __launch_bounds__(WG) void cvb_ssy_kernel(const T *__restrict__ Ys, i64 ldy, const i64 *__restrict__ idx, i64 N, i64 nobs,
                                                     double *__restrict__ ssy) {
    __shared__ double sm[WG / WAVE];
    const T *y = Ys + (i64)blockIdx.x * ldy;
    double s = 0.0;
    for (i64 o = threadIdx.x; o < nobs; o += WG) {
        const i64 r = idx[o];
        const double v = (r >= 0 && r < N) ? (double)y[r] : 0.0;
        s = fma(v, v, s);
    }
    s = block_sum<WG / WAVE>(s, sm);
    if (threadIdx.x == 0) ssy[blockIdx.x] = s;
}

}  // namespace plsk
