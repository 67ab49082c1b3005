// dual_cv_kernels.hpp -- cross-validation folds of the sample-space plan (plan_dual_cv.hpp): every fold from ONE G = X X^T.
//
// A fold that holds out the rows Te and trains on the rest runs the recursion of dual_step_kernel on vectors of length N
// with the 0/1 mask m of its training rows: Y_0 = diag(m) Y, so the held-out rows of the working copy are zero and stay zero
// and every sum with Y_a is a sum over the training rows; Z = G Y_a comes for ALL rows, and so does the score
//     t = (g - sum_j c_j t_j) / nw,   c_j = (m o t_j)^T g / tt_j,
// which on a held-out row is x_te^T r_a, that row's score under the fold's model (r_a lies in the row space of the training
// rows).  tt = (m o t)^T t, q = Y_a^T t / tt, Y_a -= (m o t) q^T.  No W, P, R or B, no copy of G: every fold reads the same G.
//
//   dual_cv_init_kernel   per fold of a round: the position of every row in the fold's test set (-1: a training row),
//                         Y_0 = diag(m) Y, the running predictions of the held-out rows = 0
//   dual_cv_step_kernel   one component of every fold of the round, one workgroup per fold: dual_step_kernel with the mask,
//                         plus the predictions of the held-out rows and column a of E
// The round's product Z = G [Y_a(0) | Y_a(1) | ...] between them is xtg_kernel<double> with X := G (batch_kernels.hpp) or,
// for at most 32 columns, dual_gy_kernel.  Every sum is taken in a fixed order; nothing waits on another workgroup.
#pragma once
#include "dual_kernels.hpp"

namespace plsk {

// grid = folds of the round, 256 threads.  idx: the test rows of the round's first fold onwards (ts per fold).
// Ya (N x M per fold, ld N), pos (N per fold), pred (ts x M per fold).
__global__ __launch_bounds__(256) void dual_cv_init_kernel(const double *__restrict__ Y64, const i64 *__restrict__ idx, int N, int M,
                                                           int ts, double *__restrict__ Ya, int *__restrict__ pos,
                                                           double *__restrict__ pred) {
    const int f = blockIdx.x, tid = threadIdx.x;
    int *ps = pos + (i64)f * N;
    double *ya = Ya + (i64)f * M * N;
    for (int n = tid; n < N; n += 256) ps[n] = -1;
    __syncthreads();
    for (int i = tid; i < ts; i += 256) {
        const i64 r = idx[(i64)f * ts + i];
        if (r >= 0 && r < N) ps[r] = i;
    }
    __syncthreads();
    for (i64 e = tid; e < (i64)N * M; e += 256) ya[e] = ps[e % N] < 0 ? Y64[e] : 0.0;
    for (int e = tid; e < ts * M; e += 256) pred[(i64)f * ts * M + e] = 0.0;
}

// Component a of fold blockIdx.x of the round (fold0 + blockIdx.x of the call); thread t owns the rows t, t + 1024, ...
// (at most DUAL_RPT).  The sequence of dual_step_kernel; what differs:
//   c_j and tt sum over the training rows only (pos < 0); t is formed and stored for every row;
//   Y_a is deflated on the training rows; on a held-out row i of the fold pred[i, m] += t q_m and
//   E[m][fold * ts + i, a] = Y[row, m] - pred[i, m] (E: M matrices of nobs x A, column-major).
// Per fold: Ya, Z (N x M), T64 (N x A), ttv (A), scr (N + A: g, then c), pos (N), pred (ts x M).
__global__ __launch_bounds__(UPD_THREADS) void dual_cv_step_kernel(const double *__restrict__ Zall, double *__restrict__ Yall,
                                                                   double *__restrict__ Tall, double *__restrict__ ttall,
                                                                   double *__restrict__ scrall, const int *__restrict__ posall,
                                                                   double *__restrict__ predall, const double *__restrict__ Y64,
                                                                   double *__restrict__ E, int N, int M, int A, int a, int ts,
                                                                   i64 fold0, i64 nobs, int power_iters) {
    __shared__ UpdShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const i64 f = blockIdx.x;
    const double *Z = Zall + f * M * N;
    double *Ya = Yall + f * M * N, *T64 = Tall + f * (i64)N * A, *ttv = ttall + f * A;
    double *gbuf = scrall + f * (N + A), *cbuf = gbuf + N;
    const int *pos = posall + f * N;
    double *pred = predall + f * ts * M;
    double g[DUAL_RPT], t[DUAL_RPT];
    int ps[DUAL_RPT];
    if (M > 1) {
        // the M (M + 1) / 2 entries of S = Y_a^T Z on or above the diagonal: a wave per entry
        for (int e = wv; e < M * (M + 1) / 2; e += UPD_WAVES) {
            int i = 0, r = e;
            while (r >= M - i) { r -= M - i; ++i; }
            const int j = i + r;
            double s = 0.0;
            for (int n = lane; n < N; n += 64) s = fma(Ya[n + (i64)i * N], Z[n + (i64)j * N], s);
            s = wave_sum(s);
            if (lane == 0) sh.Gs[i + j * M] = sh.Gs[j + i * M] = s;
        }
        __syncthreads();
        dominant_eigvec_lds(sh.Gs, sh.Bs, sh.Cs, sh.qs, M, power_iters);
    }
    double part = 0.0;
#pragma unroll
    for (int i = 0; i < DUAL_RPT; ++i) {
        const int n = tid + i * UPD_THREADS;
        double u = 0.0;
        g[i] = 0.0;
        ps[i] = -1;
        if (n < N) {
            ps[i] = pos[n];
            if (M > 1) {
                for (int m = 0; m < M; ++m) {
                    u = fma(Ya[n + (i64)m * N], sh.qs[m], u);
                    g[i] = fma(Z[n + (i64)m * N], sh.qs[m], g[i]);
                }
            } else {
                u = Ya[n];
                g[i] = Z[n];
            }
            gbuf[n] = g[i];
        }
        part = fma(u, g[i], part);  // (u is zero on the held-out rows)
    }
    const double nw = sqrt(block_sum<UPD_WAVES>(part, sh.sred));  // (its barriers publish gbuf)
    for (int j = wv; j < a; j += UPD_WAVES) {  // a wave per earlier score, the training rows
        double s = 0.0;
        for (int n = lane; n < N; n += 64) s = fma(pos[n] < 0 ? T64[n + (i64)j * N] : 0.0, gbuf[n], s);
        s = wave_sum(s) / ttv[j];
        if (lane == 0) cbuf[j] = s;
    }
    __syncthreads();
    part = 0.0;
#pragma unroll
    for (int i = 0; i < DUAL_RPT; ++i) {
        const int n = tid + i * UPD_THREADS;
        t[i] = 0.0;
        if (n < N) {
            double s = g[i];
            for (int j = 0; j < a; ++j) s = fma(-cbuf[j], T64[n + (i64)j * N], s);
            t[i] = s / nw;
            T64[n + (i64)a * N] = t[i];
        }
        if (ps[i] < 0) part = fma(t[i], t[i], part);
    }
    const double tt = block_sum<UPD_WAVES>(part, sh.sred);  // (... and T64[:, a])
    for (int m = wv; m < M; m += UPD_WAVES) {  // a wave per response (Y_a is zero on the held-out rows)
        double s = 0.0;
        for (int n = lane; n < N; n += 64) s = fma(Ya[n + (i64)m * N], T64[n + (i64)a * N], s);
        s = wave_sum(s) / tt;
        if (lane == 0) sh.qs[m] = s;
    }
    __syncthreads();
    if (tid == 0) ttv[a] = tt;
#pragma unroll
    for (int i = 0; i < DUAL_RPT; ++i) {
        const int n = tid + i * UPD_THREADS;
        if (n >= N) continue;
        if (ps[i] < 0) {
            for (int m = 0; m < M; ++m) Ya[n + (i64)m * N] = fma(-t[i], sh.qs[m], Ya[n + (i64)m * N]);
        } else {
            double *e = E + (i64)a * nobs + (fold0 + f) * ts + ps[i];
            for (int m = 0; m < M; ++m) {
                const double p = fma(t[i], sh.qs[m], pred[ps[i] + (i64)m * ts]);
                pred[ps[i] + (i64)m * ts] = p;
                e[(i64)m * nobs * A] = Y64[n + (i64)m * N] - p;
            }
        }
    }
}

}  // namespace plsk
