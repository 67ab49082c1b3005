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
//   dual_cv_step_kernel   one component of every fold of the round, one workgroup per fold: the body of dual_step_kernel
//                         with the mask (dual_step_body<DUAL_CV>, dual_kernels.hpp), plus the predictions of the held-out rows
//                         and column a of E
// The round's product Z = G [Y_a(0) | Y_a(1) | ...] between them is xtg_kernel<double, false> with X := G (launch_sym_product)
// or, for at most 32 columns, dual_gy_kernel.  Every sum is taken in a fixed order; nothing waits on another workgroup.
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

// Component a of every fold of the round, one workgroup per fold (fold0 + blockIdx.x of the call): dual_step_body<true>.
__global__ __launch_bounds__(UPD_THREADS) void dual_cv_step_kernel(const double *__restrict__ Zall, double *__restrict__ Yall,
                                                                   double *__restrict__ Tall, double *__restrict__ ttall,
                                                                   double *__restrict__ scrall, const int *__restrict__ posall,
                                                                   double *__restrict__ predall, const double *__restrict__ Y64,
                                                                   double *__restrict__ E, int N, int M, int A, int a, int ts,
                                                                   i64 fold0, i64 nobs, int power_iters) {
    dual_step_body<DUAL_CV>(Zall, Yall, Tall, ttall, scrall, N, M, A, a, power_iters, nullptr, nullptr, nullptr, posall, predall, Y64, E,
                         ts, fold0, nobs);
}

}  // namespace plsk
