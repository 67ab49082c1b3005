// resample_kernels.hpp -- pls_hip_fit_resampled (plan_resample.hpp): the same (X, Y) fitted under many sets of non-negative
// row weights -- bootstrap draws (integer counts), jack-knife segments (0/1 masks), a case-weighted fit (one replicate).
//
// Replicate b is the model of (diag(s) X, diag(s) Y), s = sqrt(w_b).  Row weights generalise the 0/1 mask of the
// cross-validation folds (dual_cv_kernels.hpp): with G = X X^T the Gram matrix of the scaled rows is diag(s) G diag(s), so
//     G~ Y~_a = s o (G (s o Y~_a)),
// the product with the SHARED G stays one launch for all replicates of a round and the weights are N-sized work on either
// side of it (dual_step_body<DUAL_WEIGHTED>, dual_kernels.hpp).  Back through sample space as the batched fits go
// (dual_batch_kernels.hpp), with the scaling undone on the way: W~ = X~^T U~ = X^T (s o U~), so
//     R_b = X^T (s o S~_b),   B_b = X^T (s o S~_b Q_b^T),
// and B_b applies to UNSCALED new rows (s y^ = (s x)^T B).
//
//   resample_init_kernel    per replicate: s = sqrt(w), Y~_0 = s o Y and the product's input s o Y~_0
//   resample_step_kernel    one component of every replicate of the round (dual_step_body<DUAL_WEIGHTED>)
//   resample_sd_kernel      per replicate: the recurrence of dual_batch_sd_kernel, then S o= s and D o= s by rows
//   row_scale_kernel        the general route: diag(s) [X | Y] of one replicate into fp64 work copies
//   resample_accum_kernel   s1 += d_b, s2 = fma(d_b, d_b, s2) with d_b = B_b - B0, the round's replicates in index order
//   resample_final_kernel   Bmean = B0 + s1 / nrep, Bm2 = s2 - s1^2 / nrep
// Every sum is taken in a fixed order; nothing waits on another workgroup.
#pragma once
#include "dual_batch_kernels.hpp"

namespace plsk {

// grid = replicates of the round, 256 threads, a thread per row.  Replicate rep0 + blockIdx.x of the call; a negative index
// is the unit-weight fit (B0).  Wt: N x nrep (ld ldw), Y64: N x M (ld N).
__global__ __launch_bounds__(WG) void resample_init_kernel(const double *__restrict__ Wt, i64 ldw, i64 rep0,
                                                           const double *__restrict__ Y64, int N, int M, double *__restrict__ sall,
                                                           double *__restrict__ Yall, double *__restrict__ Yinall) {
    const i64 f = blockIdx.x, rep = rep0 + f;
    double *sv = sall + f * N, *Ya = Yall + f * M * N, *Yin = Yinall + f * M * N;
    for (int n = threadIdx.x; n < N; n += WG) {
        const double s = rep < 0 ? 1.0 : sqrt(Wt[n + rep * ldw]);
        sv[n] = s;
        for (int m = 0; m < M; ++m) {
            const double y = s * Y64[n + (i64)m * N];
            Ya[n + (i64)m * N] = y;
            Yin[n + (i64)m * N] = s * y;
        }
    }
}

// Component a of every replicate of the round, one workgroup per replicate (the layout of dual_batch_step_kernel, plus s and
// the product's input).
__global__ __launch_bounds__(UPD_THREADS) void resample_step_kernel(const double *__restrict__ Zall, double *__restrict__ Yall,
                                                                    double *__restrict__ Tall, double *__restrict__ Uall,
                                                                    double *__restrict__ Qall, double *__restrict__ Call,
                                                                    double *__restrict__ ttall, double *__restrict__ scrall,
                                                                    const double *__restrict__ sall, double *__restrict__ Yinall,
                                                                    int N, int M, int A, int a, int power_iters) {
    dual_step_body<DUAL_WEIGHTED>(Zall, Yall, Tall, ttall, scrall, N, M, A, a, power_iters, Uall, Qall, Call, nullptr, nullptr,
                                  nullptr, nullptr, 0, 0, 0, sall, Yinall);
}

// grid = replicates of the round, 256 threads, a thread per row: dual_batch_sd_kernel's recurrence on the row, then the row of
// D = S Q^T (a ascending) from the unscaled S, then both scaled by s[n]: what the back-projection reads.  Dall null: B was not
// asked for.
__global__ __launch_bounds__(WG) void resample_sd_kernel(double *__restrict__ Uall, const double *__restrict__ Call,
                                                         const double *__restrict__ Qall, const double *__restrict__ sall, int N,
                                                         int M, int A, double *__restrict__ Dall) {
    const i64 f = blockIdx.x;
    double *S = Uall + f * N * A;
    const double *C = Call + f * A * A, *Q = Qall + f * M * A, *sv = sall + f * N;
    for (int n = threadIdx.x; n < N; n += WG) {
        for (int a = 0; a < A; ++a) {
            double r = S[n + (i64)a * N];
            for (int j = 0; j < a; ++j) r = fma(-C[j + (i64)a * A], S[n + (i64)j * N], r);
            S[n + (i64)a * N] = r;
        }
        const double s = sv[n];
        if (Dall) {
            double *D = Dall + f * N * M;
            for (int m = 0; m < M; ++m) {
                double d = 0.0;
                for (int a = 0; a < A; ++a) d = fma(S[n + (i64)a * N], Q[m + (i64)a * M], d);
                D[n + (i64)m * N] = s * d;
            }
        }
        for (int a = 0; a < A; ++a) S[n + (i64)a * N] *= s;
    }
}

// General route: rows of [X | Y] scaled by s = sqrt(w) (Wt null: the unit-weight fit) into the fp64 work copies Xs (N x K) and
// Ys (N x M), both ld ldn.  A thread per entry of N x (K + M).
template <typename T>
__global__ __launch_bounds__(WG) void row_scale_kernel(const T *__restrict__ X, i64 ldx, const T *__restrict__ Y, i64 ldy,
                                                       const double *__restrict__ Wt, i64 N, i64 K, i64 M, i64 ldn,
                                                       double *__restrict__ Xs, double *__restrict__ Ys) {
    const i64 e = (i64)blockIdx.x * WG + threadIdx.x;
    if (e >= N * (K + M)) return;
    const i64 n = e % N, c = e / N;
    const double s = Wt ? sqrt(Wt[n]) : 1.0;
    if (c < K) Xs[n + c * ldn] = s * (double)X[n + c * ldx];
    else Ys[n + (c - K) * ldn] = s * (double)Y[n + (c - K) * ldy];
}

// A thread per entry of K x M (KM entries): the round's nb replicates in index order, Br their coefficients (stride KM).
__global__ __launch_bounds__(WG) void resample_accum_kernel(const double *__restrict__ Br, const double *__restrict__ B0, i64 KM,
                                                            i64 nb, double *__restrict__ s1, double *__restrict__ s2) {
    const i64 e = (i64)blockIdx.x * WG + threadIdx.x;
    if (e >= KM) return;
    const double b0 = B0[e];
    double a1 = s1[e], a2 = s2[e];
    for (i64 b = 0; b < nb; ++b) {
        const double d = Br[e + b * KM] - b0;
        a1 += d;
        a2 = fma(d, d, a2);
    }
    s1[e] = a1;
    s2[e] = a2;
}

// Bmean = B0 + s1 / nrep, Bm2 = s2 - s1^2 / nrep (either may be null)
__global__ __launch_bounds__(WG) void resample_final_kernel(const double *__restrict__ B0, const double *__restrict__ s1,
                                                            const double *__restrict__ s2, i64 KM, double nrep,
                                                            double *__restrict__ Bmean, double *__restrict__ Bm2) {
    const i64 e = (i64)blockIdx.x * WG + threadIdx.x;
    if (e >= KM) return;
    const double a1 = s1[e];
    if (Bmean) Bmean[e] = B0[e] + a1 / nrep;
    if (Bm2) Bm2[e] = s2[e] - a1 * a1 / nrep;
}

}  // namespace plsk
