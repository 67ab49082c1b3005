// dual_batch_kernels.hpp -- pls_hip_fit_batch under the sample-space plan (plan_dual_batch.hpp): every problem from ONE
// G = X X^T.
//
// A problem of the batch is a fold without a mask and with its own Y: per component a round of problems costs one product
// Z = G [Y_a(0) | Y_a(1) | ...] and one launch of dual_batch_step_kernel, a workgroup per problem.  Q, tt and ssy are N-sized
// work.  R and B come back through sample space as well: W = X^T U, so the recurrence of dual_r_kernel runs on the columns
// of U,
//     s_a = u_a - sum_{j<a} C[j, a] s_j,   R = X^T S,   B = R Q^T = X^T (S Q^T) = X^T D,
// and R (or B) of ALL problems of a round is one product X^T [S(0) | S(1) | ...] -- K x (problems A) with ld K, which is the
// caller's array.  Nothing K-sized exists per problem besides the outputs.
//
//   dual_batch_init_kernel   a round's columns of Ys -> the fp64 working copy, ssy of every column
//   dual_batch_step_kernel   one component of every problem of the round (dual_step_body<DUAL_BATCH>, dual_kernels.hpp)
//   dual_batch_sd_kernel     per problem: S in place of U, D = S Q^T in place of Z
//   dual_xtvb_kernel         out (K x cols, ld K) = X^T V, V = N x cols fp64 (ld N): 128 columns of V by 128 columns of X per
//                            workgroup on the block core of mfma_block.hpp, the whole contraction (N <= DUAL_NMAX rows) in
//                            one workgroup -- no split, no partial blocks, straight into the caller's array
// Every sum is taken in a fixed order; nothing waits on another workgroup.
#pragma once
#include "dual_kernels.hpp"

namespace plsk {

// grid = columns of the round, 256 threads: Ya[:, c] = Ys[:, c] in fp64, ssy[c] = its sum of squares (null: not asked for)
template <typename T>
__global__ __launch_bounds__(WG) void dual_batch_init_kernel(const T *__restrict__ Ys, i64 ldy, int N, double *__restrict__ Ya,
                                                             double *__restrict__ ssy) {
    __shared__ double sm[WG / WAVE];
    const i64 c = blockIdx.x;
    const T *y = Ys + c * ldy;
    double *ya = Ya + c * N;
    double s = 0.0;
    for (int n = threadIdx.x; n < N; n += WG) {
        const double v = (double)y[n];
        ya[n] = v;
        s = fma(v, v, s);
    }
    s = block_sum<WG / WAVE>(s, sm);
    if (ssy && threadIdx.x == 0) ssy[c] = s;
}

// Component a of every problem of the round, one workgroup per problem.  Qall and ttall are the caller's arrays from the
// round's first problem on where they were asked for, workspace otherwise: the same layout either way.
__global__ __launch_bounds__(UPD_THREADS) void dual_batch_step_kernel(const double *__restrict__ Zall, double *__restrict__ Yall,
                                                                      double *__restrict__ Tall, double *__restrict__ Uall,
                                                                      double *__restrict__ Qall, double *__restrict__ Call,
                                                                      double *__restrict__ ttall, double *__restrict__ scrall, int N,
                                                                      int M, int A, int a, int power_iters) {
    dual_step_body<DUAL_BATCH>(Zall, Yall, Tall, ttall, scrall, N, M, A, a, power_iters, Uall, Qall, Call, nullptr, nullptr, nullptr,
                               nullptr, 0, 0, 0);
}

// grid = problems of the round, 256 threads, a thread per row: S[n, a] = U[n, a] - sum_{j<a} C[j, a] S[n, j] in place (j
// ascending, as dual_r_kernel), then (Dall: B was asked for) D[n, m] = sum_a S[n, a] Q[m, a], a ascending.
__global__ __launch_bounds__(WG) void dual_batch_sd_kernel(double *__restrict__ Uall, const double *__restrict__ Call,
                                                           const double *__restrict__ Qall, int N, int M, int A,
                                                           double *__restrict__ Dall) {
    const i64 f = blockIdx.x;
    double *S = Uall + f * N * A;
    const double *C = Call + f * A * A, *Q = Qall + f * M * A;
    for (int n = threadIdx.x; n < N; n += WG) {
        for (int a = 0; a < A; ++a) {
            double r = S[n + (i64)a * N];
            for (int j = 0; j < a; ++j) r = fma(-C[j + (i64)a * A], S[n + (i64)j * N], r);
            S[n + (i64)a * N] = r;
        }
        if (Dall) {
            double *D = Dall + f * N * M;
            for (int m = 0; m < M; ++m) {
                double d = 0.0;
                for (int a = 0; a < A; ++a) d = fma(S[n + (i64)a * N], Q[m + (i64)a * M], d);
                D[n + (i64)m * N] = d;
            }
        }
    }
}

constexpr int XTVB_TB = 128;           // columns of V and columns of X per workgroup
constexpr int XTVB_RC = 16;            // rows per staged chunk
constexpr int XTVB_LD = XTVB_RC + 2;   // a staged column, padded: the operand reads of a half-wave (16 columns li, 2 rows lq: 18 li + lq) hit 32 distinct bank pairs
constexpr size_t XTVB_LDS_BYTES = (size_t)2 * XTVB_TB * XTVB_LD * 8;  // two workgroups per CU

// out[k, c] = sum_n X[n, k] V[n, c] for 128 columns k of X (blockIdx.x / nbc) and 128 columns c of V (blockIdx.x % nbc: the
// workgroups that share a panel of X are neighbours, V stays in the caches).  The MFMA's rows are the columns of V, its columns
// the columns of X, 4 rows of both the contraction: a lane leaves with 16 consecutive k of an output column (quad_store_t).
// Rows beyond N, columns beyond K and beyond cols are staged as zeros; fp32 storage becomes fp64 where the panel is staged.
template <typename T>
__global__ __launch_bounds__(256, 2) void dual_xtvb_kernel(const T *__restrict__ X, i64 ldx, int N, i64 K,
                                                           const double *__restrict__ V, int cols, int nbc,
                                                           double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xtvb_raw[];
    double *Vs = reinterpret_cast<double *>(xtvb_raw), *Xs = Vs + XTVB_TB * XTVB_LD;
    const int tid = threadIdx.x;
    const int sr = tid & (XTVB_RC - 1), sc = tid >> 4;  // staging: row of the chunk, first of its 8 columns (sc, sc + 16, ...)
    const int c0 = (int)(blockIdx.x % nbc) * XTVB_TB;
    const i64 k0 = (i64)(blockIdx.x / nbc) * XTVB_TB;
    const QuadMap q;
    f64x4 acc[4][4];
    quad_zero(acc);
    double gv[8], gx[8];
    auto load_chunk = [&](int n0) {
        const int n = n0 + sr;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = sc + 16 * j;
            gv[j] = (n < N && c0 + c < cols) ? V[n + (i64)(c0 + c) * N] : 0.0;
            gx[j] = (n < N && k0 + c < K) ? (double)X[n + (k0 + c) * ldx] : 0.0;
        }
    };
    load_chunk(0);
    for (int n0 = 0; n0 < N; n0 += XTVB_RC) {
        __syncthreads();  // everyone is done reading the previous chunk
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Vs[(sc + 16 * j) * XTVB_LD + sr] = gv[j];
            Xs[(sc + 16 * j) * XTVB_LD + sr] = gx[j];
        }
        __syncthreads();
        if (n0 + XTVB_RC < N) load_chunk(n0 + XTVB_RC);  // in flight under the chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < XTVB_RC; kk += 4) quad_step<XTVB_LD, 1>(Vs, Xs, q, kk, acc);
    }
    quad_store_t(acc, q, out, K, c0, k0, cols, K);
}

}  // namespace plsk
