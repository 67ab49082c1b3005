// Many response sets against one X (pls_hip_fit_batch): every problem b is Model::plsr(X, Y_b, KERNEL_TYPE2)
// (src/pls.cpp:390-437) on the shared XX = X^T X and its own XY_b = X^T Y_b.
//
//   xtg_kernel<T, false>  (syrk_kernels.hpp) the wide product X^T G (G = the columns of a round's problems, hundreds to
//                       thousands of them) on v_mfma_f64_16x16x4_f64; the rows are split over gridDim.y workgroups whose
//                       partial blocks reduce_partials_kernel adds in fixed order.  The same kernel with X := XX (symmetric:
//                       XX^T = XX), G := the current r of every problem and ONE row split is the component step's GEMM
//                       V = XX [r_0 r_1 ...] (launch_sym_product): no split-K, no atomics.
//   batch_step_kernel   one workgroup per problem: tt_b = r_b^T v_b, then component_update_call on [v_b, tt_b] -- p, q, the
//                       deflation of XY_b and the next w and r, the sequence cv_folds_kernel runs per fold.
//   batch_ssy / pack / finish / tt: the K- and M-sized bookkeeping around them.
// Nothing here waits on another workgroup: every hand-over is a kernel boundary.
#pragma once
#include "small_kernels.hpp"
#include "syrk_kernels.hpp"

namespace plsk {

// ssy[c] = sum_i G[i, c]^2: thread-strided sums, waves in order.   grid = C workgroups of WG threads
template <typename T>
__global__ __launch_bounds__(WG) void batch_ssy_kernel(const T *__restrict__ G, i64 ldg, i64 N, double *__restrict__ ssy) {
    __shared__ double sm[WG / WAVE];
    const T *g = G + (i64)blockIdx.x * ldg;
    double s = 0.0;
    for (i64 i = threadIdx.x; i < N; i += WG) {
        const double y = (double)g[i];
        s = fma(y, y, s);
    }
    s = block_sum<WG / WAVE>(s, sm);
    if (threadIdx.x == 0) ssy[blockIdx.x] = s;
}

// The message of np whole problems (first column col0 of the round's C): per problem [XY_b (K * M), ssy_b (M)], as RED_SLICES
// slices of Lm = (K + 1) * M * np values.  XY comes slice by slice from the sliced K x C product `red` (slice stride KC), ssy
// goes to slice 0.
__global__ __launch_bounds__(WG) void batch_pack_kernel(const double *__restrict__ red, i64 KC, const double *__restrict__ ssy,
                                                        int K, int M, i64 col0, i64 Lm, double *__restrict__ msg) {
    const i64 per = (i64)(K + 1) * M;
    for (i64 j = (i64)blockIdx.x * WG + threadIdx.x; j < Lm; j += (i64)gridDim.x * WG) {
        const i64 b = j / per, rem = j - b * per;
        if (rem < (i64)K * M) {
            const i64 src = (col0 + b * M) * K + rem;  // (column col0 + b*M + m, row k: rem = m*K + k)
#pragma unroll
            for (int s = 0; s < RED_SLICES; ++s) msg[(i64)s * Lm + j] = red[(i64)s * KC + src];
        } else {
            msg[j] = ssy[col0 + b * M + (rem - (i64)K * M)];
#pragma unroll
            for (int s = 1; s < RED_SLICES; ++s) msg[(i64)s * Lm + j] = 0.0;
        }
    }
}

// per-problem workspace layout (doubles)
struct BatchLayout {
    i64 xy, w, p, r, q, red, tt, ssy, total;
    __host__ __device__ BatchLayout(int K, int M, int A) {
        i64 o = 0;
        xy = o; o += (i64)K * M;
        w = o; o += (i64)K * A;
        p = o; o += (i64)K * A;
        r = o; o += (i64)K * A;
        q = o; o += (i64)M * A;
        red = o; o += K + 1;
        tt = o; o += A;
        ssy = o; o += M;
        total = (o + 1) & ~(i64)1;
    }
};

// Workgroup b = problem p0 + b of the round.  Dynamic LDS: A doubles.
//   a < 0 : XY_b and ssy_b from the (summed) message of this piece -- the slices added in index order -- then w_0, r_0.
//   a >= 0: v_b = column p0 + b of Vm (= XX r_b), tt = r_b^T v_b, then the update on [v_b, tt].
// The next r goes to column p0 + b of Rc, the operand of the next GEMM.
__global__ __launch_bounds__(UPD_THREADS) void batch_step_kernel(const double *__restrict__ msg, i64 Lm, const double *__restrict__ Vm,
                                                                 double *Rc, i64 ldv, double *__restrict__ ws, int p0, int K, int M,
                                                                 int A, int a, int power_iters) {
    extern __shared__ double cs[];
    __shared__ UpdShared sh;
    __shared__ double ttred[UPD_WAVES];
    const int tid = threadIdx.x;
    const BatchLayout L(K, M, A);
    double *base = ws + (i64)(p0 + (int)blockIdx.x) * L.total;
    double *XYb = base + L.xy, *Wb = base + L.w, *Pb = base + L.p, *Rb = base + L.r, *Qb = base + L.q, *red1 = base + L.red;
    double *rcur = Rc + (i64)(p0 + (int)blockIdx.x) * ldv;
    if (a < 0) {
        const double *mb = msg + (i64)blockIdx.x * (K + 1) * M;
        for (int j = tid; j < (K + 1) * M; j += UPD_THREADS) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < RED_SLICES; ++i) s += mb[(i64)i * Lm + j];
            if (j < K * M) XYb[j] = s;
            else base[L.ssy + (j - K * M)] = s;
        }
        __syncthreads();
        component_update_call(nullptr, 1, XYb, Wb, Pb, Qb, Rb, rcur, K, M, A, -1, 0, power_iters, 0, cs, sh);
        return;
    }
    const double *v = Vm + (i64)(p0 + (int)blockIdx.x) * ldv;
    double part = 0.0;
    for (int k = tid; k < K; k += UPD_THREADS) {
        const double p = v[k];
        part = fma(rcur[k], p, part);
        red1[k] = p;
    }
    const double tt = block_sum<UPD_WAVES>(part, ttred);
    if (tid == 0) {
        red1[K] = tt;
        base[L.tt + a] = tt;
    }
    __syncthreads();  // (the workgroup's own stores: visible to all its waves behind the barrier)
    component_update_call(red1, 1, XYb, Wb, Pb, Qb, Rb, rcur, K, M, A, a, 0, power_iters, 0, cs, sh);
}

// The outputs of problem blockIdx.x of the round (global problem index b0 + blockIdx.x); any of them may be null.
// B = R Q^T in the order of coefficients_kernel.
__global__ __launch_bounds__(WG) void batch_finish_kernel(const double *__restrict__ ws, int K, int M, int A, i64 b0,
                                                          double *__restrict__ R, double *__restrict__ Q, double *__restrict__ tt,
                                                          double *__restrict__ B, double *__restrict__ ssy) {
    const BatchLayout L(K, M, A);
    const double *base = ws + (i64)blockIdx.x * L.total;
    const double *Rb = base + L.r, *Qb = base + L.q;
    const i64 b = b0 + blockIdx.x;
    if (R)
        for (i64 j = threadIdx.x; j < (i64)K * A; j += WG) R[b * K * A + j] = Rb[j];
    if (Q)
        for (int j = threadIdx.x; j < M * A; j += WG) Q[b * M * A + j] = Qb[j];
    if (tt)
        for (int j = threadIdx.x; j < A; j += WG) tt[b * A + j] = base[L.tt + j];
    if (ssy)
        for (int j = threadIdx.x; j < M; j += WG) ssy[b * M + j] = base[L.ssy + j];
    if (B)
        for (i64 idx = threadIdx.x; idx < (i64)K * M; idx += WG) {
            const int k = (int)(idx % K), m = (int)(idx / K);
            double s = 0.0;
            for (int j = 0; j < A; ++j) s = fma(Rb[k + (i64)j * K], Qb[m + (i64)j * M], s);
            B[b * K * M + idx] = s;
        }
}

// per-problem route: tt[a] = r_a^T XX r_a for one fitted model (R: K x A).   grid = A workgroups of WG threads
__global__ __launch_bounds__(WG) void batch_tt_kernel(const double *__restrict__ XX, const double *__restrict__ R, int K,
                                                      double *__restrict__ tt) {
    __shared__ double sm[WG / WAVE];
    const double *r = R + (i64)blockIdx.x * K;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double acc = 0.0;  // (identical in every lane of the wave)
    for (int k = wv; k < K; k += WG / WAVE) {
        const double *col = XX + (i64)k * K;
        double s = 0.0;
        for (int j = lane; j < K; j += WAVE) s = fma(col[j], r[j], s);
        acc = fma(r[k], wave_sum(s), acc);
    }
    __syncthreads();
    if (lane == 0) sm[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < WG / WAVE; ++w) s += sm[w];
        tt[blockIdx.x] = s;
    }
}

}  // namespace plsk
