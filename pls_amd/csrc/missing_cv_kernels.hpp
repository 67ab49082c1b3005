// missing_cv_kernels.hpp -- the folds of pls_hip_cv_folds_missing, a round at a time (plan_missing_cv.hpp enqueues them).
// Every kernel here is launched ONCE per round with the fold of the round in blockIdx.z: workgroup (x, y, f) does for fold f
// what workgroup (x, y) of the kernel of the same name in missing_kernels.hpp does for a fit -- the sweeps, their finish and
// normalise kernels and the one-wave kernels of the Y side ARE those kernels' bodies, given the fields of fold f's slab
// (miss_layout.hpp, MissCvLayout).  So the sums of a fold are the fit's, in the fit's order, and do not depend on the round.
// The training mask m of a fold (1 / 0 per row) enters through N-sized vectors only:
//   misscv_mask_kernel, misscv_mask_clear_kernel   m
//   misscv_u_start_kernel, misscv_u_kernel         u~ = m o u: what the column sweep for w accumulates against
//   misscv_tmask_kernel                            t~ = m o t: what q, the stop rule and the column sweep for p see
//   misscv_y_init_kernel, misscv_y_deflate_kernel  Y_a on every row (deflated with the full t), its column sums of squares over
//                                                  the training rows (the choice of u)
//   misscv_record_kernel                           the held-out rows of Y_{a+1} -> E
// A held-out row adds exact zeros to every column sum and is deflated with its own score.
#pragma once
#include "missing_kernels.hpp"

namespace plsk {

struct MissCvView {
    char *base;  // the slab of the round's first fold
    MissCvLayout l;
    template <typename U>
    __device__ __forceinline__ U *at(int field) const {
        return reinterpret_cast<U *>(base + (i64)blockIdx.z * l.bytes + l.off[field]);
    }
    __device__ __forceinline__ const int *stop(bool multi) const { return multi ? at<int>(MCV_WORDS) + 1 : nullptr; }
};

// m = 1 on every row; then the held-out rows of the fold are cleared (idx: the round's first fold, ts rows per fold)
__global__ __launch_bounds__(WG) void misscv_mask_kernel(MissCvView v, i64 N) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i < N) v.at<double>(MCV_MASK)[i] = 1.0;
}
__global__ __launch_bounds__(WG) void misscv_mask_clear_kernel(MissCvView v, const long long *__restrict__ idx, int ts) {
    const int j = (int)(blockIdx.x * WG + threadIdx.x);
    if (j < ts) v.at<double>(MCV_MASK)[idx[(i64)blockIdx.z * ts + j]] = 0.0;
}

// Ya = Y; yss[blockIdx.x][j] = this workgroup's sum of squares of column j over the TRAINING rows (M > 1: the choice of u)
template <typename T>
__global__ __launch_bounds__(WG) void misscv_y_init_kernel(MissCvView v, const T *__restrict__ Y, i64 ldy, i64 N, int M, bool want_ss) {
    __shared__ double smem[WG / WAVE];
    double *Ya = v.at<double>(MCV_YA), *sspart = v.at<double>(MCV_YSS);
    const double *mk = v.at<double>(MCV_MASK);
    for (int j = 0; j < M; ++j) {
        double s = 0.0;
        for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < N; i += (i64)gridDim.x * WG) {
            const double y = (double)Y[i + (i64)j * ldy];
            Ya[i + (i64)j * N] = y;
            s = fma(mk[i] * y, y, s);
        }
        if (want_ss) {
            s = block_sum<WG / WAVE>(s, smem);
            if (threadIdx.x == 0) sspart[(i64)blockIdx.x * M + j] = s;
        }
    }
}

// Ya <- Ya - t q_a^T on EVERY row (the full t), with the sums of squares of the new columns over the training rows
__global__ __launch_bounds__(WG) void misscv_y_deflate_kernel(MissCvView v, i64 N, int M, int a, bool want_ss) {
    __shared__ double smem[WG / WAVE];
    double *Ya = v.at<double>(MCV_YA), *sspart = v.at<double>(MCV_YSS);
    const double *mk = v.at<double>(MCV_MASK), *t = v.at<double>(MCV_T), *q = v.at<double>(MCV_Q) + (i64)a * M;
    for (int j = 0; j < M; ++j) {
        const double qj = q[j];
        double s = 0.0;
        for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < N; i += (i64)gridDim.x * WG) {
            const double y = fma(-t[i], qj, Ya[i + (i64)j * N]);
            Ya[i + (i64)j * N] = y;
            s = fma(mk[i] * y, y, s);
        }
        if (want_ss) {
            s = block_sum<WG / WAVE>(s, smem);
            if (threadIdx.x == 0) sspart[(i64)blockIdx.x * M + j] = s;
        }
    }
}

__global__ __launch_bounds__(WAVE) void misscv_u_pick_kernel(MissCvView v, int G, int M) {
    int *words = v.at<int>(MCV_WORDS);
    miss_u_pick_body(v.at<double>(MCV_YSS), G, M, words, words + 1);
}

// u~ = m o (the column of Ya that starts the component; M = 1: its only one)
__global__ __launch_bounds__(WG) void misscv_u_start_kernel(MissCvView v, i64 N, bool multi) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i >= N) return;
    const int j = multi ? *v.at<int>(MCV_WORDS) : 0;
    v.at<double>(MCV_U)[i] = v.at<double>(MCV_MASK)[i] * v.at<double>(MCV_YA)[i + (i64)j * N];
}

// u~ = m o (Ya q_a / q_a^T q_a)
__global__ __launch_bounds__(WG) void misscv_u_kernel(MissCvView v, i64 N, int M, int a) {
    if (*v.stop(true)) return;
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i >= N) return;
    const double *Ya = v.at<double>(MCV_YA), *q = v.at<double>(MCV_Q) + (i64)a * M;
    double s = 0.0;
    for (int j = 0; j < M; ++j) s = fma(Ya[i + (i64)j * N], q[j], s);
    v.at<double>(MCV_U)[i] = v.at<double>(MCV_MASK)[i] * miss_quot(s, *v.at<double>(MCV_QQ));
}

// t~ = m o t
__global__ __launch_bounds__(WG) void misscv_tmask_kernel(MissCvView v, i64 N, bool multi) {
    const int *stop = v.stop(multi);
    if (stop && *stop) return;
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i < N) v.at<double>(MCV_TM)[i] = v.at<double>(MCV_MASK)[i] * v.at<double>(MCV_T)[i];
}

// The column sweep of fold blockIdx.z.  X != nullptr: the first component reads the caller's matrix (every fold the same one)
// and stores the fold's work copy; else the work copy in place.  It accumulates against field vf (MCV_U for w, MCV_TM for p) and
// deflates with the full t and the p of the component before.
template <typename T, int V, bool STORE, bool DEFL, bool ACC>
__global__ __launch_bounds__(WG) void misscv_col_kernel(MissCvView v, const T *X, i64 ldx, i64 ldw, i64 N, int K, int vf, bool multi) {
    T *work = v.at<T>(MCV_WORK);
    miss_col_body<T, V, STORE, DEFL, ACC>(X ? X : work, X ? ldx : ldw, work, ldw, N, K, v.at<double>(vf), v.at<double>(MCV_T),
                                          v.at<double>(MCV_P), v.at<double>(MCV_COLPART), v.stop(multi));
}
__global__ __launch_bounds__(WG) void misscv_col_finish_kernel(MissCvView v, int G, int K, int outf, bool want_ss, bool multi) {
    miss_col_finish_body(v.at<double>(MCV_COLPART), G, K, v.at<double>(outf), want_ss ? v.at<double>(MCV_SSPART) : nullptr, v.stop(multi));
}
__global__ __launch_bounds__(WG) void misscv_normalize_kernel(MissCvView v, int K, int nb, bool multi) {
    miss_normalize_body(v.at<double>(MCV_W), K, v.at<double>(MCV_SSPART), nb, v.stop(multi));
}

// The row sweep of fold blockIdx.z over its work copy: t of EVERY row from w
template <typename T, int V>
__global__ __launch_bounds__(WG) void misscv_row_kernel(MissCvView v, i64 ldw, i64 N, int K, int lrl, int kper, bool split, bool multi) {
    miss_row_body<T, V>(v.at<T>(MCV_WORK), ldw, N, K, v.at<double>(MCV_W), lrl, kper, v.at<double>(MCV_T),
                        split ? v.at<double>(MCV_TPART) : nullptr, v.stop(multi));
}
__global__ __launch_bounds__(WG) void misscv_row_finish_kernel(MissCvView v, int S, i64 N, bool multi) {
    miss_row_finish_body(v.at<double>(MCV_TPART), S, N, v.at<double>(MCV_T), v.stop(multi));
}

__global__ __launch_bounds__(WG) void misscv_yt_kernel(MissCvView v, i64 N, int M, bool multi) {
    miss_yt_body(v.at<double>(MCV_YA), N, M, v.at<double>(MCV_TM), v.at<double>(MCV_TPREV), v.at<double>(MCV_YPART), v.stop(multi));
}
// q_a, q^T q, the convergence word of the fold; iters: of the round's first fold (A per fold), may be null
__global__ __launch_bounds__(WAVE) void misscv_q_kernel(MissCvView v, int G, int M, int A, int a, int it, int max_it, bool multi,
                                                        long long *iters) {
    miss_q_body(v.at<double>(MCV_YPART), G, M, it, max_it, v.at<double>(MCV_Q) + (i64)a * M, v.at<double>(MCV_QQ),
                multi ? v.at<int>(MCV_WORDS) + 1 : nullptr, iters ? iters + (i64)blockIdx.z * A + a : nullptr);
}

// E[m][a][(f0 + f) ts + j] = Y_{a+1}[idx[f ts + j], m]: grid = (blocks of ts, M, folds); E and idx at the round's first fold
__global__ __launch_bounds__(WG) void misscv_record_kernel(MissCvView v, const long long *__restrict__ idx, int ts, i64 N, int A, i64 nobs,
                                                           int a, double *__restrict__ E) {
    const int j = (int)(blockIdx.x * WG + threadIdx.x);
    if (j >= ts) return;
    const i64 o = (i64)blockIdx.z * ts + j;
    E[(i64)blockIdx.y * (nobs * A) + (i64)a * nobs + o] = v.at<double>(MCV_YA)[idx[o] + (i64)blockIdx.y * N];
}

// *out = 1 when the convergence word of every fold of the round is set, else 0.  One workgroup, blockIdx.z = 0.
__global__ __launch_bounds__(WG) void misscv_round_done_kernel(MissCvView v, int nround, int *__restrict__ out) {
    int all = 1;
    for (int f = threadIdx.x; f < nround; f += WG)
        all &= *(reinterpret_cast<const int *>(v.base + (i64)f * v.l.bytes + v.l.off[MCV_WORDS]) + 1) != 0;
    all = __syncthreads_and(all);
    if (threadIdx.x == 0) *out = all;
}

}  // namespace plsk
