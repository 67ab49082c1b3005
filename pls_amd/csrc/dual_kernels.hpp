// dual_kernels.hpp -- the kernels of the sample-space plan (PLS_HIP_ALGO_DUAL, plan_dual.hpp): a fit of a short, wide X from
// G = X X^T (N x N) instead of from X^T X (K x K).
//
//   xxt_kernel            G = X X^T on v_mfma_f64_16x16x4_f64 (its own staging around the block core of mfma_block.hpp), the
//                         blocks on or above the diagonal, the sum over the columns of X split over workgroups;
//                         xxt_reduce_kernel adds the partial blocks in split order and mirrors them
//   dual_gy_kernel        Z = G Y_a (N x M): one wave per column of the symmetric G, the whole chip
//   dual_step_kernel      everything else of a component, N (M + a) work, ONE workgroup: direction, norm, orthogonalisation
//                         of the score against the earlier ones, loading of Y, deflation of Y_a (dual_step_body, which the
//                         cross-validation folds of dual_cv_kernels.hpp run with their training-row masks, the batched fits
//                         of dual_batch_kernels.hpp per problem and the cross-validated batches of dual_cvbatch_kernels.hpp
//                         per (problem, fold) pair)
//   dual_xtv_kernel       [W | P] = X^T [U | T diag(1/tt)], up to 64 columns per sweep over X, on the matrix cores
//   dual_r_kernel         r_a = w_a - sum_{j<a} C[j, a] r_j, a thread per row of R
//   dual_convert_kernel   Y -> fp64 working copy, fp64 scores -> T in the storage type
//
// v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15] and D[row (l >> 4) + 4 reg][col l & 15].
// In xxt the contraction index is 4 COLUMNS of X and an operand fragment 16 consecutive rows of them -- contiguous pieces of
// the column-major source, where syrk_kernels.hpp has to turn its slabs round.  Every sum is taken in a fixed order: two
// fits of the same data return the same bits.  fp32 storage becomes fp64 where a panel is staged; all arithmetic is fp64.
#pragma once
#include "common.hpp"
#include "small_kernels.hpp"
#include "syrk_kernels.hpp"

namespace plsk {

constexpr int DUAL_NMAX = 8192;  // rows of a DUAL fit: G = X X^T is N x N doubles (512 MB at the cap)
constexpr int DUAL_MMAX = MMAX;  // responses: the direction solve of one workgroup (dominant_eigvec_lds)
constexpr int DUAL_RPT = DUAL_NMAX / UPD_THREADS;  // rows per thread of dual_step_kernel

constexpr int XXT_TB = 128;           // block of G per workgroup
constexpr int XXT_KC = 16;            // columns of X per staged slab
constexpr int XXT_LDR = XXT_TB + 16;  // rows of a staged column, padded: the operand reads of a half-wave (16 rows of 2 columns) hit 32 distinct bank pairs

// blockIdx.x enumerates the nbn (nbn + 1) / 2 blocks (bi <= bj), blockIdx.y the split of the columns of X: slabs
// [y per_split, (y + 1) per_split).  Every workgroup writes its whole 128 x 128 block of part[y] (zeros when it has no slab).
template <typename T>
__global__ __launch_bounds__(256, 2) void xxt_kernel(const T *__restrict__ X, i64 ldx, int N, i64 K, int nbn, i64 per_split,
                                                     double *__restrict__ part) {
    __shared__ double As[XXT_KC * XXT_LDR], Bsm[XXT_KC * XXT_LDR];
    int bi, bj;
    tri_block(blockIdx.x, nbn, bi, bj);
    const bool diag = (bi == bj);
    const double *Bs = diag ? As : Bsm;

    const int tid = threadIdx.x;
    const int sr = tid & (XXT_TB - 1), sc = tid >> 7;  // staging: row of the panel, first of its 8 columns (sc, sc + 2, ...)
    const int ra = bi * XXT_TB + sr, rb = bj * XXT_TB + sr;
    const QuadMap q;
    f64x4 acc[4][4];
    quad_zero(acc);

    const i64 nslabs = (K + XXT_KC - 1) / XXT_KC;
    const i64 s0 = min(nslabs, (i64)blockIdx.y * per_split), s1 = min(nslabs, s0 + per_split);
    double ga[XXT_KC / 2], gb[XXT_KC / 2];
    auto load_slab = [&](i64 s) {
#pragma unroll
        for (int j = 0; j < XXT_KC / 2; ++j) {
            const i64 col = s * XXT_KC + sc + 2 * j;
            ga[j] = (ra < N && col < K) ? (double)X[ra + col * ldx] : 0.0;
            gb[j] = (!diag && rb < N && col < K) ? (double)X[rb + col * ldx] : 0.0;
        }
    };
    if (s0 < s1) load_slab(s0);
    for (i64 s = s0; s < s1; ++s) {
        __syncthreads();  // everyone is done reading the previous slab
#pragma unroll
        for (int j = 0; j < XXT_KC / 2; ++j) {
            As[(sc + 2 * j) * XXT_LDR + sr] = ga[j];
            if (!diag) Bsm[(sc + 2 * j) * XXT_LDR + sr] = gb[j];
        }
        __syncthreads();
        if (s + 1 < s1) load_slab(s + 1);  // in flight under the slab's MFMAs
#pragma unroll
        for (int kk = 0; kk < XXT_KC; kk += 4) quad_step<1, XXT_LDR>(As, Bs, q, kk, acc);
    }
    quad_store(acc, q, part + (i64)blockIdx.y * ((i64)N * N), (i64)N, bi * XXT_TB, bj * XXT_TB, N, N, false);
}

// G[i, j] = G[j, i] = sum over the splits, in split order, of the entry (i, j) on or above the diagonal.
// grid (blocks, 64), 256 threads: one entry of a block per thread.
__global__ __launch_bounds__(256) void xxt_reduce_kernel(const double *__restrict__ part, int nsplit, int N, int nbn,
                                                         double *__restrict__ G) {
    int bi, bj;
    tri_block(blockIdx.x, nbn, bi, bj);
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int i = bi * XXT_TB + (e & (XXT_TB - 1)), j = bj * XXT_TB + e / XXT_TB;
    if (i >= N || j >= N || i > j) return;
    const i64 NN = (i64)N * N;
    const double *p = part + i + (i64)j * N;
    double s = 0.0;
    for (int z = 0; z < nsplit; ++z) s += p[(i64)z * NN];
    G[i + (i64)j * N] = s;
    G[j + (i64)i * N] = s;
}

// Z[i, m] = sum_j G[j, i] Ya[j, m] (G is symmetric: column i is row i): one wave per i, lanes along j, the lane sums added by
// wave_sum.  MT >= M accumulators per lane.
template <int MT>
__global__ __launch_bounds__(256) void dual_gy_kernel(const double *__restrict__ G, const double *__restrict__ Ya, int N, int M,
                                                      double *__restrict__ Z) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;  // (wave-uniform)
    const double *g = G + (i64)i * N;
    double acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.0;
    for (int j = lane; j < N; j += 64) {
        const double gv = g[j];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < M) acc[m] = fma(gv, Ya[j + (i64)m * N], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const double s = wave_sum(acc[m]);
        if (m < M && lane == 0) Z[i + (i64)m * N] = s;
    }
}

// One component on N-sized data, one workgroup of 1024 threads; thread t owns the rows t, t + 1024, ... (at most DUAL_RPT).
//   direction   M = 1: u = Y_a, g = Z.  M > 1: S = Y_a^T Z (= XY_a^T XY_a, src/pls.cpp:406), q^ its dominant eigenvector,
//               u = Y_a q^, g = Z q^
//   nw = sqrt(u^T g) = |X^T u| (:411);  c_j = t_j^T g / tt_j, t = (g - sum_j c_j t_j) / nw (the t = X r of :419);
//   tt = t^T t, q = Y_a^T t / tt (:428), Y_a -= t q^T
// MODE = DUAL_FIT, the fit (dual_step_kernel): also stores C[j, a] = c_j / nw = p_j^T w_a, V[:, a] = u / nw, V[:, A + a] = t / tt
// and Q[:, a].
// MODE = DUAL_CV, fold blockIdx.x of a round of cross-validation folds (dual_cv_step_kernel, fold fold0 + blockIdx.x of the
// call): the fold's slice of every array -- Ya, Z (N x M), T64 (N x A), ttv (A), scr (N + A), pos (N), pred (ts x M) -- and
// the 0/1 mask of its training rows (pos < 0; dual_cv_kernels.hpp has the algebra):
//   c_j and tt sum over the training rows only; t is formed and stored for every row;
//   Y_a is deflated on the training rows; on a held-out row i of the fold pred[i, m] += t q_m and
//   E[m][fold * ts + i, a] = Y[row, m] - pred[i, m] (E: M matrices of nobs x A, column-major).
// MODE = DUAL_BATCH, problem blockIdx.x of a round of pls_hip_fit_batch (dual_batch_step_kernel, dual_batch_kernels.hpp): the
// fit's step, no mask, on the problem's slice of every array -- Ya, Z (N x M), T64, V (N x A: U only), C (A x A), Q (M x A),
// ttv (A), scr (N + A).
// MODE = DUAL_WEIGHTED, replicate blockIdx.x of a round of pls_hip_fit_resampled (resample_step_kernel, resample_kernels.hpp):
// DUAL_BATCH on the row-scaled problem (diag(s) X, diag(s) Y), s = sqrt(w) the replicate's slice of sall (N).  Zall holds
// G (s o Y_a), so the product with diag(s) G diag(s) is g = s o Z wherever Z is read; the deflation stores Y_a and, into the
// replicate's slice of Yinall (N x M), s o Y_a -- the next product's input.
// MODE = DUAL_CVB, item fold0 + blockIdx.x of a round of pls_hip_cv_press_batch (dual_cvb_step_kernel, dual_cvbatch_kernels.hpp;
// fold0 carries the round's first item): DUAL_CV on the pair (problem item / nfolds, fold item % nfolds).  pos (N per FOLD of the
// call) is indexed by the fold and shared by the problems; Y64 holds the responses of the item's held-out rows (ts x M per item);
// E (null: not asked for) is indexed by the problem.  The residual of a held-out row also goes to the item's slice of escr
// (ts x M) at the row's TEST POSITION, and one wave per response then sums their squares over the positions in a fixed order
// into press[m + a M] of the item (M x A per item): the sum does not depend on which thread owns which row.
// Stores T64[:, a] = t and ttv[a].  scr: N + A doubles (g, then c).
enum { DUAL_FIT = 0, DUAL_CV = 1, DUAL_BATCH = 2, DUAL_WEIGHTED = 3, DUAL_CVB = 4 };
template <int MODE>
__device__ __forceinline__ void dual_step_body(const double *__restrict__ Zall, double *__restrict__ Yall, double *__restrict__ Tall,
                                               double *__restrict__ ttall, double *__restrict__ scrall, int N, int M, int A, int a,
                                               int power_iters, double *__restrict__ V, double *__restrict__ Q,
                                               double *__restrict__ C, const int *__restrict__ posall, double *__restrict__ predall,
                                               const double *__restrict__ Y64, double *__restrict__ E, int ts, i64 fold0, i64 nobs,
                                               const double *__restrict__ sall = nullptr, double *__restrict__ Yinall = nullptr,
                                               i64 nfolds = 1, double *__restrict__ escrall = nullptr,
                                               double *__restrict__ pressall = nullptr) {
    __shared__ UpdShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr bool CVB = MODE == DUAL_CVB, CV = MODE == DUAL_CV || CVB, WT = MODE == DUAL_WEIGHTED;
    const i64 f = MODE != DUAL_FIT ? blockIdx.x : 0;
    const double *Z = Zall + f * M * N;
    double *Ya = Yall + f * M * N, *T64 = Tall + f * (i64)N * A, *ttv = ttall + f * A;
    double *gbuf = scrall + f * (N + A), *cbuf = gbuf + N;
    const i64 prob = CVB ? (fold0 + f) / nfolds : 0, fold = CVB ? (fold0 + f) % nfolds : fold0 + f;  // (CV)
    const int *pos = CV ? posall + (CVB ? fold : f) * N : nullptr;
    double *pred = CV ? predall + f * ts * M : nullptr;
    const double *sv = WT ? sall + f * N : nullptr;
    double *Yin = WT ? Yinall + f * M * N : nullptr;
    if constexpr (MODE == DUAL_BATCH || WT) {
        V += f * N * A;
        Q += f * M * A;
        C += f * A * A;
    }
    double u[DUAL_RPT], g[DUAL_RPT], t[DUAL_RPT];
    int ps[DUAL_RPT];  // (CV) the row's position in the fold's test set, -1: a training row
    if (M > 1) {
        // the M (M + 1) / 2 entries of S = Y_a^T Z on or above the diagonal: a wave per entry
        for (int e = wv; e < M * (M + 1) / 2; e += UPD_WAVES) {
            int i, j;
            tri_block(e, M, i, j);
            double s = 0.0;
            if constexpr (WT) {
                for (int n = lane; n < N; n += 64) s = fma(Ya[n + (i64)i * N], sv[n] * Z[n + (i64)j * N], s);
            } else {
                for (int n = lane; n < N; n += 64) s = fma(Ya[n + (i64)i * N], Z[n + (i64)j * N], s);
            }
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
        u[i] = g[i] = 0.0;
        ps[i] = -1;
        if (n < N) {
            if constexpr (CV) ps[i] = pos[n];
            if (M > 1) {
                for (int m = 0; m < M; ++m) {
                    u[i] = fma(Ya[n + (i64)m * N], sh.qs[m], u[i]);
                    if constexpr (WT) g[i] = fma(sv[n] * Z[n + (i64)m * N], sh.qs[m], g[i]);
                    else g[i] = fma(Z[n + (i64)m * N], sh.qs[m], g[i]);
                }
            } else {
                u[i] = Ya[n];
                if constexpr (WT) g[i] = sv[n] * Z[n];
                else g[i] = Z[n];
            }
            gbuf[n] = g[i];
        }
        part = fma(u[i], g[i], part);  // (CV: u is zero on the held-out rows)
    }
    const double nw = sqrt(block_sum<UPD_WAVES>(part, sh.sred));  // (its barriers publish gbuf)
    for (int j = wv; j < a; j += UPD_WAVES) {  // a wave per earlier score (CV: the training rows)
        double s = 0.0;
        for (int n = lane; n < N; n += 64) s = fma((!CV || pos[n] < 0) ? T64[n + (i64)j * N] : 0.0, gbuf[n], s);
        s = wave_sum(s) / ttv[j];
        if (lane == 0) {
            cbuf[j] = s;
            if constexpr (!CV) C[j + (i64)a * A] = s / nw;
        }
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
    for (int m = wv; m < M; m += UPD_WAVES) {  // a wave per response (CV: Y_a is zero on the held-out rows)
        double s = 0.0;
        for (int n = lane; n < N; n += 64) s = fma(Ya[n + (i64)m * N], T64[n + (i64)a * N], s);
        s = wave_sum(s) / tt;
        if (lane == 0) {
            sh.qs[m] = s;
            if constexpr (!CV) Q[m + (i64)a * M] = s;
        }
    }
    __syncthreads();
    if (tid == 0) ttv[a] = tt;
#pragma unroll
    for (int i = 0; i < DUAL_RPT; ++i) {
        const int n = tid + i * UPD_THREADS;
        if (n >= N) continue;
        if (ps[i] < 0) {
            if constexpr (WT) {
                for (int m = 0; m < M; ++m) {
                    const double y = fma(-t[i], sh.qs[m], Ya[n + (i64)m * N]);
                    Ya[n + (i64)m * N] = y;
                    Yin[n + (i64)m * N] = sv[n] * y;
                }
            } else {
                for (int m = 0; m < M; ++m) Ya[n + (i64)m * N] = fma(-t[i], sh.qs[m], Ya[n + (i64)m * N]);
            }
            if constexpr (!CV) {
                V[n + (i64)a * N] = u[i] / nw;
                if constexpr (MODE == DUAL_FIT) V[n + (i64)(A + a) * N] = t[i] / tt;
            }
        } else {
            double *e = E + (prob * M * A + a) * nobs + fold * ts + ps[i];
            for (int m = 0; m < M; ++m) {
                const double p = fma(t[i], sh.qs[m], pred[ps[i] + (i64)m * ts]);
                pred[ps[i] + (i64)m * ts] = p;
                if constexpr (CVB) {
                    const double r = Y64[(f * M + m) * ts + ps[i]] - p;
                    escrall[(f * M + m) * ts + ps[i]] = r;
                    if (E) e[(i64)m * nobs * A] = r;
                } else {
                    e[(i64)m * nobs * A] = Y64[n + (i64)m * N] - p;
                }
            }
        }
    }
    if constexpr (CVB) {
        __syncthreads();  // (publishes escr)
        for (int m = wv; m < M; m += UPD_WAVES) {  // a wave per response: the held-out rows by test position
            const double *r = escrall + (f * M + m) * ts;
            double s = 0.0;
            for (int i = lane; i < ts; i += 64) s = fma(r[i], r[i], s);
            s = wave_sum(s);
            if (lane == 0) pressall[f * M * A + m + (i64)a * M] = s;
        }
    }
}

__global__ __launch_bounds__(UPD_THREADS) void dual_step_kernel(const double *__restrict__ Z, double *__restrict__ Ya,
                                                                double *__restrict__ T64, double *__restrict__ V,
                                                                double *__restrict__ Q, double *__restrict__ C,
                                                                double *__restrict__ ttv, double *__restrict__ scr, int N, int M,
                                                                int A, int a, int power_iters) {
    dual_step_body<DUAL_FIT>(Z, Ya, T64, ttv, scr, N, M, A, a, power_iters, V, Q, C, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}

constexpr int XTV_KB = 64;   // columns of X per workgroup
constexpr int XTV_RC = 64;   // rows per staged chunk
constexpr int XTV_NC = 64;   // columns of V per sweep
constexpr int XTV_LD = XTV_RC + 2;  // operand reads (lane: column l & 15, row l >> 4) hit 32 distinct bank pairs per half-wave
constexpr size_t XTV_LDS_BYTES = (size_t)(XTV_KB + XTV_NC) * XTV_LD * 8;

// out[k, c] = sum_n X[n, k] V[n, c0 + c] for the 64 columns k of this workgroup and nc <= 64 columns c: wave w owns the 16
// columns k0 + 16 w .. of X (the MFMA's rows), the tiles of 16 columns of V are its columns, 4 rows of X the contraction.
// Column c0 + c of V goes to W[:, c0 + c] when c0 + c < A, to P[:, c0 + c - A] otherwise; the block leaves through LDS so
// that every store is 64 consecutive rows of an output column.
// NCT: tiles of 16 columns of V the instantiation carries, ceil(nc / 16).
template <typename T, int NCT>
__global__ __launch_bounds__(256, 2) void dual_xtv_kernel(const T *__restrict__ X, i64 ldx, int N, i64 K, const double *__restrict__ V,
                                                          int c0, int nc, int A, double *__restrict__ W, double *__restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xtv_raw[];
    double *Xs = reinterpret_cast<double *>(xtv_raw), *Vs = Xs + XTV_KB * XTV_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const i64 k0 = (i64)blockIdx.x * XTV_KB;
    f64x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    double gx[16], gv[16];
    auto load_chunk = [&](int n0) {  // thread: row n0 + lane of the columns wv, wv + 4, ...
        const int n = n0 + lane;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = wv + 4 * j;
            gx[j] = (n < N && k0 + c < K) ? (double)X[n + (k0 + c) * ldx] : 0.0;
            gv[j] = (n < N && c < nc) ? V[n + (i64)(c0 + c) * N] : 0.0;
        }
    };
    load_chunk(0);
    for (int n0 = 0; n0 < N; n0 += XTV_RC) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            Xs[(wv + 4 * j) * XTV_LD + lane] = gx[j];
            Vs[(wv + 4 * j) * XTV_LD + lane] = gv[j];
        }
        __syncthreads();
        if (n0 + XTV_RC < N) load_chunk(n0 + XTV_RC);
#pragma unroll 2  // (fully unrolled the 80 operand reads are hoisted and spill)
        for (int kk = 0; kk < XTV_RC; kk += 4) {
            const double xa = Xs[(16 * wv + li) * XTV_LD + kk + lq];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, Vs[(16 * ct + li) * XTV_LD + kk + lq], acc[ct], 0, 0, 0);
        }
    }
    __syncthreads();
    double *Os = Xs;  // [column c][row k of the block]
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) Os[(16 * ct + li) * XTV_LD + 16 * wv + lq + 4 * r] = acc[ct][r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = wv + 4 * j, cg = c0 + c;
        if (c < nc && k0 + lane < K) {
            double *o = cg < A ? W + (i64)cg * K : P + (i64)(cg - A) * K;
            o[k0 + lane] = Os[c * XTV_LD + lane];
        }
    }
}

// r_a = w_a - sum_{j<a} C[j, a] r_j (src/pls.cpp:412-416 with p_j^T w_a = C[j, a]): a thread per row, no reduction over K;
// C[j, a] is the same address in every lane (the scalar cache).
__global__ __launch_bounds__(256) void dual_r_kernel(const double *__restrict__ W, const double *__restrict__ C, i64 K, int A,
                                                     double *__restrict__ R) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    for (int a = 0; a < A; ++a) {
        double r = W[k + (i64)a * K];
        for (int j = 0; j < a; ++j) r = fma(-C[j + (i64)a * A], R[k + (i64)j * K], r);
        R[k + (i64)a * K] = r;
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void dual_convert_kernel(const TI *__restrict__ src, i64 lds, TO *__restrict__ dst, i64 ldd, int N,
                                                           int cols) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= (i64)N * cols) return;
    const i64 n = e % N, c = e / N;
    dst[n + c * ldd] = (TO)src[n + c * lds];
}

}  // namespace plsk
