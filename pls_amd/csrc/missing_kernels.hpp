// missing_kernels.hpp -- NIPALS with the missing cells of X skipped (pls_hip_fit_missing, pls_hip_scores_missing,
// pls_hip_colwise_z_scores_missing; plan_missing.hpp enqueues them).  NaN in X marks a missing cell; obs(i,k) = X[i,k] is no NaN.
//   miss_col_kernel          num[k], den[k] = sum over the OBSERVED rows of column k of x v_i, v_i^2 (w from u, p from t); the same
//                            template deflates on the way (x - t_prev[i] p_prev[k] in registers, stored to the work copy)
//   miss_row_kernel          num[i], den[i] = sum over the observed columns of row i of x w_k, w_k^2 (t from w); tall X in one
//                            pass, short wide X split over K with partials and miss_row_finish_kernel
//   the row sweep's parts    miss_obs_xw / miss_obs_xx (the observed-cell steps), miss_load_rows, miss_row_walk<T, V, U, NACC>
//                            with a cell policy, miss_lanes_meet, miss_ranges_sum: written once, for this file's row sweep and
//                            for the streaming sweep of xdiag_missing_kernels.hpp
//   the small kernels       normalisation of w, q, t^T t, the convergence word, u = Y q / q^T q, the deflation of Y, the R recursion
//   miss_colmoments_kernel   count, mean, M2 of the observed cells of a column in one sweep; miss_zscale_kernel scales
// All sums fp64 and in a fixed order, no atomics; a quotient whose denominator is exactly 0 (no observed cell) is 0.  The mask
// test is x == x: the library is built without -ffast-math, with it the test would be compiled away.
// Every kernel of an iteration of the M > 1 loop reads the device convergence word `stop` first and returns when it is set.
// The sweeps, their finish and normalise kernels and the one-wave kernels of the Y side are written as *_body functions with a
// __global__ wrapper each: missing_cv_kernels.hpp wraps the same bodies once more, with the fold of a round in blockIdx.z.
#pragma once
#include "common.hpp"
#include "miss_layout.hpp"  // MISS_KC, MISS_RF_ROWS, the sweep geometry

namespace plsk {

constexpr int MISS_MAX_M = 32;  // responses the entry point takes

__device__ __forceinline__ double miss_quot(double num, double den) { return den == 0.0 ? 0.0 : num / den; }

// The observed-cell steps, the only places the mask test of a sweep is written: a NaN cell leaves the sums as they are.
//   num += x w, den += w^2 (w: the factor the cell is multiplied with)
__device__ __forceinline__ void miss_obs_xw(double x, double w, double &num, double &den) {
    const bool ob = x == x;
    num = ob ? fma(x, w, num) : num;
    den = ob ? fma(w, w, den) : den;
}
//   q += x^2, cnt += 1 (a double on the streaming route, an int in the resident tile)
template <typename C>
__device__ __forceinline__ void miss_obs_xx(double x, double &q, C &cnt) {
    const bool ob = x == x;
    q = ob ? fma(x, x, q) : q;
    cnt = ob ? cnt + 1 : cnt;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Column sweep.  grid = (column groups ceil(K / MISS_KC), row groups G): the layout of xty_kernel with the two grid dimensions
// swapped (K may exceed 65,535 groups).  A workgroup walks the row chunks blockIdx.y, blockIdx.y + G, ... of WG * V rows.
//   STORE   the (deflated) cell goes to dst (src == dst: in place; src = the caller's matrix for the first component)
//   DEFL    x <- x - tp[i] pp[k] before it is stored and used (a NaN stays a NaN)
//   ACC     part[blockIdx.y][k] = {sum_obs x v_i, sum_obs v_i^2} (off: pls_hip_scores_missing only deflates)
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int V, bool STORE, bool DEFL, bool ACC>
__device__ __forceinline__ void miss_col_body(const T *src, i64 lds_, T *dst, i64 ldd, i64 N, int K, const double *__restrict__ v,
                                              const double *__restrict__ tp, const double *__restrict__ pp,
                                              double *__restrict__ part, const int *__restrict__ stop) {
    constexpr int KC = MISS_KC;
    if (stop && *stop) return;
    __shared__ double red[WG / WAVE][2 * KC];
    const i64 k0 = (i64)blockIdx.x * KC;
    const int kn = (int)(K - k0 < KC ? K - k0 : KC);
    double an[KC], ad[KC], pk[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        an[kc] = 0.0;
        ad[kc] = 0.0;
        pk[kc] = (DEFL && kc < kn) ? pp[k0 + kc] : 0.0;
    }
    constexpr i64 CH = (i64)WG * V;
    for (i64 c = blockIdx.y; c * CH < N; c += gridDim.y) {
        const i64 i0 = c * CH + (i64)threadIdx.x * V;
        if (i0 + V <= N) {
            double vv[V], tv[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                vv[j] = ACC ? v[i0 + j] : 0.0;
                tv[j] = DEFL ? tp[i0 + j] : 0.0;
            }
            Pack<T, V> x[KC];
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
                if (kc < kn) x[kc] = ld_pack_nt<T, V>(src + i0 + (k0 + kc) * lds_);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
                if (kc < kn) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        double xd = (double)x[kc].v[j];
                        if (DEFL) xd = fma(-tv[j], pk[kc], xd);
                        if (ACC) miss_obs_xw(xd, vv[j], an[kc], ad[kc]);
                        x[kc].v[j] = (T)xd;
                    }
                    if (STORE) st_pack_nt<T, V>(dst + i0 + (k0 + kc) * ldd, x[kc]);
                }
        } else if (i0 < N) {
            const int nv = (int)(N - i0);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (j < nv) {
                    const double vj = ACC ? v[i0 + j] : 0.0, tj = DEFL ? tp[i0 + j] : 0.0;
#pragma unroll
                    for (int kc = 0; kc < KC; ++kc)
                        if (kc < kn) {
                            double xd = (double)src[i0 + j + (k0 + kc) * lds_];
                            if (DEFL) xd = fma(-tj, pk[kc], xd);
                            if (ACC) miss_obs_xw(xd, vj, an[kc], ad[kc]);
                            if (STORE) dst[i0 + j + (k0 + kc) * ldd] = (T)xd;
                        }
                }
        }
    }
    if (!ACC) return;
    // workgroup reduction: butterfly per value, then waves in order
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        const double sn = wave_sum(an[kc]), sd = wave_sum(ad[kc]);
        if (lane == 0) {
            red[w][2 * kc] = sn;
            red[w][2 * kc + 1] = sd;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * KC && (int)(threadIdx.x >> 1) < kn) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < WG / WAVE; ++i) s += red[i][threadIdx.x];
        part[((i64)blockIdx.y * K + k0) * 2 + threadIdx.x] = s;
    }
}
template <typename T, int V, bool STORE, bool DEFL, bool ACC>
__global__ __launch_bounds__(WG) void miss_col_kernel(const T *src, i64 lds_, T *dst, i64 ldd, i64 N, int K, const double *__restrict__ v,
                                                      const double *__restrict__ tp, const double *__restrict__ pp,
                                                      double *__restrict__ part, const int *__restrict__ stop) {
    miss_col_body<T, V, STORE, DEFL, ACC>(src, lds_, dst, ldd, N, K, v, tp, pp, part, stop);
}

// out[k] = num / den with the G partial rows added in order; sspart[blockIdx.x] = this block's sum of out[k]^2 (w only)
__device__ __forceinline__ void miss_col_finish_body(const double *__restrict__ part, int G, int K, double *__restrict__ out,
                                                     double *__restrict__ sspart, const int *__restrict__ stop) {
    __shared__ double smem[WG / WAVE];
    if (stop && *stop) return;
    const i64 k = (i64)blockIdx.x * WG + threadIdx.x;
    double val = 0.0;
    if (k < K) {
        double num = 0.0, den = 0.0;
        for (int g = 0; g < G; ++g) {
            num += part[((i64)g * K + k) * 2];
            den += part[((i64)g * K + k) * 2 + 1];
        }
        val = miss_quot(num, den);
        out[k] = val;
    }
    if (sspart) {
        const double s = block_sum<WG / WAVE>(val * val, smem);
        if (threadIdx.x == 0) sspart[blockIdx.x] = s;
    }
}
__global__ __launch_bounds__(WG) void miss_col_finish_kernel(const double *__restrict__ part, int G, int K, double *__restrict__ out,
                                                             double *__restrict__ sspart, const int *__restrict__ stop) {
    miss_col_finish_body(part, G, K, out, sspart, stop);
}

// w <- w / |w|_2, the nb block sums of squares added in a fixed order by every workgroup (|w| = 0: w stays 0)
__device__ __forceinline__ void miss_normalize_body(double *__restrict__ w, int K, const double *__restrict__ sspart, int nb,
                                                    const int *__restrict__ stop) {
    __shared__ double smem[WG / WAVE];
    if (stop && *stop) return;
    double s = 0.0;
    for (int j = threadIdx.x; j < nb; j += WG) s += sspart[j];
    const double nrm = sqrt(block_sum<WG / WAVE>(s, smem));
    const i64 k = (i64)blockIdx.x * WG + threadIdx.x;
    if (k < K) w[k] = miss_quot(w[k], nrm);
}
__global__ __launch_bounds__(WG) void miss_normalize_kernel(double *__restrict__ w, int K, const double *__restrict__ sspart, int nb,
                                                            const int *__restrict__ stop) {
    miss_normalize_body(w, K, sspart, nb, stop);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Row sweep, shared by the fit, the folds (over the work copy) and the streaming diagnostics (over the caller's X).
// The workgroup is RL = 1 << lrl row lanes x CL = WG / RL column lanes: lane (r, c) owns the V rows (blockIdx.x RL + r) V ... and
// walks the columns kb + c, kb + c + CL, ... of the K range blockIdx.y (miss_row_split), U columns in flight per batch, then a
// tail; the column lanes of a row meet in LDS in the order of c.  A cell policy says what the factor of column k is and what
// happens to the cells of a batch between their load and their accumulation.
//   acc[0], acc[1]   num, den = sum over the observed columns of x w_k, w_k^2
//   acc[2], acc[3]   NACC = 4 only: sum of x^2, observed cells
//   PADDED           the work copy (16-byte columns: ldx a multiple of V): every lane loads whole packs, the padding rows are
//                    read and never used.  Else rows beyond N are never read: the lanes are split ONCE into those whose V rows
//                    all exist and those of the one pack that straddles row N.  (A guard per load, or the split on the work copy
//                    too, costs the fit's sweep its 8 waves per SIMD: profiles/missing_rows/resources.md.)
// ------------------------------------------------------------------------------------------------------------------------------
// V rows i .. i + V - 1 of one column as fp64; whole = (i + V <= N): one pack, else element by element -- rows beyond N are 0,
// never used and never read.  The row sweep passes `whole` as a constant (it splits its lanes once), so its loops test nothing
// per load.
template <typename T, int V>
__device__ __forceinline__ void miss_load_rows(const T *__restrict__ col, i64 i, i64 N, bool whole, double (&x)[V]) {
    if (whole) {
        const Pack<T, V> p = ld_pack_nt<T, V>(col + i);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (double)p.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (i + j < N) ? (double)col[i + j] : 0.0;
    }
}

// the cell policy of the fit: the cell as it was loaded
struct MissCellAsLoaded {
    const double *__restrict__ w;
    __device__ __forceinline__ double factor(i64 k) const { return w[k]; }
    template <int U, int V>
    __device__ __forceinline__ void apply(double (&)[U][V], i64, i64, int) const {}
};

// the column lanes of a row meet in LDS in the order of c; the lanes c == 0 leave with the sums of their rows
template <int NACC, int V>
__device__ __forceinline__ void miss_lanes_meet(double (&acc)[NACC][V], int RL, int CL, int r, int c) {
    __shared__ double sm[WG][NACC * V];
    if (CL == 1) return;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int n = 0; n < NACC; ++n) sm[threadIdx.x][NACC * v + n] = acc[n][v];
    __syncthreads();
    if (c != 0) return;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        double s[NACC] = {};
        for (int cc = 0; cc < CL; ++cc)
#pragma unroll
            for (int n = 0; n < NACC; ++n) s[n] += sm[r + cc * RL][NACC * v + n];
#pragma unroll
        for (int n = 0; n < NACC; ++n) acc[n][v] = s[n];
    }
}

// One lane's columns k, k + CL, ... in batches of U for as long as a whole batch lies below ke; returns the first column left.
// U = 1 is the tail loop.
template <typename T, int V, int U, int NACC, typename Cell>
__device__ __forceinline__ i64 miss_lane_batches(const T *__restrict__ X, i64 ldx, i64 N, i64 i0, bool whole, i64 k, i64 ke, int CL,
                                                 const Cell &cell, double (&acc)[NACC][V]) {
    for (; k + (i64)(U - 1) * CL < ke; k += (i64)U * CL) {
        double x[U][V], wk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            miss_load_rows<T, V>(X + (k + (i64)u * CL) * ldx, i0, N, whole, x[u]);
            wk[u] = cell.factor(k + (i64)u * CL);
        }
        cell.apply(x, i0, k, CL);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                miss_obs_xw(x[u][v], wk[u], acc[0][v], acc[1][v]);
                if constexpr (NACC == 4) miss_obs_xx(x[u][v], acc[2][v], acc[3][v]);
            }
    }
    return k;
}

// One lane's walk and the meet.  True for the lanes that hold the sums of rows i0 .. i0 + V - 1 of this K range in acc.
template <typename T, int V, int U, int NACC, bool PADDED, typename Cell>
__device__ __forceinline__ bool miss_row_walk(const T *__restrict__ X, i64 ldx, i64 N, int K, int lrl, int kper, const Cell &cell,
                                              double (&acc)[NACC][V], i64 &i0) {
    static_assert(NACC == 2 || NACC == 4, "num, den and, for the diagnostics, q and the count");
    const int RL = 1 << lrl, CL = WG >> lrl;
    const int r = threadIdx.x & (RL - 1), c = threadIdx.x >> lrl;
    i0 = ((i64)blockIdx.x * RL + r) * V;
    const i64 kb = (i64)blockIdx.y * kper;
    const i64 ke = kb + kper < K ? kb + kper : K;
#pragma unroll
    for (int n = 0; n < NACC; ++n)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[n][v] = 0.0;
    if (PADDED ? i0 < N : i0 + V <= N) {
        const i64 k = miss_lane_batches<T, V, U>(X, ldx, N, i0, true, kb + c, ke, CL, cell, acc);
        miss_lane_batches<T, V, 1>(X, ldx, N, i0, true, k, ke, CL, cell, acc);
    } else if (i0 < N) {  // the lanes of the one row pack that straddles N: the same walk with element loads
        const i64 k = miss_lane_batches<T, V, U>(X, ldx, N, i0, false, kb + c, ke, CL, cell, acc);
        miss_lane_batches<T, V, 1>(X, ldx, N, i0, false, k, ke, CL, cell, acc);
    }
    miss_lanes_meet<NACC, V>(acc, RL, CL, r, c);
    return c == 0;
}

//   tpart == nullptr (one K range)  t[i] = num / den
//   else                            tpart[blockIdx.y][i] = {num, den}; miss_row_finish_kernel adds the ranges in order
template <typename T, int V>
__device__ __forceinline__ void miss_row_body(const T *__restrict__ X, i64 ldx, i64 N, int K, const double *__restrict__ w, int lrl,
                                              int kper, double *__restrict__ t, double *__restrict__ tpart,
                                              const int *__restrict__ stop) {
    if (stop && *stop) return;
    double acc[2][V];
    i64 i0;
    if (!miss_row_walk<T, V, 8, 2, true>(X, ldx, N, K, lrl, kper, MissCellAsLoaded{w}, acc, i0)) return;
#pragma unroll
    for (int j = 0; j < V; ++j)
        if (i0 + j < N) {
            if (tpart) {
                st_pack<double, 2>(tpart + ((i64)blockIdx.y * N + i0 + j) * 2, Pack<double, 2>{{acc[0][j], acc[1][j]}});
            } else {
                t[i0 + j] = miss_quot(acc[0][j], acc[1][j]);
            }
        }
}
template <typename T, int V>
__global__ __launch_bounds__(WG) void miss_row_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, const double *__restrict__ w, int lrl,
                                                      int kper, double *__restrict__ t, double *__restrict__ tpart,
                                                      const int *__restrict__ stop) {
    miss_row_body<T, V>(X, ldx, N, K, w, lrl, kper, t, tpart, stop);
}

// The S ranges of a row, NACC values each.  A workgroup owns MISS_RF_ROWS (miss_layout.hpp) rows; range lane sl adds the ranges
// sl, sl + SL, ... in order (SL = WG / MISS_RF_ROWS, four loads in flight: one dependent chain of S loads per row cost more than
// the sweep), then the SL lanes of a row meet in LDS in the order of sl.  True for the lane that holds the sums of row i.
template <int NACC>
__device__ __forceinline__ bool miss_ranges_sum(const double *__restrict__ part, int S, i64 N, double (&sum)[NACC], i64 &i) {
    constexpr int RR = MISS_RF_ROWS, SL = WG / RR;
    __shared__ double sm[SL][RR][NACC];
    const int ri = threadIdx.x % RR, sl = threadIdx.x / RR;
    i = (i64)blockIdx.x * RR + ri;
#pragma unroll
    for (int n = 0; n < NACC; ++n) sum[n] = 0.0;
    if (i < N) {
#pragma unroll 4
        for (int s = sl; s < S; s += SL) {
            const double *p = part + ((i64)s * N + i) * NACC;
#pragma unroll
            for (int n = 0; n < NACC; n += 2) {
                const Pack<double, 2> v = ld_pack<double, 2>(p + n);
                sum[n] += v.v[0];
                sum[n + 1] += v.v[1];
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NACC; ++n) sm[sl][ri][n] = sum[n];
    __syncthreads();
    if (sl != 0 || i >= N) return false;
#pragma unroll
    for (int n = 0; n < NACC; ++n) {
        sum[n] = 0.0;
#pragma unroll
        for (int q = 0; q < SL; ++q) sum[n] += sm[q][ri][n];
    }
    return true;
}

// t[i] = num / den over the S ranges
__device__ __forceinline__ void miss_row_finish_body(const double *__restrict__ tpart, int S, i64 N, double *__restrict__ t,
                                                     const int *__restrict__ stop) {
    if (stop && *stop) return;
    double sum[2];
    i64 i;
    if (miss_ranges_sum<2>(tpart, S, N, sum, i)) t[i] = miss_quot(sum[0], sum[1]);
}
__global__ __launch_bounds__(WG) void miss_row_finish_kernel(const double *__restrict__ tpart, int S, i64 N, double *__restrict__ t,
                                                             const int *__restrict__ stop) {
    miss_row_finish_body(tpart, S, N, t, stop);
}

// ------------------------------------------------------------------------------------------------------------------------------
// The Y side: Ya is the fp64 work copy of Y (N x M, ld N).  Row-chunked kernels run G workgroups and leave one partial row each.
// ------------------------------------------------------------------------------------------------------------------------------
// Ya = Y; sspart[blockIdx.x][j] = this workgroup's sum of squares of column j (M > 1: the choice of u)
template <typename T>
__global__ __launch_bounds__(WG) void miss_y_init_kernel(const T *__restrict__ Y, i64 ldy, i64 N, int M, double *__restrict__ Ya,
                                                         double *__restrict__ sspart) {
    __shared__ double smem[WG / WAVE];
    for (int j = 0; j < M; ++j) {
        double s = 0.0;
        for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < N; i += (i64)gridDim.x * WG) {
            const double y = (double)Y[i + (i64)j * ldy];
            Ya[i + (i64)j * N] = y;
            s = fma(y, y, s);
        }
        if (sspart) {
            s = block_sum<WG / WAVE>(s, smem);
            if (threadIdx.x == 0) sspart[(i64)blockIdx.x * M + j] = s;
        }
    }
}

// Ya <- Ya - t q^T, with the sums of squares of the new columns
__global__ __launch_bounds__(WG) void miss_y_deflate_kernel(double *__restrict__ Ya, i64 N, int M, const double *__restrict__ t,
                                                            const double *__restrict__ q, double *__restrict__ sspart) {
    __shared__ double smem[WG / WAVE];
    for (int j = 0; j < M; ++j) {
        const double qj = q[j];
        double s = 0.0;
        for (i64 i = (i64)blockIdx.x * WG + threadIdx.x; i < N; i += (i64)gridDim.x * WG) {
            const double y = fma(-t[i], qj, Ya[i + (i64)j * N]);
            Ya[i + (i64)j * N] = y;
            s = fma(y, y, s);
        }
        if (sspart) {
            s = block_sum<WG / WAVE>(s, smem);
            if (threadIdx.x == 0) sspart[(i64)blockIdx.x * M + j] = s;
        }
    }
}

// One wave: the column of Ya with the largest sum of squares (lowest index on ties) -> *jstar; clears the convergence word
__device__ __forceinline__ void miss_u_pick_body(const double *__restrict__ sspart, int G, int M, int *__restrict__ jstar,
                                                 int *__restrict__ stop) {
    __shared__ double ss[MISS_MAX_M];
    for (int j = 0; j < M; ++j) {
        double s = 0.0;
        for (int g = threadIdx.x; g < G; g += WAVE) s += sspart[(i64)g * M + j];
        s = wave_sum(s);
        if (threadIdx.x == 0) ss[j] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int j = 1; j < M; ++j)
            if (ss[j] > ss[best]) best = j;
        *jstar = best;
        *stop = 0;
    }
}
__global__ __launch_bounds__(WAVE) void miss_u_pick_kernel(const double *__restrict__ sspart, int G, int M, int *__restrict__ jstar,
                                                           int *__restrict__ stop) {
    miss_u_pick_body(sspart, G, M, jstar, stop);
}

__global__ __launch_bounds__(WG) void miss_u_copy_kernel(const double *__restrict__ Ya, i64 N, const int *__restrict__ jstar,
                                                         double *__restrict__ u) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i < N) u[i] = Ya[i + (i64)(*jstar) * N];
}

// part[blockIdx.x] = {Ya^T t (M), t^T t, |t - tprev|^2} of this workgroup's rows; tprev <- t
__device__ __forceinline__ void miss_yt_body(const double *__restrict__ Ya, i64 N, int M, const double *__restrict__ t,
                                             double *__restrict__ tprev, double *__restrict__ part, const int *__restrict__ stop) {
    __shared__ double smem[WG / WAVE];
    if (stop && *stop) return;
    const i64 i_first = (i64)blockIdx.x * WG + threadIdx.x, step = (i64)gridDim.x * WG;
    double *out = part + (i64)blockIdx.x * (M + 2);
    for (int j = 0; j < M; ++j) {
        double s = 0.0;
        for (i64 i = i_first; i < N; i += step) s = fma(Ya[i + (i64)j * N], t[i], s);
        s = block_sum<WG / WAVE>(s, smem);
        if (threadIdx.x == 0) out[j] = s;
    }
    double tt = 0.0, dd = 0.0;
    for (i64 i = i_first; i < N; i += step) {
        const double ti = t[i], d = ti - tprev[i];
        tt = fma(ti, ti, tt);
        dd = fma(d, d, dd);
        tprev[i] = ti;
    }
    tt = block_sum<WG / WAVE>(tt, smem);
    dd = block_sum<WG / WAVE>(dd, smem);
    if (threadIdx.x == 0) {
        out[M] = tt;
        out[M + 1] = dd;
    }
}
__global__ __launch_bounds__(WG) void miss_yt_kernel(const double *__restrict__ Ya, i64 N, int M, const double *__restrict__ t,
                                                     double *__restrict__ tprev, double *__restrict__ part, const int *__restrict__ stop) {
    miss_yt_body(Ya, N, M, t, tprev, part, stop);
}

// One wave: q = Ya^T t / t^T t -> q (a column of Q), *qq = q^T q; the end of iteration `it` of a component: done when there is one
// response, when it >= 2 and |t - tprev|^2 <= 1e-20 t^T t, or at max_it -- then the convergence word is set and *iters = it
__device__ __forceinline__ void miss_q_body(const double *__restrict__ part, int G, int M, int it, int max_it,
                                            double *__restrict__ q, double *__restrict__ qq, int *__restrict__ stop,
                                            long long *__restrict__ iters) {
    __shared__ double val[MISS_MAX_M + 2];
    if (stop && *stop) return;
    for (int v = 0; v < M + 2; ++v) {  // the lanes share the G partial rows of a value, then the butterfly: a fixed order
        double s = 0.0;
        for (int g = threadIdx.x; g < G; g += WAVE) s += part[(i64)g * (M + 2) + v];
        s = wave_sum(s);
        if (threadIdx.x == 0) val[v] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tt = val[M], dd = val[M + 1];
        double s = 0.0;
        for (int j = 0; j < M; ++j) {
            const double qj = miss_quot(val[j], tt);
            q[j] = qj;
            s = fma(qj, qj, s);
        }
        *qq = s;
        const bool done = M == 1 || (it >= 2 && dd <= 1e-20 * tt) || it >= max_it;
        if (done) {
            if (stop) *stop = 1;
            if (iters) *iters = it;
        }
    }
}
__global__ __launch_bounds__(WAVE) void miss_q_kernel(const double *__restrict__ part, int G, int M, int it, int max_it,
                                                      double *__restrict__ q, double *__restrict__ qq, int *__restrict__ stop,
                                                      long long *__restrict__ iters) {
    miss_q_body(part, G, M, it, max_it, q, qq, stop, iters);
}

// u = Ya q / q^T q
__global__ __launch_bounds__(WG) void miss_u_kernel(const double *__restrict__ Ya, i64 N, int M, const double *__restrict__ q,
                                                    const double *__restrict__ qq, double *__restrict__ u, const int *__restrict__ stop) {
    if (stop && *stop) return;
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int j = 0; j < M; ++j) s = fma(Ya[i + (i64)j * N], q[j], s);
    u[i] = miss_quot(s, *qq);
}

// a column of T / S in the storage type from the fp64 scores
template <typename T>
__global__ __launch_bounds__(WG) void miss_store_scores_kernel(const double *__restrict__ t, i64 N, T *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i < N) out[i] = (T)t[i];
}

// cpart[j][blockIdx.x] = this workgroup's share of p_j^T w; grid = (PB slices of K, earlier components j)
constexpr int MISS_PW_SLICES = 32;
__global__ __launch_bounds__(WG) void miss_pw_kernel(const double *__restrict__ P, const double *__restrict__ w, int K,
                                                     double *__restrict__ cpart) {
    __shared__ double smem[WG / WAVE];
    const double *p = P + (i64)blockIdx.y * K;
    double s = 0.0;
#pragma unroll 4
    for (i64 k = (i64)blockIdx.x * WG + threadIdx.x; k < K; k += (i64)gridDim.x * WG) s = fma(p[k], w[k], s);
    s = block_sum<WG / WAVE>(s, smem);
    if (threadIdx.x == 0) cpart[(i64)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// r_a = w_a - sum_{j < a} r_j c[j], c[j] = the PB slices of cpart[j] added in order (by every workgroup, WG components at a time)
__global__ __launch_bounds__(WG) void miss_r_kernel(const double *__restrict__ w, const double *__restrict__ R,
                                                    const double *__restrict__ cpart, int PB, int a, int K, double *__restrict__ r) {
    __shared__ double cs[WG];
    const i64 k = (i64)blockIdx.x * WG + threadIdx.x;
    double s = k < K ? w[k] : 0.0;
    for (int j0 = 0; j0 < a; j0 += WG) {
        const int jn = a - j0 < WG ? a - j0 : WG;
        if ((int)threadIdx.x < jn) {
            double c = 0.0;
            for (int b = 0; b < PB; ++b) c += cpart[(i64)(j0 + threadIdx.x) * PB + b];
            cs[threadIdx.x] = c;
        }
        __syncthreads();
        if (k < K)
            for (int j = 0; j < jn; ++j) s = fma(-R[k + (i64)(j0 + j) * K], cs[j], s);
        __syncthreads();
    }
    if (k < K) r[k] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Column statistics over the observed cells, one sweep: every lane keeps (n, sum, sum of squares) of x - c with c its own first
// observed value, turns them into (n, c, dm, M2) with mean = c + dm, and the partials are merged pairwise in a fixed order (Chan
// et al.): lanes in LDS, then the G row groups in miss_colmoments_finish_kernel.  The mean stays split into its anchor c (an
// observed value) and the small part dm until the very end: the difference of two partial means is then formed from differences
// of data values and of small parts, not of two means rounded at eps |mean| -- on a column of 1e4 +- 1 that rounding alone costs
// M2 four digits.  grid = (K, G).
// ------------------------------------------------------------------------------------------------------------------------------
struct MissMoments {
    double n, c, dm, m2;
};
__device__ __forceinline__ MissMoments miss_merge(const MissMoments &a, const MissMoments &b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = ((b.c - a.c) + b.dm) - a.dm;
    return {n, a.c, a.dm + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

template <typename T>
__global__ __launch_bounds__(WG) void miss_colmoments_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, double *__restrict__ part) {
    __shared__ MissMoments sm[WG];
    const T *col = X + (i64)blockIdx.x * ldx;
    double c = 0.0, n = 0.0, s1 = 0.0, s2 = 0.0;
    for (i64 i = (i64)blockIdx.y * WG + threadIdx.x; i < N; i += (i64)gridDim.y * WG) {
        const double x = (double)col[i];
        if (x == x) {
            if (n == 0.0) c = x;
            const double d = x - c;
            n += 1.0;
            s1 += d;
            s2 = fma(d, d, s2);
        }
    }
    MissMoments m = {0.0, 0.0, 0.0, 0.0};
    if (n > 0.0) m = {n, c, s1 / n, fmax(s2 - s1 * (s1 / n), 0.0)};
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int h = WG / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = miss_merge(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *o = part + ((i64)blockIdx.y * K + blockIdx.x) * 4;
        o[0] = sm[0].n;
        o[1] = sm[0].c;
        o[2] = sm[0].dm;
        o[3] = sm[0].m2;
    }
}

// mean, sd = sqrt(M2 / (nobs - 1)), nobs per column; fewer than two observed cells: sd = NaN (no observed cell: mean = NaN too)
__global__ __launch_bounds__(WG) void miss_colmoments_finish_kernel(const double *__restrict__ part, int G, int K, double *__restrict__ mean,
                                                                    double *__restrict__ sd, long long *__restrict__ nobs) {
    const i64 k = (i64)blockIdx.x * WG + threadIdx.x;
    if (k >= K) return;
    MissMoments m = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g) {
        const double *o = part + ((i64)g * K + k) * 4;
        m = miss_merge(m, MissMoments{o[0], o[1], o[2], o[3]});
    }
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    mean[k] = m.n > 0.0 ? m.c + m.dm : nan;
    sd[k] = m.n > 1.0 ? sqrt(m.m2 / (m.n - 1.0)) : nan;
    if (nobs) nobs[k] = (long long)m.n;
}

// Z = (X - mean) / sd, NaN kept (Z == X: in place).  grid = (K, row groups)
template <typename T>
__global__ __launch_bounds__(WG) void miss_zscale_kernel(const T *X, i64 ldx, T *Z, i64 ldz, i64 N, const double *__restrict__ mean,
                                                         const double *__restrict__ sd) {
    const double mu = mean[blockIdx.x], s = sd[blockIdx.x];
    const T *xc = X + (i64)blockIdx.x * ldx;
    T *zc = Z + (i64)blockIdx.x * ldz;
    for (i64 i = (i64)blockIdx.y * WG + threadIdx.x; i < N; i += (i64)gridDim.y * WG) zc[i] = (T)(((double)xc[i] - mu) / s);
}

}  // namespace plsk
