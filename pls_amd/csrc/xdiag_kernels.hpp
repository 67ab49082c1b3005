// xdiag_kernels.hpp -- X-space diagnostics of a fitted model (pls_hip_x_diagnostics): Q residuals, Hotelling T^2, R^2 X.
//   xdiag_scores_kernel        S = X R in fp64 for fp32 storage (fp64 storage takes launch_xb)
//   xdiag_sweep_kernel         F_c = X - S[:, :c] P[:, :c]^T formed explicitly, row sums of squares for every c of a range
//   xdiag_transpose_kernel     R^T, P^T (zero-padded to whole ranges) for the scalar loads of the two kernels above
//   xdiag_split_finish_kernel  adds the column blocks of the sweep of a short, wide matrix in index order
//   xdiag_score_stats_kernel   column sums of squares of the scores (sst), fp32 copy of the scores
//   xdiag_finish_kernel        slices -> ssx, sst, tvar = sst / (n_total - 1)
//   xdiag_t2_kernel            T2[i, c-1] = sum_{a<c} S[i,a]^2 / tvar[a]
// Lanes run across rows (column-major X: a wave reads a contiguous column piece), a row's scores and running sums stay in
// registers, R / P are uniform over the wave and come through the scalar cache.  Every sum has a fixed order.
#pragma once
#include "common.hpp"

namespace plsk {

// VEC consecutive rows of column k for the lane that owns rows i0 .. i0+VEC-1; rows beyond N read as 0
template <typename T, int VEC>
__device__ __forceinline__ void xd_load(const T *__restrict__ col, i64 i0, i64 N, bool full, double (&x)[VEC]) {
    if (full) {
        const Pack<T, VEC> p = ld_pack_nt<T, VEC>(col + i0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v] = (double)p.v[v];
    } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v] = (i0 + v < N) ? (double)col[i0 + v] : 0.0;
    }
}

// Sd[i, c] = sum_k X[i,k] R[k,c] for c_lo <= c < c_hi (at most CR of them), fp64 whatever the storage type of X.  RT = R^T, AP x K, zero rows
// behind the A-th up to a multiple of the longest range: the loop reads CR of them without a test.
// grid = ceil(N / (WG * VEC)).
template <typename T, int VEC, int CR>
__global__ __launch_bounds__(WG) void xdiag_scores_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K,
                                                          const double *__restrict__ RT, int AP, int c_lo, int c_hi,
                                                          double *__restrict__ Sd, i64 ldsd) {
    const i64 i0 = ((i64)blockIdx.x * WG + threadIdx.x) * VEC;
    const bool full = i0 + VEC <= N;
    const int nc = c_hi - c_lo;
    double acc[CR][VEC];
#pragma unroll
    for (int c = 0; c < CR; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[c][v] = 0.0;
    for (int k = 0; k < K; ++k) {
        double x[VEC];
        xd_load<T, VEC>(X + (i64)k * ldx, i0, N, full, x);
#pragma unroll
        for (int c = 0; c < CR; ++c) {  // (no test on c: the padding of RT holds zeros)
            const double r = RT[c_lo + c + (i64)k * AP];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[c][v] = fma(x[v], r, acc[c][v]);
        }
    }
#pragma unroll
    for (int c = 0; c < CR; ++c) {
        if (c < nc) {
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                if (i0 + v < N) Sd[i0 + v + (i64)(c_lo + c) * ldsd] = acc[c][v];
        }
    }
}

// NB columns of the sweep: x -= s_c P[k, c] component by component, q_c += x^2 after component c.  PT = P^T (AP x K,
// zero rows behind the A-th): the loadings of one column are contiguous, a range of them is a few wide scalar loads.
// Components below c_lo are applied from the scores in memory and not recorded.
template <typename T, int VEC, int CR, int NB>
__device__ __forceinline__ void xd_step(const T *__restrict__ X, i64 ldx, i64 N, int AP, int k, i64 i0, bool full,
                                        const double *__restrict__ Sd, i64 ldsd, const double *__restrict__ PT, int c_lo,
                                        const double (&s)[CR][VEC], double (&q)[CR][VEC], double (&qx)[VEC]) {
    double x[NB][VEC];
#pragma unroll
    for (int b = 0; b < NB; ++b) xd_load<T, VEC>(X + (i64)(k + b) * ldx, i0, N, full, x[b]);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int v = 0; v < VEC; ++v) qx[v] = fma(x[b][v], x[b][v], qx[v]);
    for (int c = 0; c < c_lo; ++c) {
        double sv[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) sv[v] = (i0 + v < N) ? Sd[i0 + v + (i64)c * ldsd] : 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const double p = PT[c + (i64)(k + b) * AP];
#pragma unroll
            for (int v = 0; v < VEC; ++v) x[b][v] = fma(-sv[v], p, x[b][v]);
        }
    }
#pragma unroll
    for (int c = 0; c < CR; ++c) {  // (no test on c: beyond the range the scores in s and the padding of PT hold zeros)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const double p = PT[c_lo + c + (i64)(k + b) * AP];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                x[b][v] = fma(-s[c][v], p, x[b][v]);
                q[c][v] = fma(x[b][v], x[b][v], q[c][v]);
            }
        }
    }
}

// The residual sweep for the component counts c_lo+1 .. c_hi (at most CR) over the columns [blockIdx.y * kper, + kper) of X.
//   xout[blockIdx.y * slice + i]                   = sum_k X[i,k]^2 of the column block        (xout may be null)
//   qout[blockIdx.y * slice + i + (c - c_lo) * ldq] = sum_k F_{c+1}[i,k]^2 of the column block  (qout may be null)
//   part[blockIdx.x * L + j], L = nc + first: the workgroup's sums over its rows, j = 0 the squares of X when `first`, then
//   the component counts of the range (part may be null; only with one column block).
// grid = (ceil(N / (WG * VEC)), column blocks).
template <typename T, int VEC, int CR>
__global__ __launch_bounds__(WG) void xdiag_sweep_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, int kper,
                                                         const double *__restrict__ Sd, i64 ldsd,
                                                         const double *__restrict__ PT, int AP, int c_lo, int c_hi,
                                                         double *__restrict__ xout, double *__restrict__ qout, i64 ldq,
                                                         i64 slice, int first, double *__restrict__ part) {
    constexpr int NB = (CR > 8 ? 4 : 8) / VEC;  // columns in flight per lane; fewer where the range's P values fill the scalar registers
    __shared__ double sm[WG / WAVE][CR + 1];
    const i64 i0 = ((i64)blockIdx.x * WG + threadIdx.x) * VEC;
    const bool full = i0 + VEC <= N;
    const int nc = c_hi - c_lo;
    const int k0 = blockIdx.y * kper, k1 = min(K, k0 + kper);
    double s[CR][VEC], q[CR][VEC], qx[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) qx[v] = 0.0;
#pragma unroll
    for (int c = 0; c < CR; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            q[c][v] = 0.0;
            s[c][v] = (c < nc && i0 + v < N) ? Sd[i0 + v + (i64)(c_lo + c) * ldsd] : 0.0;
        }
    int k = k0;
    for (; k + NB <= k1; k += NB) xd_step<T, VEC, CR, NB>(X, ldx, N, AP, k, i0, full, Sd, ldsd, PT, c_lo, s, q, qx);
    for (; k < k1; ++k) xd_step<T, VEC, CR, 1>(X, ldx, N, AP, k, i0, full, Sd, ldsd, PT, c_lo, s, q, qx);

    const i64 base = (i64)blockIdx.y * slice;
    if (xout) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
            if (i0 + v < N) xout[base + i0 + v] = qx[v];
    }
    if (qout) {
#pragma unroll
        for (int c = 0; c < CR; ++c) {
            if (c < nc) {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (i0 + v < N) qout[base + i0 + v + (i64)c * ldq] = q[c][v];
            }
        }
    }
    if (part) {  // (rows beyond N hold zeros)
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        double t = qx[0];
#pragma unroll
        for (int v = 1; v < VEC; ++v) t += qx[v];
        t = wave_sum(t);
        if (lane == 0) sm[wv][0] = t;
#pragma unroll
        for (int c = 0; c < CR; ++c) {
            if (c < nc) {
                double u = q[c][0];
#pragma unroll
                for (int v = 1; v < VEC; ++v) u += q[c][v];
                u = wave_sum(u);
                if (lane == 0) sm[wv][c + 1] = u;
            }
        }
        __syncthreads();
        const int L = nc + (first ? 1 : 0);
        if ((int)threadIdx.x < L) {
            const int j = threadIdx.x + (first ? 0 : 1);
            double u = 0.0;
#pragma unroll
            for (int w = 0; w < WG / WAVE; ++w) u += sm[w][j];
            part[(i64)blockIdx.x * L + threadIdx.x] = u;
        }
    }
}

// MT (AP x K, AP >= A) = M^T of M (K x A, ld K), rows A .. AP-1 zero: the layout the scalar loads of the kernels above want
__global__ __launch_bounds__(WG) void xdiag_transpose_kernel(const double *__restrict__ M, int K, int A, int AP,
                                                             double *__restrict__ MT) {
    const i64 j = (i64)blockIdx.x * WG + threadIdx.x;
    if (j >= (i64)K * AP) return;
    const int c = (int)(j % AP);
    const i64 k = j / AP;
    MT[j] = c < A ? M[k + (i64)c * K] : 0.0;
}

// Column-split sweep: ws[ks][j][i] (j = 0 squares of X, j = 1 + c - c_lo the component counts; ld N) -> the sums over the
// KS column blocks in index order.  Qout[i + (c - c_lo) * ldq] (may be null) and the workgroup's sums over its rows,
// part[blockIdx.x * L + ...] as the sweep writes them (may be null).  One thread per row, dynamic LDS (WG/WAVE) * (nc+1) doubles.
__global__ __launch_bounds__(WG) void xdiag_split_finish_kernel(const double *__restrict__ ws, i64 N, int nc, int KS, int first,
                                                                double *__restrict__ Qout, i64 ldq,
                                                                double *__restrict__ part) {
    extern __shared__ double xd_sm[];  // [WG/WAVE][nc + 1]
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L1 = nc + 1;
    for (int j = 0; j < L1; ++j) {
        double t = 0.0;
        if (i < N)
            for (int ks = 0; ks < KS; ++ks) t += ws[((i64)ks * L1 + j) * N + i];
        if (j > 0 && Qout && i < N) Qout[i + (i64)(j - 1) * ldq] = t;
        if (part) {
            const double u = wave_sum(t);
            if (lane == 0) xd_sm[wv * L1 + j] = u;
        }
    }
    if (part) {
        __syncthreads();
        const int L = nc + (first ? 1 : 0);
        for (int jj = threadIdx.x; jj < L; jj += WG) {
            const int j = jj + (first ? 0 : 1);
            double u = 0.0;
#pragma unroll
            for (int w = 0; w < WG / WAVE; ++w) u += xd_sm[w * L1 + j];
            part[(i64)blockIdx.x * L + jj] = u;
        }
    }
}

// part[g][c - c_lo] = sum over the group's rows of Sd[i, c]^2 (SQUARE; else of Sd[i, c]: the Q columns of
// pls_hip_x_diagnostics_missing) (may be null); Sout (fp32 storage, may be null) = the scores rounded.  One thread per row,
// grid-stride; dynamic LDS (WG/WAVE) * (c_hi - c_lo) doubles.  The layout reduce_partials_kernel sums.
template <bool SQUARE>
__global__ __launch_bounds__(WG) void xdiag_score_stats_kernel(const double *__restrict__ Sd, i64 ldsd, i64 N, int c_lo,
                                                               int c_hi, float *__restrict__ Sout, i64 ldso,
                                                               double *__restrict__ part) {
    extern __shared__ double xd_sm[];  // [WG/WAVE][nc]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nc = c_hi - c_lo;
    double *mine = xd_sm + (i64)wv * nc;
    for (int j = lane; j < nc; j += WAVE) mine[j] = 0.0;
    for (i64 b0 = (i64)blockIdx.x * WG; b0 < N; b0 += (i64)gridDim.x * WG) {
        const i64 i = b0 + threadIdx.x;
        for (int c = c_lo; c < c_hi; ++c) {
            const double s = (i < N) ? Sd[i + (i64)c * ldsd] : 0.0;
            if (Sout && i < N) Sout[i + (i64)c * ldso] = (float)s;
            if (part) {
                const double tot = wave_sum(SQUARE ? s * s : s);
                if (lane == 0) mine[c - c_lo] += tot;
            }
        }
    }
    if (part) {
        __syncthreads();
        for (int j = threadIdx.x; j < nc; j += WG) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < WG / WAVE; ++w) t += xd_sm[(i64)w * nc + j];
            part[(i64)blockIdx.x * nc + j] = t;
        }
    }
}

// red: RED_SLICES slices of [ssx[0..A], sst[0..A-1]] (summed over ranks on a sharded handle); the slices are added in index order.
__global__ __launch_bounds__(WG) void xdiag_finish_kernel(const double *__restrict__ red, int A, double n1,
                                                          double *__restrict__ ssx, double *__restrict__ sst,
                                                          double *__restrict__ tvar) {
    const i64 LP = 2 * (i64)A + 1;
    const i64 j = (i64)blockIdx.x * WG + threadIdx.x;
    if (j >= LP) return;
    double v = 0.0;
    for (int i = 0; i < RED_SLICES; ++i) v += red[(i64)i * LP + j];
    if (j <= A) {
        if (ssx) ssx[j] = v;
    } else {
        if (sst) sst[j - A - 1] = v;
        if (tvar) tvar[j - A - 1] = v / n1;
    }
}

// T2[i, c] = sum_{a <= c} Sd[i,a]^2 / tvar[a]; one thread per row
__global__ __launch_bounds__(WG) void xdiag_t2_kernel(const double *__restrict__ Sd, i64 ldsd, i64 N, int A,
                                                      const double *__restrict__ tvar, double *__restrict__ T2, i64 ldt2) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i >= N) return;
    double t = 0.0;
    for (int c = 0; c < A; ++c) {
        const double s = Sd[i + (i64)c * ldsd];
        t += s * s / tvar[c];
        T2[i + (i64)c * ldt2] = t;
    }
}

}  // namespace plsk
