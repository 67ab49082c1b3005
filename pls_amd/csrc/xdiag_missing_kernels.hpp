// xdiag_missing_kernels.hpp -- X-space diagnostics of rows with missing cells (pls_hip_x_diagnostics_missing;
// plan_xdiag_missing.hpp enqueues them, xdiagmiss_layout.hpp has the geometry).  NaN in X marks a missing cell.  For row i:
//   q_0 = sum_obs x_k^2;  for a = 0 .. A-1:  t_a = sum_obs x_k W[k,a] / sum_obs W[k,a]^2,  x_k <- x_k - t_a P[k,a],  q_{a+1} = sum_obs x_k^2
// The row is fp64 from the load on and never rounded to the storage type.  Both routes deflate a cell by the same chain of
// fma(-t_j, P[k,j], x), j ascending, so a cell has the same bits on either; the routes differ in how a row's sums are split.
//   xdm_resident_kernel       a workgroup holds a tile of rows in LDS across all components: X is read once, pass a deflates with
//                             t_{a-1} and accumulates q_a and the sums of t_a in the same walk; the column lanes of a row meet once
//                             per pass, in LDS, in lane order
//   xdm_stream_kernel         one read-only sweep for component a: every cell rebuilt in registers from the scores 0 .. a-1, the
//                             partial sums of t_a and q_a per K range; xdm_stream_finish_kernel adds the ranges in index order.
//                             Both are the row sweep of missing_kernels.hpp (miss_row_walk, miss_ranges_sum) with four sums per
//                             row; what is written here is the deflation chain (XdmCellDeflated) and the epilogues
// The column sums of the Q columns (ssx) are xdiag_score_stats_kernel<false> of xdiag_kernels.hpp.
// All sums fp64 and in a fixed order, no atomics; a quotient whose denominator is exactly 0 is 0 (miss_quot).  The mask test is
// x == x (no -ffast-math), written in miss_obs_xw / miss_obs_xx only.  Rows beyond N are never read (miss_load_rows).
#pragma once
#include "common.hpp"
#include "missing_kernels.hpp"  // miss_quot, the observed-cell steps, the row sweep
#include "xdiagmiss_layout.hpp"

namespace plsk {

// ------------------------------------------------------------------------------------------------------------------------------
// Row-resident route.  grid = tiles of RT = 1 << lrt rows; dynamic LDS = the tile [K][RT] of doubles.  Load: lane (rv, cv) brings
// V rows of the columns cv, cv + WG / (RT / V), ...  Compute: lane (r, c) owns row r and the columns c, c + CL, ... (CL = WG / RT).
// npass = A + 1 (q_A wanted) or A.  Sd (N x A, ld ldsd) is always written; q0 (N), Q (N x A, ld ldq), nobs (N) may be null.
// ------------------------------------------------------------------------------------------------------------------------------
template <bool FIRST, bool LAST>
__device__ __forceinline__ void xdm_resident_pass(double *__restrict__ tile, int RT, int CL, int r, int c, int K, double tprev,
                                                  const double *__restrict__ wa, const double *__restrict__ pp, double &num,
                                                  double &den, double &q, int &cnt) {
    constexpr int U = 4;  // LDS loads in flight per lane
    int unused = 0;       // the cells are counted in the first pass only
    const i64 step = (i64)CL * RT;
    double *cell = tile + (i64)c * RT + r;
    int k = c;
    for (; k + (U - 1) * CL < K; k += U * CL, cell += U * step) {
        double x[U], w[U], p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = cell[u * step];
            w[u] = LAST ? 0.0 : wa[k + u * CL];
            p[u] = FIRST ? 0.0 : pp[k + u * CL];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!FIRST) {
                x[u] = fma(-tprev, p[u], x[u]);
                if (!LAST) cell[u * step] = x[u];
            }
            miss_obs_xx(x[u], q, FIRST ? cnt : unused);
            if (!LAST) miss_obs_xw(x[u], w[u], num, den);
        }
    }
    for (; k < K; k += CL, cell += step) {
        double x = *cell;
        if (!FIRST) {
            x = fma(-tprev, pp[k], x);
            if (!LAST) *cell = x;
        }
        miss_obs_xx(x, q, FIRST ? cnt : unused);
        if (!LAST) miss_obs_xw(x, wa[k], num, den);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(WG) void xdm_resident_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, int A, int lrt, int npass,
                                                          const double *__restrict__ W, const double *__restrict__ P,
                                                          double *__restrict__ Sd, i64 ldsd, double *__restrict__ q0,
                                                          double *__restrict__ Q, i64 ldq, long long *__restrict__ nobs) {
    extern __shared__ __attribute__((aligned(16))) double xdm_tile[];  // [K][RT]
    __shared__ double hand[2][XDM_HAND][WG];
    __shared__ int hand_cnt[WG];
    const int tid = threadIdx.x;
    const int RT = 1 << lrt, CL = WG >> lrt;
    const i64 r0 = (i64)blockIdx.x * RT;
    {   // the one read of X
        constexpr int LV = V == 4 ? 2 : V == 2 ? 1 : 0;
        const int lrv = lrt - LV;  // log2 of the row packs of the tile
        const int rv = tid & ((1 << lrv) - 1), cv = tid >> lrv, CV = WG >> lrv;
        const i64 i = r0 + (i64)rv * V;
        const T *col = X + (i64)cv * ldx;
        const i64 cstep = (i64)CV * ldx;
        double *dst = xdm_tile + (i64)cv * RT + rv * V;
        constexpr int U = 4;  // loads in flight per lane
        int k = cv;
        for (; k + (U - 1) * CV < K; k += U * CV, col += U * cstep, dst += (i64)U * CV * RT) {
            double x[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) miss_load_rows<T, V>(col + u * cstep, i, N, i + V <= N, x[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) dst[(i64)u * CV * RT + j] = x[u][j];
        }
        for (; k < K; k += CV, col += cstep, dst += (i64)CV * RT) {
            double x[V];
            miss_load_rows<T, V>(col, i, N, i + V <= N, x);
#pragma unroll
            for (int j = 0; j < V; ++j) dst[j] = x[j];
        }
    }
    __syncthreads();
    const int r = tid & (RT - 1), c = tid >> lrt;
    const i64 i = r0 + r;
    double tprev = 0.0;
    for (int a = 0; a < npass; ++a) {
        const double *wa = W + (i64)a * K, *pp = P + (i64)(a - 1) * K;  // (neither is read where it does not exist)
        double num = 0.0, den = 0.0, q = 0.0;
        int cnt = 0;
        if (a == 0) xdm_resident_pass<true, false>(xdm_tile, RT, CL, r, c, K, 0.0, wa, nullptr, num, den, q, cnt);
        else if (a < A) xdm_resident_pass<false, false>(xdm_tile, RT, CL, r, c, K, tprev, wa, pp, num, den, q, cnt);
        else xdm_resident_pass<false, true>(xdm_tile, RT, CL, r, c, K, tprev, nullptr, pp, num, den, q, cnt);
        // the hand-over: the column lanes of a row in lane order, every lane of the row adds them itself (one barrier per pass;
        // pass a + 2 overwrites this parity only after every lane has passed the barrier of pass a + 1)
        double(*h)[WG] = hand[a & 1];
        h[0][tid] = num;
        h[1][tid] = den;
        h[2][tid] = q;
        if (a == 0) hand_cnt[tid] = cnt;
        __syncthreads();
        double sn = 0.0, sd = 0.0, sq = 0.0;
        for (int cc = 0; cc < CL; ++cc) {
            sn += h[0][cc * RT + r];
            sd += h[1][cc * RT + r];
            sq += h[2][cc * RT + r];
        }
        tprev = miss_quot(sn, sd);
        if (c == 0 && i < N) {
            if (a < A) Sd[i + (i64)a * ldsd] = tprev;
            if (a == 0) {
                if (q0) q0[i] = sq;
                if (nobs) {
                    long long n = 0;
                    for (int cc = 0; cc < CL; ++cc) n += hand_cnt[cc * RT + r];
                    nobs[i] = n;
                }
            } else if (Q) {
                Q[i + (i64)(a - 1) * ldq] = sq;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Streaming route, the sweep for component a (a == A: the last one, q_A only; W is not read).  grid = (row blocks, K ranges): the
// row sweep of missing_kernels.hpp (miss_row_walk) with four sums per row and the cell policy below.  Sd (N x A, ld ldsd) holds the
// scores 0 .. a-1.  part[blockIdx.y][i] = {num, den, q, observed cells}.
// ------------------------------------------------------------------------------------------------------------------------------
// the cell policy: x <- x - t_j P[k,j], j = 0 .. a-1 ascending; the loads of JU components are issued together (they do not
// depend on x).  wa == nullptr: the last sweep, the factor is 0.
template <int V>
struct XdmCellDeflated {
    const double *__restrict__ wa, *__restrict__ P, *__restrict__ Sd;
    i64 ldsd, N;
    int a, K;
    __device__ __forceinline__ double factor(i64 k) const { return wa ? wa[k] : 0.0; }
    template <int U>
    __device__ __forceinline__ void apply(double (&x)[U][V], i64 i0, i64 k, int CL) const {
        constexpr int JU = V == 4 ? 2 : 4;
        int j = 0;
        // (U == 1, the walk's tail: a column at a time takes the plain chain below -- the same fma per cell in the same order)
        for (; U > 1 && j + JU <= a; j += JU) {
            double tj[JU][V], pj[JU][U];
#pragma unroll
            for (int jj = 0; jj < JU; ++jj) {
#pragma unroll
                for (int v = 0; v < V; ++v) tj[jj][v] = (i0 + v < N) ? Sd[i0 + v + (i64)(j + jj) * ldsd] : 0.0;
#pragma unroll
                for (int u = 0; u < U; ++u) pj[jj][u] = P[k + (i64)u * CL + (i64)(j + jj) * K];
            }
#pragma unroll
            for (int jj = 0; jj < JU; ++jj)
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < V; ++v) x[u][v] = fma(-tj[jj][v], pj[jj][u], x[u][v]);
        }
        for (; j < a; ++j) {
            double tj[V];
#pragma unroll
            for (int v = 0; v < V; ++v) tj[v] = (i0 + v < N) ? Sd[i0 + v + (i64)j * ldsd] : 0.0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double pj = P[k + (i64)u * CL + (i64)j * K];
#pragma unroll
                for (int v = 0; v < V; ++v) x[u][v] = fma(-tj[v], pj, x[u][v]);
            }
        }
    }
};

template <typename T, int V>
__global__ __launch_bounds__(WG) void xdm_stream_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, int a, int last,
                                                        const double *__restrict__ wa, const double *__restrict__ P,
                                                        const double *__restrict__ Sd, i64 ldsd, int lrl, int kper,
                                                        double *__restrict__ part) {
    double acc[XDM_PART][V];
    i64 i0;
    const XdmCellDeflated<V> cell{last ? nullptr : wa, P, Sd, ldsd, N, a, K};
    if (!miss_row_walk<T, V, 4, XDM_PART, false>(X, ldx, N, K, lrl, kper, cell, acc, i0)) return;
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (i0 + v < N) {
            double *o = part + ((i64)blockIdx.y * N + i0 + v) * XDM_PART;
            st_pack<double, 2>(o, Pack<double, 2>{{acc[0][v], acc[1][v]}});
            st_pack<double, 2>(o + 2, Pack<double, 2>{{acc[2][v], acc[3][v]}});
        }
}

// The S ranges of a row (miss_ranges_sum): t (null: the last sweep) = num / den, q (may be null), nobs (may be null)
__global__ __launch_bounds__(WG) void xdm_stream_finish_kernel(const double *__restrict__ part, int S, i64 N, double *__restrict__ t,
                                                               double *__restrict__ q, long long *__restrict__ nobs) {
    double sum[XDM_PART];
    i64 i;
    if (!miss_ranges_sum<XDM_PART>(part, S, N, sum, i)) return;
    if (t) t[i] = miss_quot(sum[0], sum[1]);
    if (q) q[i] = sum[2];
    if (nobs) nobs[i] = (long long)sum[3];
}

}  // namespace plsk
