// xdiag_missing_kernels.hpp -- X-space diagnostics of rows with missing cells (pls_hip_x_diagnostics_missing;
// plan_xdiag_missing.hpp enqueues them, xdiagmiss_layout.hpp has the geometry).  NaN in X marks a missing cell.  For row i:
//   q_0 = sum_obs x_k^2;  for a = 0 .. A-1:  t_a = sum_obs x_k W[k,a] / sum_obs W[k,a]^2,  x_k <- x_k - t_a P[k,a],  q_{a+1} = sum_obs x_k^2
// The row is fp64 from the load on and never rounded to the storage type.  Both routes deflate a cell by the same chain of
// fma(-t_j, P[k,j], x), j ascending, so a cell has the same bits on either; the routes differ in how a row's sums are split.
//   xdm_resident_kernel       a workgroup holds a tile of rows in LDS across all components: X is read once, pass a deflates with
//                             t_{a-1} and accumulates q_a and the sums of t_a in the same walk; the column lanes of a row meet once
//                             per pass, in LDS, in lane order
//   xdm_stream_kernel         one read-only sweep for component a: every cell rebuilt in registers from the scores 0 .. a-1, the
//                             partial sums of t_a and q_a per K range; xdm_stream_finish_kernel adds the ranges in index order
//   xdm_colsum_kernel         per-workgroup column sums of the Q columns (ssx), the layout reduce_partials_kernel sums
// All sums fp64 and in a fixed order, no atomics; a quotient whose denominator is exactly 0 is 0 (miss_quot).  The mask test is
// x == x (no -ffast-math).  Rows beyond N are never read: the pack that straddles row N is loaded element by element.
#pragma once
#include "common.hpp"
#include "missing_kernels.hpp"  // miss_quot
#include "xdiagmiss_layout.hpp"

namespace plsk {

// V rows i .. i + V - 1 of one column as fp64; rows beyond N are 0 and never used
template <typename T, int V>
__device__ __forceinline__ void xdm_load(const T *__restrict__ col, i64 i, i64 N, double (&x)[V]) {
    if (i + V <= N) {
        const Pack<T, V> p = ld_pack_nt<T, V>(col + i);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (double)p.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (i + j < N) ? (double)col[i + j] : 0.0;
    }
}

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
            const bool ob = x[u] == x[u];
            q = ob ? fma(x[u], x[u], q) : q;
            if (!LAST) {
                num = ob ? fma(x[u], w[u], num) : num;
                den = ob ? fma(w[u], w[u], den) : den;
            }
            if (FIRST) cnt += ob ? 1 : 0;
        }
    }
    for (; k < K; k += CL, cell += step) {
        double x = *cell;
        if (!FIRST) {
            x = fma(-tprev, pp[k], x);
            if (!LAST) *cell = x;
        }
        const bool ob = x == x;
        q = ob ? fma(x, x, q) : q;
        if (!LAST) {
            const double w = wa[k];
            num = ob ? fma(x, w, num) : num;
            den = ob ? fma(w, w, den) : den;
        }
        if (FIRST) cnt += ob ? 1 : 0;
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
            for (int u = 0; u < U; ++u) xdm_load<T, V>(col + u * cstep, i, N, x[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) dst[(i64)u * CV * RT + j] = x[u][j];
        }
        for (; k < K; k += CV, col += cstep, dst += (i64)CV * RT) {
            double x[V];
            xdm_load<T, V>(col, i, N, x);
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
// Streaming route, the sweep for component a (a == A: the last one, q_A only; W is not read).  grid = (row blocks, K ranges) in the
// geometry of miss_row_kernel: lane (r, c) owns the V rows (blockIdx.x RL + r) V ... and walks the columns kb + c, kb + c + CL, ...
// of the range blockIdx.y; the column lanes meet in LDS in the order of c.  Sd (N x A, ld ldsd) holds the scores 0 .. a-1.
// part[blockIdx.y][i] = {num, den, q, observed cells}.
// ------------------------------------------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(WG) void xdm_stream_kernel(const T *__restrict__ X, i64 ldx, i64 N, int K, int a, int last,
                                                        const double *__restrict__ wa, const double *__restrict__ P,
                                                        const double *__restrict__ Sd, i64 ldsd, int lrl, int kper,
                                                        double *__restrict__ part) {
    __shared__ double sm[WG][XDM_PART * V];
    const int RL = 1 << lrl, CL = WG >> lrl;
    const int r = threadIdx.x & (RL - 1), c = threadIdx.x >> lrl;
    const i64 i0 = ((i64)blockIdx.x * RL + r) * V;
    const i64 kb = (i64)blockIdx.y * kper;
    const i64 ke = kb + kper < K ? kb + kper : K;
    double an[V], ad[V], aq[V], ac[V];
#pragma unroll
    for (int j = 0; j < V; ++j) an[j] = ad[j] = aq[j] = ac[j] = 0.0;
    if (i0 < N) {
        constexpr int U = 4;  // columns in flight per lane
        i64 k = kb + c;
        for (; k + (i64)(U - 1) * CL < ke; k += (i64)U * CL) {
            double x[U][V], wk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xdm_load<T, V>(X + (k + (i64)u * CL) * ldx, i0, N, x[u]);
                wk[u] = last ? 0.0 : wa[k + (i64)u * CL];
            }
            // x <- x - t_j P[k,j], j ascending; the loads of JU components are issued together (they do not depend on x)
            constexpr int JU = V == 4 ? 2 : 4;
            int j = 0;
            for (; j + JU <= a; j += JU) {
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
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double xd = x[u][v];
                    const bool ob = xd == xd;
                    an[v] = ob ? fma(xd, wk[u], an[v]) : an[v];
                    ad[v] = ob ? fma(wk[u], wk[u], ad[v]) : ad[v];
                    aq[v] = ob ? fma(xd, xd, aq[v]) : aq[v];
                    ac[v] = ob ? ac[v] + 1.0 : ac[v];
                }
        }
        for (; k < ke; k += CL) {
            double x[V];
            xdm_load<T, V>(X + k * ldx, i0, N, x);
            const double wk = last ? 0.0 : wa[k];
            for (int j = 0; j < a; ++j) {
                const double pj = P[k + (i64)j * K];
#pragma unroll
                for (int v = 0; v < V; ++v) x[v] = fma(-((i0 + v < N) ? Sd[i0 + v + (i64)j * ldsd] : 0.0), pj, x[v]);
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double xd = x[v];
                const bool ob = xd == xd;
                an[v] = ob ? fma(xd, wk, an[v]) : an[v];
                ad[v] = ob ? fma(wk, wk, ad[v]) : ad[v];
                aq[v] = ob ? fma(xd, xd, aq[v]) : aq[v];
                ac[v] = ob ? ac[v] + 1.0 : ac[v];
            }
        }
    }
    if (CL > 1) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sm[threadIdx.x][XDM_PART * v] = an[v];
            sm[threadIdx.x][XDM_PART * v + 1] = ad[v];
            sm[threadIdx.x][XDM_PART * v + 2] = aq[v];
            sm[threadIdx.x][XDM_PART * v + 3] = ac[v];
        }
        __syncthreads();
        if (c == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                double sn = 0.0, sd = 0.0, sq = 0.0, sc = 0.0;
                for (int cc = 0; cc < CL; ++cc) {
                    sn += sm[r + cc * RL][XDM_PART * v];
                    sd += sm[r + cc * RL][XDM_PART * v + 1];
                    sq += sm[r + cc * RL][XDM_PART * v + 2];
                    sc += sm[r + cc * RL][XDM_PART * v + 3];
                }
                an[v] = sn;
                ad[v] = sd;
                aq[v] = sq;
                ac[v] = sc;
            }
        }
    }
    if (c != 0) return;
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (i0 + v < N) {
            double *o = part + ((i64)blockIdx.y * N + i0 + v) * XDM_PART;
            st_pack<double, 2>(o, Pack<double, 2>{{an[v], ad[v]}});
            st_pack<double, 2>(o + 2, Pack<double, 2>{{aq[v], ac[v]}});
        }
}

// The S ranges of a row: t (null: the last sweep) = num / den, q (may be null), nobs (may be null).  A workgroup owns XDM_RF_ROWS
// rows; range lane sl adds the ranges sl, sl + SL, ... in order (SL = WG / XDM_RF_ROWS), then the SL lanes of a row meet in LDS in
// the order of sl -- the shape of miss_row_finish_kernel: one dependent chain of S loads per row cost more than the sweep.
constexpr int XDM_RF_ROWS = 16;
__global__ __launch_bounds__(WG) void xdm_stream_finish_kernel(const double *__restrict__ part, int S, i64 N, double *__restrict__ t,
                                                               double *__restrict__ q, long long *__restrict__ nobs) {
    constexpr int RR = XDM_RF_ROWS, SL = WG / RR;
    __shared__ double sm[SL][RR][XDM_PART];
    const int ri = threadIdx.x % RR, sl = threadIdx.x / RR;
    const i64 i = (i64)blockIdx.x * RR + ri;
    double num = 0.0, den = 0.0, sq = 0.0, cnt = 0.0;
    if (i < N) {
#pragma unroll 4
        for (int s = sl; s < S; s += SL) {
            const double *p = part + ((i64)s * N + i) * XDM_PART;
            const Pack<double, 2> u = ld_pack<double, 2>(p), v = ld_pack<double, 2>(p + 2);
            num += u.v[0];
            den += u.v[1];
            sq += v.v[0];
            cnt += v.v[1];
        }
    }
    sm[sl][ri][0] = num;
    sm[sl][ri][1] = den;
    sm[sl][ri][2] = sq;
    sm[sl][ri][3] = cnt;
    __syncthreads();
    if (sl != 0 || i >= N) return;
    num = den = sq = cnt = 0.0;
#pragma unroll
    for (int j = 0; j < SL; ++j) {
        num += sm[j][ri][0];
        den += sm[j][ri][1];
        sq += sm[j][ri][2];
        cnt += sm[j][ri][3];
    }
    if (t) t[i] = miss_quot(num, den);
    if (q) q[i] = sq;
    if (nobs) nobs[i] = (long long)cnt;
}

// part[g][j] = sum over the group's rows of src[i, j], j < nc (ld in elements).  One thread per row, grid-stride; dynamic LDS
// (WG / WAVE) * nc doubles.  The layout reduce_partials_kernel sums.
__global__ __launch_bounds__(WG) void xdm_colsum_kernel(const double *__restrict__ src, i64 ld, i64 N, int nc,
                                                        double *__restrict__ part) {
    extern __shared__ double xdm_sm[];  // [WG / WAVE][nc]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *mine = xdm_sm + (i64)wv * nc;
    for (int j = lane; j < nc; j += WAVE) mine[j] = 0.0;
    for (i64 b0 = (i64)blockIdx.x * WG; b0 < N; b0 += (i64)gridDim.x * WG) {
        const i64 i = b0 + threadIdx.x;
        for (int j = 0; j < nc; ++j) {
            const double tot = wave_sum((i < N) ? src[i + (i64)j * ld] : 0.0);
            if (lane == 0) mine[j] += tot;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nc; j += WG) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < WG / WAVE; ++w) t += xdm_sm[(i64)w * nc + j];
        part[(i64)blockIdx.x * nc + j] = t;
    }
}

}  // namespace plsk
