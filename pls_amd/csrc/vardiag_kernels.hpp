// vardiag_kernels.hpp -- variable-space diagnostics of a fitted model (pls_hip_var_diagnostics): per-variable residual sums of
// squares for every component count, VIP.
//   vardiag_rows_kernel      the fp64 scores, row-contiguous and zero-padded (whole tiles of rows, components to a multiple of 4)
//   vardiag_sweep_kernel     F_c = X - S[:, :c] P[:, :c]^T formed explicitly, COLUMN sums of squares for every c of a range
//   vardiag_finish_kernel    the slices of the message -> sst, ssxk
//   vardiag_vip_prep_kernel  ||w_a||^2 and ssy_a = tau_a sum_m Q[m,a]^2
//   vardiag_vip_kernel       VIP[k, c-1]
// The sweep is the column-wise twin of xdiag_sweep_kernel: lanes run across 64 COLUMNS, so a column's loadings and running sums
// stay in the lane's registers and nothing crosses lanes; a row's scores are uniform over the wave and come through the scalar
// cache from the row-contiguous copy.  X is column-major, so a workgroup stages a tile (VD_TR rows x 64 columns, contiguous
// column pieces) into LDS and reads it back transposed; the next tile is on its way to registers meanwhile.  Every sum has a
// fixed order.  The geometry is vardiag_layout.hpp's.
#pragma once
#include "common.hpp"
#include "vardiag_layout.hpp"

namespace plsk {

static_assert(VD_THREADS == WG && VD_TC == WAVE && VD_RED_SLICES == RED_SLICES, "vardiag_layout.hpp restates these");
static_assert((WG / WAVE) * (VD_RANGE + 1) * WAVE * 8 <= VD_TILE_BYTES, "the waves' sums are combined in the tile's LDS");

// ST[i * AS + c] = Sd[i + c * ldsd] for i < N, c < A; zero for N <= i < rows and A <= c < AS (AS % 4 == 0).  One thread per row.
__global__ __launch_bounds__(WG) void vardiag_rows_kernel(const double *__restrict__ Sd, i64 ldsd, i64 N, int A, int AS, i64 rows,
                                                          double *__restrict__ ST) {
    const i64 i = (i64)blockIdx.x * WG + threadIdx.x;
    if (i >= rows) return;
    for (int c0 = 0; c0 < AS; c0 += 4) {
        Pack<double, 2> a, b;
        a.v[0] = (i < N && c0 + 0 < A) ? Sd[i + (i64)(c0 + 0) * ldsd] : 0.0;
        a.v[1] = (i < N && c0 + 1 < A) ? Sd[i + (i64)(c0 + 1) * ldsd] : 0.0;
        b.v[0] = (i < N && c0 + 2 < A) ? Sd[i + (i64)(c0 + 2) * ldsd] : 0.0;
        b.v[1] = (i < N && c0 + 3 < A) ? Sd[i + (i64)(c0 + 3) * ldsd] : 0.0;
        st_pack<double, 2>(ST + i * AS + c0, a);
        st_pack<double, 2>(ST + i * AS + c0 + 2, b);
    }
}

// The tile of rows i0 .. i0 + VD_TR - 1, columns k0 .. k0 + 63 into registers: vector e = it * WG + tid is VEC consecutive rows
// of one column, a wave's vectors are contiguous in memory.  Rows beyond N and columns beyond K read as 0.
template <typename T, int VEC>
__device__ __forceinline__ void vd_fetch(const T *__restrict__ X, i64 ldx, i64 N, i64 K, i64 i0, i64 k0, int tid,
                                         Pack<T, VEC> (&pre)[VD_TR * VD_TC / (WG * VEC)]) {
    constexpr int NV = VD_TR * VD_TC / (WG * VEC), G = VD_TR / VEC;
    const bool full = i0 + VD_TR <= N && k0 + VD_TC <= K;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
        const int e = it * WG + tid;
        const i64 col = k0 + e / G, row = i0 + (i64)(e % G) * VEC;
        if (full) {
            pre[it] = ld_pack_nt<T, VEC>(X + col * ldx + row);
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) pre[it].v[v] = (col < K && row + v < N) ? X[col * ldx + row + v] : (T)0;
        }
    }
}

// ... and from the registers into LDS as fp64, column c at c * VD_LDC
template <typename T, int VEC>
__device__ __forceinline__ void vd_store(double *tile, int tid, const Pack<T, VEC> (&pre)[VD_TR * VD_TC / (WG * VEC)]) {
    constexpr int NV = VD_TR * VD_TC / (WG * VEC), G = VD_TR / VEC;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
        const int e = it * WG + tid;
        double *dst = tile + (e / G) * VD_LDC + (e % G) * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) dst[v] = (double)pre[it].v[v];
    }
}

// The column sweep for the component counts c_lo+1 .. c_hi (at most CR) of column block blockIdx.x / RS over the row tiles of row
// split blockIdx.x % RS (vardiag_layout.hpp).  P is K x A, ld K: lanes read consecutive addresses.  ST: vardiag_rows_kernel's.
//   part[rs * p_rs + j * p_j + k], j < L = nc + first: the split's sums for column k, j = 0 the squares of X when
//   `first` (c_lo == 0), then the component counts of the range.
// Components below c_lo are applied from the scores to the tile in LDS, every lane to its own column, and not recorded.
// grid = column blocks x row splits, one dimension; dynamic LDS VD_TILE_BYTES.
template <typename T, int VEC, int CR>
__global__ __launch_bounds__(WG) void vardiag_sweep_kernel(const T *__restrict__ X, i64 ldx, i64 N, i64 K, i64 NT, int RS,
                                                           const double *__restrict__ ST, int AS, const double *__restrict__ P,
                                                           int c_lo, int c_hi, double *__restrict__ part, i64 p_rs, i64 p_j) {
    extern __shared__ double vd_tile[];  // [VD_TC][VD_LDC]; at the end [WG / WAVE][CR + 1][WAVE]
    constexpr int NV = VD_TR * VD_TC / (WG * VEC), RW = VD_TR / (WG / WAVE);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup id = rs + RS * cb: consecutive ids go to different XCDs, so the column blocks that read the same rows of ST share an L2
    const int rs = (int)(blockIdx.x % (unsigned)RS), nc = c_hi - c_lo, first = c_lo == 0 ? 1 : 0;
    const i64 k0 = (i64)(blockIdx.x / (unsigned)RS) * VD_TC, k = k0 + lane;
    const bool kin = k < K;
    const i64 t0 = NT * rs / RS, t1 = NT * (rs + 1) / RS;
    double p[CR], q[CR], qx = 0.0;
#pragma unroll
    for (int c = 0; c < CR; ++c) {
        p[c] = (c < nc && kin) ? P[k + (i64)(c_lo + c) * K] : 0.0;
        q[c] = 0.0;
    }
    double *xcol = vd_tile + lane * VD_LDC + wv * RW;  // this lane's column, this wave's rows
    Pack<T, VEC> pre[NV];
    vd_fetch<T, VEC>(X, ldx, N, K, t0 * VD_TR, k0, tid, pre);
    for (i64 t = t0; t < t1; ++t) {
        lds_barrier();  // (the waves are done with the tile before)
        vd_store<T, VEC>(vd_tile, tid, pre);
        lds_barrier();
        float warm0 = 0.f, warm1 = 0.f;
        if (t + 1 < t1) {
            vd_fetch<T, VEC>(X, ldx, N, K, (t + 1) * VD_TR, k0, tid, pre);
            // the next tile's scores of this wave's rows on their way into L2 (two lanes per row, a word of every 64 bytes of the
            // range): the scalar loads below then miss their cache as far as L2, not as far as memory
            const int last = (AS - c_lo) * 8 - 4;
            const char *row = (const char *)(ST + ((t + 1) * VD_TR + wv * RW + (lane >> 1)) * AS + c_lo);
            warm0 = *(const float *)(row + min((lane & 1) * 128, last));
            warm1 = *(const float *)(row + min((lane & 1) * 128 + 64, last));
        }
        const double *srow = ST + (t * VD_TR + wv * RW) * AS;  // uniform over the wave: scalar loads
        for (int cb = 0; cb < c_lo; cb += 8) {  // (c_lo is a multiple of VD_RANGE, VD_RANGE of 8)
            double pl[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pl[j] = kin ? P[k + (i64)(cb + j) * K] : 0.0;
            for (int r = 0; r < RW; ++r) {
                double x = xcol[r];
#pragma unroll
                for (int j = 0; j < 8; ++j) x = fma(-srow[(i64)r * AS + cb + j], pl[j], x);
                xcol[r] = x;
            }
        }
        const double *s = srow + c_lo;
#pragma unroll 2
        for (int r = 0; r < RW; ++r, s += AS) {
            double x = xcol[r];
            qx = fma(x, x, qx);
#pragma unroll
            for (int c = 0; c < CR; ++c) {  // (no test on c: beyond the range the loadings in p and the padding of ST hold zeros)
                x = fma(-s[c], p[c], x);
                q[c] = fma(x, x, q[c]);
            }
        }
        asm volatile("" ::"v"(warm0), "v"(warm1));  // (the loads are kept; they have long landed)
    }
    // the four waves' sums in wave order
    lds_barrier();
    vd_tile[(wv * (CR + 1)) * WAVE + lane] = qx;
#pragma unroll
    for (int c = 0; c < CR; ++c) vd_tile[(wv * (CR + 1) + 1 + c) * WAVE + lane] = q[c];
    lds_barrier();
    for (int j = wv + 1 - first; j <= nc; j += WG / WAVE) {
        double u = 0.0;
#pragma unroll
        for (int w = 0; w < WG / WAVE; ++w) u += vd_tile[(w * (CR + 1) + j) * WAVE + lane];
        if (kin) part[(i64)rs * p_rs + (i64)(j - 1 + first) * p_j + k] = u;
    }
}

// red: RED_SLICES slices of [sst (A) | ssxk (K x (A + 1), ld K)] (summed over ranks on a sharded handle; without the second part
// when L == A), added in index order.  sst, ssxk may be null.
__global__ __launch_bounds__(WG) void vardiag_finish_kernel(const double *__restrict__ red, i64 L, int A, i64 K,
                                                            double *__restrict__ sst, double *__restrict__ ssxk, i64 ldk) {
    const i64 j = (i64)blockIdx.x * WG + threadIdx.x;
    if (j >= L) return;
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < RED_SLICES; ++i) v += red[(i64)i * L + j];
    if (j < A) {
        if (sst) sst[j] = v;
    } else if (ssxk) {
        const i64 jj = j - A;
        ssxk[jj % K + (jj / K) * ldk] = v;
    }
}

// One workgroup per component a: out[a] = ||w_a||^2, out[A + a] = ssy_a = tau[a] * sum_m Q[m,a]^2.  W is K x A (ld K), Q is M x A (ld M).
__global__ __launch_bounds__(WG) void vardiag_vip_prep_kernel(const double *__restrict__ W, i64 K, const double *__restrict__ Q, i64 M,
                                                              const double *__restrict__ tau, int A, double *__restrict__ out) {
    __shared__ double sm[WG / WAVE];
    const int a = blockIdx.x;
    double w2 = 0.0, q2 = 0.0;
    for (i64 k = threadIdx.x; k < K; k += WG) {
        const double w = W[k + (i64)a * K];
        w2 = fma(w, w, w2);
    }
    for (i64 m = threadIdx.x; m < M; m += WG) {
        const double v = Q[m + (i64)a * M];
        q2 = fma(v, v, q2);
    }
    w2 = block_sum<WG / WAVE>(w2, sm);
    q2 = block_sum<WG / WAVE>(q2, sm);
    if (threadIdx.x == 0) {
        out[a] = w2;
        out[A + a] = tau[a] * q2;
    }
}

// VIP[k, c-1] = sqrt(K sum_{a<c} ssy_a W[k,a]^2 / ||w_a||^2 / sum_{a<c} ssy_a); one thread per variable.  pre: vardiag_vip_prep_kernel's.
__global__ __launch_bounds__(WG) void vardiag_vip_kernel(const double *__restrict__ W, i64 K, int A, const double *__restrict__ pre,
                                                         double *__restrict__ VIP, i64 ldv) {
    const i64 k = (i64)blockIdx.x * WG + threadIdx.x;
    if (k >= K) return;
    double num = 0.0, den = 0.0;
    for (int a = 0; a < A; ++a) {
        const double w = W[k + (i64)a * K], ssy = pre[A + a];
        num += ssy * (w * w / pre[a]);
        den += ssy;
        VIP[k + (i64)a * ldv] = sqrt((double)K * num / den);
    }
}

}  // namespace plsk
