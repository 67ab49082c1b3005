// Many response sets against one X (pls_hip_fit_batch): every problem b is Model::plsr(X, Y_b, KERNEL_TYPE2)
// (src/pls.cpp:390-437) on the shared XX = X^T X and its own XY_b = X^T Y_b.
//
//   xtg_kernel          the wide product X^T G (G = the columns of a round's problems, hundreds to thousands of them) on
//                       v_mfma_f64_16x16x4_f64: the operand staging of an OFF-DIAGONAL block of the register-staged SYRK
//                       (syrk_kernels.hpp, syrk_kernel) with the second panel taken from G.  A workgroup = 4 waves = a
//                       128 x 128 block of the result, each wave a 64 x 64 quadrant of 4 x 4 MFMA tiles; the rows are
//                       split over gridDim.y workgroups whose partial blocks reduce_partials_kernel adds in fixed order.
//                       The same kernel with X := XX (symmetric: XX^T = XX), G := the current r of every problem and ONE
//                       row split is the component step's GEMM V = XX [r_0 r_1 ...]: no split-K, no atomics.
//   batch_step_kernel   one workgroup per problem: tt_b = r_b^T v_b, then component_update_call on [v_b, tt_b] -- p, q, the
//                       deflation of XY_b and the next w and r, the sequence cv_folds_kernel runs per fold.
//   batch_ssy / pack / finish / tt: the K- and M-sized bookkeeping around them.
// Nothing here waits on another workgroup: every hand-over is a kernel boundary.
#pragma once
#include "small_kernels.hpp"
#include "syrk_kernels.hpp"

namespace plsk {

typedef double bk_f64x4 __attribute__((ext_vector_type(4)));

// out[split][a + b * ldo] = sum over the split's rows i of X[i, a] * G[i, b]     (a < K, b < C)
// grid = (ceil(K/128) * nbc, row splits), nbc = ceil(C/128); 256 threads; dynamic LDS = SyrkCfg<T>::LDS_BYTES.
// vec != 0: X, G are 16-byte aligned with ld % V == 0 (whole V-row packs are loaded at once); 0: element by element.
template <typename T>
__global__ __launch_bounds__(256, 2) void xtg_kernel(const T *__restrict__ X, i64 ldx, const T *__restrict__ G, i64 ldg, i64 N,
                                                     int K, int C, int nbc, int vec, double *__restrict__ out, i64 ldo,
                                                     i64 pstride) {
    constexpr int V = SyrkCfg<T>::V, RB = SyrkCfg<T>::RB, LDP = SyrkCfg<T>::LDP;
    extern __shared__ __attribute__((aligned(16))) unsigned char xtg_raw[];  // As[TB][LDP], Bs[TB][LDP]
    T *As = reinterpret_cast<T *>(xtg_raw), *Bs = As + SYRK_TB * LDP;

    const int bi = blockIdx.x / nbc, bj = blockIdx.x % nbc;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int rp = tid & 15, cgi = tid >> 4;  // staging map: row group (V rows), column group; 8 columns per thread and panel
    const int a0 = (wv >> 1) * 64, b0 = (wv & 1) * 64;
    const int li = lane & 15, lq = lane >> 4;

    bk_f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = bk_f64x4{0.0, 0.0, 0.0, 0.0};

    const i64 nslabs = (N + RB - 1) / RB;
    Pack<T, V> ga[8], gb[8];

    auto load_slab = [&](i64 s) {
        const i64 r0 = s * RB + V * rp;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ca = bi * SYRK_TB + cgi + 16 * j, cb = bj * SYRK_TB + cgi + 16 * j;
#pragma unroll
            for (int e = 0; e < V; ++e) ga[j].v[e] = gb[j].v[e] = (T)0;
            if (vec && r0 + V <= N) {
                if (ca < K) ga[j] = ld_pack<T, V>(X + r0 + (i64)ca * ldx);
                if (cb < C) gb[j] = ld_pack<T, V>(G + r0 + (i64)cb * ldg);
            } else if (r0 < N) {  // ragged last rows, unaligned layouts: the missing slots stay zero
                for (int e = 0; e < V; ++e)
                    if (r0 + e < N) {
                        if (ca < K) ga[j].v[e] = X[r0 + e + (i64)ca * ldx];
                        if (cb < C) gb[j].v[e] = G[r0 + e + (i64)cb * ldg];
                    }
            }
        }
    };
    auto store_slab = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = cgi + 16 * j;
            constexpr int H = 8 / sizeof(T);
#pragma unroll
            for (int e = 0; e < V; e += H) {
                *reinterpret_cast<Pack<T, H> *>(As + c * LDP + V * rp + e) = *reinterpret_cast<const Pack<T, H> *>(&ga[j].v[e]);
                *reinterpret_cast<Pack<T, H> *>(Bs + c * LDP + V * rp + e) = *reinterpret_cast<const Pack<T, H> *>(&gb[j].v[e]);
            }
        }
    };

    const i64 per_split = (nslabs + gridDim.y - 1) / gridDim.y;  // a contiguous range of slabs per row split
    const i64 s_end = min(nslabs, (i64)(blockIdx.y + 1) * per_split);
    for (i64 s = (i64)blockIdx.y * per_split; s < s_end; ++s) {
        load_slab(s);
        __syncthreads();  // everyone is done reading the previous slab
        store_slab();
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < RB; kk += 4) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = (double)As[(a0 + 16 * m + li) * LDP + kk + lq];
#pragma unroll
            for (int n = 0; n < 4; ++n) b[n] = (double)Bs[(b0 + 16 * n + li) * LDP + kk + lq];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }

    // f64 C/D layout: lane holds D[row = (lane >> 4) + 4 * reg][col = lane & 15]; row <-> column of X, col <-> column of G
    double *o = out + (i64)blockIdx.y * pstride;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ga_ = bi * SYRK_TB + a0 + 16 * m + lq + 4 * r;
                const int gb_ = bj * SYRK_TB + b0 + 16 * n + li;
                if (ga_ < K && gb_ < C) o[ga_ + (i64)gb_ * ldo] = acc[m][n][r];
            }
}

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
