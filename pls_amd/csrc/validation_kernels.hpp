// validation_kernels.hpp -- model selection on cross-validation residuals (Model::validation / optimal_num_components,
// src/pls.cpp:190-211, :235-289): PRESS of every column of E, the reference column of every response, and the Wilcoxon
// signed-rank sums D of every (response, alternative) pair.
//
// E is the layout pls_hip_cv_folds writes: column (m, c) is the contiguous run E[(m A + c) nobs .. + nobs).
//
//   press_partial_kernel / press_finish_kernel   one streaming pass over E.  A column is cut into chunks of VAL_CH rows, one
//       workgroup and one partial per (column, chunk); the finish kernel adds a column's partials in index order.  The
//       chunk length is a constant, so the order of the additions depends on nobs and on the 16-byte phase of the column's
//       address only -- never on the grid, the device or the call.
//   signed_rank_lds_kernel      one workgroup per pair, columns that fit in LDS: keys + 16-bit row indices in LDS, bitonic
//       network on (|del|, row), rank-sum in int64.
//   radix_hist / radix_scan / radix_scatter       longer columns: stable LSD radix sort of the 63 magnitude bits, 8 bits per
//       pass, all pairs of a round in one grid.  The first pass forms the keys from E, the last pass does not store: a
//       key's final position IS its rank, so it adds rank * sign into the pair's int64 accumulator.
//
// The key of row i is the bit pattern of |del_i| (non-negative doubles order like their bits read as unsigned integers)
// with bit 63 set when del_i < 0.  sign = 0 for a zero magnitude and for a NaN.  Ties in |del| rank in row order.
// D is accumulated in int64 (LDS / global INTEGER atomics: exact, so the order of arrival does not matter).
#pragma once
#include "common.hpp"

namespace plsk {

constexpr int VAL_CH = 4096;                 // rows per PRESS partial: 256 threads x 8 loads of 16 bytes
constexpr int VAL_LDS_THREADS = 1024;
constexpr int VAL_LDS_ROW_BYTES = 10;        // 8-byte key + 2-byte row index
constexpr int VAL_LDS_MAX_ROWS = 16000;      // 160,000 bytes of the CU's 160 KiB (static LDS of the kernel: 8 bytes)
constexpr int VAL_LDS_ROWS_48K = 4800;       // what fits without raising the dynamic-LDS limit
constexpr int RADIX_ITEMS = 8;               // keys per thread and pass
constexpr int RADIX_SEG = WAVE * RADIX_ITEMS;  // consecutive keys of one wave
constexpr int RADIX_TILE = WG * RADIX_ITEMS;   // keys of one workgroup
constexpr int RADIX_PASSES = 8;
constexpr unsigned long long VAL_SIGN_BIT = 1ull << 63;

__device__ __forceinline__ unsigned long long val_key(double e_ref, double e_alt) {
    const double del = fabs(e_ref) - fabs(e_alt);
    unsigned long long k = (unsigned long long)__double_as_longlong(fabs(del));
    if (del < 0) k |= VAL_SIGN_BIT;
    return k;
}
__device__ __forceinline__ int val_sign(unsigned long long k) {
    const unsigned long long mag = k & ~VAL_SIGN_BIT;
    if (mag == 0 || mag > 0x7ff0000000000000ull) return 0;  // del == 0, or NaN
    return (k & VAL_SIGN_BIT) ? -1 : 1;
}

// probw = 1 - normalcdf((v - ev) / sv), the operations of the host wilcoxon() (src/pls.cpp:152-160, :204-210) in its order,
// unfused, so that host and device agree to the last bits.  n (n + 1) (2 n + 1) is formed in fp64: the reference's size_t
// product wraps beyond n = 2.09e6; below that both are the correctly rounded exact product.
__device__ inline double val_probw(double d, double n) {
#pragma clang fp contract(off)
    const double t = n * (n + 1.0) / 2.0;
    const double v = (t - d) / 2.0, ev = t / 2.0;
    const double sv = sqrt(n * (n + 1.0) * (2.0 * n + 1.0) / 24.0);
    const double z = (v - ev) / sv;
    const double a = fabs(z);
    const double poly = 1 + 0.196854 * a + 0.115194 * a * a + 0.000344 * a * a * a + 0.019527 * a * a * a * a;
    const double p2 = poly * poly;
    const double p = 0.5 / (p2 * p2);
    const double cdf = z < 0 ? p : 1.0 - p;
    return 1.0 - cdf;
}

__device__ __forceinline__ long long wave_sum_i64(long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}

// ---- PRESS ----------------------------------------------------------------------------------------------------------
// grid: nchunk * ncols workgroups (chunk fastest).  E: first element of the piece (column stride ld, `rows` rows, a
// multiple of VAL_CH unless it is the end of the column); part[(col0 + col) * nchunk_total + chunk0 + chunk].
__global__ __launch_bounds__(WG) void press_partial_kernel(const double *__restrict__ E, i64 ld, i64 rows, int nchunk, int chunk0,
                                                           int nchunk_total, i64 col0, double *__restrict__ part) {
    __shared__ double sm[WG / WAVE];
    const i64 col = blockIdx.x / nchunk;
    const int chunk = blockIdx.x % nchunk;
    const i64 r0 = (i64)chunk * VAL_CH;
    const int n = (int)min((i64)VAL_CH, rows - r0);
    const double *p = E + col * ld + r0;
    // 16-byte loads from the first 16-byte boundary on; the element before it (and an odd last one) go to thread 0
    const int head = min((int)(((uintptr_t)p >> 3) & 1), n);
    const double *q = p + head;
    const int m = n - head, npair = m >> 1;
    Pack<double, 2> v[VAL_CH / (2 * WG)];
#pragma unroll
    for (int j = 0; j < VAL_CH / (2 * WG); ++j) {
        const int k = (int)threadIdx.x + j * WG;
        if (k < npair) v[j] = ld_pack<double, 2>(q + 2 * k);
        else v[j].v[0] = v[j].v[1] = 0.0;
    }
    double s = 0.0;
    if (threadIdx.x == 0 && head) s = p[0] * p[0];
#pragma unroll
    for (int j = 0; j < VAL_CH / (2 * WG); ++j) {
        s = fma(v[j].v[0], v[j].v[0], s);
        s = fma(v[j].v[1], v[j].v[1], s);
    }
    if (threadIdx.x == 0 && (m & 1)) s = fma(q[m - 1], q[m - 1], s);
    s = block_sum<WG / WAVE>(s, sm);
    if (threadIdx.x == 0) part[(col0 + col) * nchunk_total + chunk0 + chunk] = s;
}

// grid: M workgroups.  PRESS[m + c M] = sum of the column's partials in index order; ref[m] = first column with the strictly
// smallest PRESS (the `<` scan of src/pls.cpp:271-277: a NaN never replaces the current minimum).
__global__ __launch_bounds__(WG) void press_finish_kernel(const double *__restrict__ part, int nchunk, int A, int M,
                                                          double *__restrict__ PRESS, long long *__restrict__ ref) {
    __shared__ double sm[WG / WAVE];
    const int m = blockIdx.x;
    double best = 0.0;
    int bi = 0;
    for (int c = 0; c < A; ++c) {
        const double *pp = part + ((i64)m * A + c) * nchunk;
        double s = 0.0;
        for (int k = threadIdx.x; k < nchunk; k += WG) s += pp[k];
        s = block_sum<WG / WAVE>(s, sm);
        if (threadIdx.x == 0) PRESS[m + (i64)c * M] = s;
        if (c == 0) best = s;
        else if (s < best) { best = s; bi = c; }
    }
    if (threadIdx.x == 0) ref[m] = bi;
}

// ---- one workgroup per pair ---------------------------------------------------------------------------------------------
// grid: M * A workgroups (alt fastest), VAL_LDS_THREADS threads, nobs * VAL_LDS_ROW_BYTES of dynamic LDS.  A workgroup
// with alt >= ref[m] writes D = 0, probw = NaN and leaves.  The network is the bitonic sorter with every comparator pointing
// up (the first step of a merge pairs i with its mirror image), so positions >= nobs act as +infinity without being stored.
__global__ __launch_bounds__(VAL_LDS_THREADS) void signed_rank_lds_kernel(const double *__restrict__ E, int nobs, int A, int M,
                                                                          const long long *__restrict__ ref,
                                                                          double *__restrict__ D, double *__restrict__ probw) {
    extern __shared__ unsigned long long val_dyn[];
    __shared__ long long acc;
    const int alt = blockIdx.x % A, m = blockIdx.x / A;
    const int r = (int)ref[m];
    const i64 o = m + (i64)alt * M;
    if (alt >= r) {
        if (threadIdx.x == 0) {
            D[o] = 0.0;
            probw[o] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }
    unsigned long long *key = val_dyn;
    unsigned short *row = reinterpret_cast<unsigned short *>(val_dyn + nobs);
    const double *er = E + ((i64)m * A + r) * nobs, *ea = E + ((i64)m * A + alt) * nobs;
    for (int i = threadIdx.x; i < nobs; i += VAL_LDS_THREADS) {
        key[i] = val_key(er[i], ea[i]);
        row[i] = (unsigned short)i;
    }
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    int P = 1;
    while (P < nobs) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += VAL_LDS_THREADS) {
                const int q = t & (j - 1), bs = (t & ~(j - 1)) << 1;  // j is a power of two
                const int lo = bs + q;
                const int hi = (j == (k >> 1)) ? bs + (k - 1 - q) : lo + j;
                if (hi < nobs) {
                    const unsigned long long a = key[lo], b = key[hi];
                    const unsigned long long am = a & ~VAL_SIGN_BIT, bm = b & ~VAL_SIGN_BIT;
                    const unsigned short ra = row[lo], rb = row[hi];
                    if (am > bm || (am == bm && ra > rb)) {
                        key[lo] = b; key[hi] = a;
                        row[lo] = rb; row[hi] = ra;
                    }
                }
            }
            __syncthreads();
        }
    }
    long long s = 0;
    for (int i = threadIdx.x; i < nobs; i += VAL_LDS_THREADS) s += (long long)(i + 1) * val_sign(key[i]);
    s = wave_sum_i64(s);
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&acc), (unsigned long long)s);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double d = (double)acc;
        D[o] = d;
        probw[o] = val_probw(d, (double)nobs);
    }
}

// ---- streaming route: stable LSD radix sort, 8 bits per pass ---------------------------------------------------------------
// A round covers the pairs [p0, p0 + gridDim.y) of the enumeration p = m (A - 1) + alt, alt < A - 1; a workgroup whose
// alt >= ref[m] leaves at once.  Workspace of pair slot y: keys y * nobs of either buffer, hist[(y * 256 + digit) * nblk + blk].
struct RadixPair {
    int m, alt, ref;
    bool live;
};
__device__ __forceinline__ RadixPair radix_pair(int p, int A, const long long *ref) {
    RadixPair o;
    o.m = p / (A - 1);
    o.alt = p % (A - 1);
    o.ref = (int)ref[o.m];
    o.live = o.alt < o.ref;
    return o;
}

template <bool FIRST>
__global__ __launch_bounds__(WG) void radix_hist_kernel(const double *__restrict__ E, const unsigned long long *__restrict__ src,
                                                        i64 nobs, int A, const long long *__restrict__ ref, int p0, int shift,
                                                        unsigned mask, int nblk, unsigned *__restrict__ hist) {
    __shared__ unsigned cnt[256];
    const RadixPair pr = radix_pair(p0 + blockIdx.y, A, ref);
    if (!pr.live) return;
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const double *er = E + ((i64)pr.m * A + pr.ref) * nobs, *ea = E + ((i64)pr.m * A + pr.alt) * nobs;
    const unsigned long long *s = src + (i64)blockIdx.y * nobs;
    const i64 base = (i64)blockIdx.x * RADIX_TILE;
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const i64 i = base + j * WG + threadIdx.x;
        if (i < nobs) {
            const unsigned long long k = FIRST ? val_key(er[i], ea[i]) : s[i];
            atomicAdd(&cnt[(unsigned)(k >> shift) & mask], 1u);
        }
    }
    __syncthreads();
    hist[((i64)blockIdx.y * 256 + threadIdx.x) * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// grid: one workgroup of 1024 threads per pair slot; exclusive prefix sum over the slot's 256 * nblk counts (digit-major), in place
__global__ __launch_bounds__(1024) void radix_scan_kernel(unsigned *__restrict__ hist, int L, int A, const long long *__restrict__ ref,
                                                          int p0) {
    __shared__ unsigned sums[1024];
    if (!radix_pair(p0 + blockIdx.x, A, ref).live) return;
    unsigned *h = hist + (i64)blockIdx.x * L;
    const int per = (L + 1023) / 1024;
    const int lo = min(L, (int)threadIdx.x * per), hi = min(L, lo + per);
    unsigned s = 0;
    for (int k = lo; k < hi; ++k) s += h[k];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned v = (int)threadIdx.x >= off ? sums[threadIdx.x - off] : 0u;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = sums[threadIdx.x] - s;
    for (int k = lo; k < hi; ++k) {
        const unsigned t = h[k];
        h[k] = run;
        run += t;
    }
}

// Stable scatter.  Wave w owns the consecutive keys [w RADIX_SEG, + RADIX_SEG) of the tile and walks them 64 at a time: the
// lanes with the same digit find each other with 8 ballots, a key's offset inside its wave's run of that digit is the wave's
// count so far plus the number of such lanes below it.  Afterwards the four waves' counts are stacked in wave order on the
// scanned histogram entry of (digit, this workgroup).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(WG) void radix_scatter_kernel(const double *__restrict__ E, const unsigned long long *__restrict__ src,
                                                           unsigned long long *__restrict__ dst, i64 nobs, int A,
                                                           const long long *__restrict__ ref, int p0, int shift, unsigned mask,
                                                           int nblk, const unsigned *__restrict__ hist,
                                                           long long *__restrict__ acc) {
    __shared__ unsigned cnt[WG / WAVE][256];
    __shared__ long long wsum[WG / WAVE];
    const RadixPair pr = radix_pair(p0 + blockIdx.y, A, ref);
    if (!pr.live) return;
    for (int k = threadIdx.x; k < (WG / WAVE) * 256; k += WG) (&cnt[0][0])[k] = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & (WAVE - 1);
    const double *er = E + ((i64)pr.m * A + pr.ref) * nobs, *ea = E + ((i64)pr.m * A + pr.alt) * nobs;
    const unsigned long long *s = src + (i64)blockIdx.y * nobs;
    const i64 seg = (i64)blockIdx.x * RADIX_TILE + (i64)w * RADIX_SEG;
    volatile unsigned *cw = cnt[w];
    const unsigned long long below_me = (1ull << lane) - 1ull;
    unsigned long long key[RADIX_ITEMS];
    unsigned off[RADIX_ITEMS];
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const i64 i = seg + j * WAVE + lane;
        const bool valid = i < nobs;
        key[j] = valid ? (FIRST ? val_key(er[i], ea[i]) : s[i]) : 0ull;
        const unsigned d = (unsigned)(key[j] >> shift) & mask;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const unsigned long long below = peers & below_me;
        const unsigned pre = cw[d];
        off[j] = pre + (unsigned)__popcll(below);
        __builtin_amdgcn_wave_barrier();
        if (valid && below == 0) cw[d] = pre + (unsigned)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // digit threadIdx.x: counts of the waves -> their start positions in the output
        unsigned run = hist[((i64)blockIdx.y * 256 + threadIdx.x) * nblk + blockIdx.x];
#pragma unroll
        for (int ww = 0; ww < WG / WAVE; ++ww) {
            const unsigned t = cnt[ww][threadIdx.x];
            cnt[ww][threadIdx.x] = run;
            run += t;
        }
    }
    __syncthreads();
    long long a = 0;
    unsigned long long *o = dst + (i64)blockIdx.y * nobs;
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const i64 i = seg + j * WAVE + lane;
        if (i < nobs) {
            const unsigned d = (unsigned)(key[j] >> shift) & mask;
            const i64 pos = (i64)cnt[w][d] + off[j];
            if constexpr (LAST) a += (pos + 1) * val_sign(key[j]);
            else o[pos] = key[j];
        }
    }
    if constexpr (LAST) {
        a = wave_sum_i64(a);
        if (lane == 0) wsum[w] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long t = 0;
#pragma unroll
            for (int ww = 0; ww < WG / WAVE; ++ww) t += wsum[ww];
            atomicAdd(reinterpret_cast<unsigned long long *>(acc + (i64)pr.m * A + pr.alt), (unsigned long long)t);
        }
    }
}

// one thread per (m, c): D and probw from the int64 rank sums; 0 and NaN where c >= ref[m]
__global__ __launch_bounds__(WG) void signed_rank_finish_kernel(const long long *__restrict__ acc, i64 nobs, int A, int M,
                                                                const long long *__restrict__ ref, double *__restrict__ D,
                                                                double *__restrict__ probw) {
    const i64 idx = (i64)blockIdx.x * WG + threadIdx.x;
    if (idx >= (i64)M * A) return;
    const int m = (int)(idx / A), c = (int)(idx % A);
    const i64 o = m + (i64)c * M;
    if (c < ref[m]) {
        const double d = (double)acc[idx];
        D[o] = d;
        probw[o] = val_probw(d, (double)nobs);
    } else {
        D[o] = 0.0;
        probw[o] = __longlong_as_double(0x7ff8000000000000ll);
    }
}

}  // namespace plsk
