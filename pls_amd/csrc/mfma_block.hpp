// mfma_block.hpp -- the 128 x 128 block product on v_mfma_f64_16x16x4_f64 that xtg_kernel (syrk_kernels.hpp: X^T X and
// X^T G), xxt_kernel (dual_kernels.hpp: X X^T) and dual_xtvb_kernel (dual_batch_kernels.hpp: X^T V, V fp64) share.  Each kernel
// stages its own two panels into LDS; from there on the work is the same:
//   workgroup = 4 waves, wave (wv >> 1, wv & 1) owns a 64 x 64 quadrant = 4 x 4 MFMA tiles, 64 fp64 accumulators per lane;
//   a step of 4 contraction indices is 8 operand reads (lane l: row l & 15 of a tile, index l >> 4) and 16 MFMAs;
//   lane l leaves with D[row (l >> 4) + 4 reg][col l & 15] of every tile.
// The panels' LDS images differ -- [row][index + pad] or [index][row + pad], fp64 or the storage type -- so the two
// strides and the element type are template parameters; fp32 becomes fp64 at the operand read.
#pragma once
#include "common.hpp"

namespace plsk {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// entry idx of the upper triangle (i <= j) of an nb x nb grid, row by row
__device__ __forceinline__ void tri_block(int idx, int nb, int &i, int &j) {
    i = 0;
    while (idx >= nb - i) { idx -= nb - i; ++i; }
    j = i + idx;
}

struct QuadMap {
    int a0, b0, li, lq;  // first row / column of the wave's quadrant in the block; the lane's row in a tile, its index in a step
    __device__ __forceinline__ QuadMap() {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        a0 = (wv >> 1) * 64, b0 = (wv & 1) * 64;
        li = lane & 15, lq = lane >> 4;
    }
};

__device__ __forceinline__ void quad_zero(f64x4 (&acc)[4][4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// contraction indices kk .. kk + 3: row i, index k of a panel lies at [i * SI + k * SK]
template <int SI, int SK, typename TL>
__device__ __forceinline__ void quad_step(const TL *As, const TL *Bs, const QuadMap &q, int kk, f64x4 (&acc)[4][4]) {
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = (double)As[(q.a0 + 16 * m + q.li) * SI + (kk + q.lq) * SK];
#pragma unroll
    for (int n = 0; n < 4; ++n) b[n] = (double)Bs[(q.b0 + 16 * n + q.li) * SI + (kk + q.lq) * SK];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
}

// the block whose first entry is (i0, j0): out[gi + gj * ldo] for gi < ilim, gj < jlim; mirror: out[gj + gi * ldo] as well
__device__ __forceinline__ void quad_store(const f64x4 (&acc)[4][4], const QuadMap &q, double *__restrict__ out, i64 ldo, int i0,
                                           int j0, int ilim, int jlim, bool mirror) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + q.a0 + 16 * m + q.lq + 4 * r;
                const int gj = j0 + q.b0 + 16 * n + q.li;
                if (gi < ilim && gj < jlim) {
                    const double v = acc[m][n][r];
                    out[gi + (i64)gj * ldo] = v;
                    if (mirror) out[gj + (i64)gi * ldo] = v;
                }
            }
}

// the transposed block: out[gj + gi * ldo] for gi < ilim, gj < jlim.  The 16 lanes of a tile row store 16 consecutive entries
// of an output column (128 bytes), where quad_store leaves 4: for a product whose B panel runs along the output's rows
__device__ __forceinline__ void quad_store_t(const f64x4 (&acc)[4][4], const QuadMap &q, double *__restrict__ out, i64 ldo, int i0,
                                             i64 j0, int ilim, i64 jlim) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + q.a0 + 16 * m + q.lq + 4 * r;
                const i64 gj = j0 + q.b0 + 16 * n + q.li;
                if (gi < ilim && gj < jlim) out[gj + (i64)gi * ldo] = acc[m][n][r];
            }
}

// Row splits of a product of nblocks blocks on a chip of `slots` resident workgroups (2 per CU): all workgroups resident
// at once when the blocks allow it -- a grid that is one workgroup over a residency wave takes twice as long (measured:
// 520 workgroups 10.0 ms, 510 workgroups 6.5 ms) -- otherwise about `waves` residency waves, so that the tail is small.
inline i64 row_splits(i64 nblocks, i64 slots, i64 waves) {
    return nblocks <= slots ? slots / nblocks : (waves * slots + nblocks - 1) / nblocks;
}

}  // namespace plsk
