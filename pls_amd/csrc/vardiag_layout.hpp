// vardiag_layout.hpp -- the tile, the row splits, the component ranges and the workspace of pls_hip_var_diagnostics:
// vardiag_geom_of, a pure function of (N, K, A, element size, CU count, alignment).  plan_vardiag.hpp only executes what it
// returns.  Plain C++17, no HIP and no handle: tests/cpp/vardiag_layout.cpp builds it with the host compiler alone.
//
// The column sweep (vardiag_kernels.hpp): lanes run across the VD_TC = 64 columns of a column block, a workgroup stages tiles of
// VD_TR = 128 rows x 64 columns into LDS as fp64 (every column padded to VD_TR + 1 elements) and reads them back transposed.
// Workgroup (cb, rs) owns column block cb and the contiguous row tiles [vd_tile_lo(rs), vd_tile_lo(rs + 1)): every (row tile,
// column block) has exactly one owner.  RS = the row splits: as many as give every CU VD_WG_PER_CU workgroups (the tile of one
// workgroup is 66 KB of the CU's 160 KB), never more than there are row tiles.  One sweep covers a range of at most VD_RANGE
// component counts, range j the counts VD_RANGE j + 1 .. min(A, VD_RANGE (j + 1)); the kernel of a range computes CR = the count
// rounded up to four.  The partial sums of a range, one plane of K values per count (and one for the squares of X in the first
// range), one set per row split, are added in split order by reduce_partials_kernel.
#pragma once
#include <algorithm>
#include <cstdint>

namespace plsk {

typedef long long vd_i64;

constexpr int VD_TC = 64;        // columns of a tile = lanes of a wave
constexpr int VD_TR = 128;       // rows of a tile: 1 KiB column pieces in fp64 storage
constexpr int VD_LDC = VD_TR + 1;  // elements between two columns of the tile in LDS: odd, so that a half wave reading one row of 32 columns touches every bank once
constexpr int VD_RANGE = 24;     // component counts per sweep: 4 VGPRs each (loading + running sum of one column)
constexpr int VD_WG_PER_CU = 2;  // workgroups a CU holds (LDS)
constexpr int VD_THREADS = 256;  // == WG (held by a static_assert in the plan)
constexpr int VD_RED_SLICES = 8;  // == RED_SLICES (held by a static_assert in the plan)
constexpr vd_i64 VD_LDS_CU = 160 << 10;
constexpr vd_i64 VD_TILE_BYTES = (vd_i64)VD_TC * VD_LDC * 8;
constexpr vd_i64 VD_INT_MAX = 2147483647;

struct VdGeom {
    int vec;       // rows per lane of a load from X: 16 / es when the alignment allows it, else 1
    vd_i64 NT;     // row tiles
    vd_i64 CB;     // column blocks
    int RS;        // row splits
    int nranges;   // sweeps
    int AS;        // components of a row of the row-contiguous scores: A rounded up to four (zero-padded)
    vd_i64 lds_bytes;  // dynamic LDS of a workgroup
    // partials of one range: value (rs, j, k) at rs * p_rs + j * p_j + k.  One launch of the reduction adds all planes of a range
    // while they fit its 32-bit length (p_one_launch: p_rs = L K, p_j = K); beyond that a launch per plane (p_j = RS K, p_rs = K).
    int p_one_launch;
    vd_i64 part_bytes;  // the largest range's partials
    vd_i64 st_bytes;    // the row-contiguous scores: NT * VD_TR rows of AS
    vd_i64 msg_values;  // values of one slice of the message: A + K (A + 1) with ssxk, A without
};

inline int vd_range_lo(int j) { return j * VD_RANGE; }
inline int vd_range_hi(int j, int A) { return std::min(A, (j + 1) * VD_RANGE); }
inline int vd_cr(int nc) { return (nc + 3) / 4 * 4; }
inline vd_i64 vd_tile_lo(vd_i64 NT, int RS, int rs) { return NT * rs / RS; }

// aligned: pointer and leading dimension of X allow 16-byte loads.  with_ssxk: the column sweep is asked for.
inline VdGeom vardiag_geom_of(vd_i64 N, vd_i64 K, vd_i64 A, int es, int num_cu, bool aligned, bool with_ssxk = true) {
    VdGeom g{};
    g.vec = aligned ? 16 / es : 1;
    g.NT = (N + VD_TR - 1) / VD_TR;
    g.CB = (K + VD_TC - 1) / VD_TC;
    const vd_i64 want = ((vd_i64)VD_WG_PER_CU * num_cu + g.CB - 1) / g.CB;
    g.RS = (int)std::max<vd_i64>(1, std::min<vd_i64>(want, g.NT));
    g.nranges = (int)((A + VD_RANGE - 1) / VD_RANGE);
    g.AS = (int)((A + 3) / 4 * 4);
    g.lds_bytes = VD_TILE_BYTES;
    const vd_i64 Lmax = std::min<vd_i64>(A, VD_RANGE) + 1;
    g.p_one_launch = K * Lmax <= VD_INT_MAX - 64 ? 1 : 0;
    g.part_bytes = with_ssxk ? (vd_i64)g.RS * Lmax * K * 8 : 0;
    g.st_bytes = with_ssxk ? g.NT * VD_TR * g.AS * 8 : 0;
    g.msg_values = A + (with_ssxk ? K * (A + 1) : 0);
    return g;
}

}  // namespace plsk
