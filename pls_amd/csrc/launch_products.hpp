// launch_products.hpp -- typed launchers of the streaming products over X: X B / X v, X^T Y / X^T t, the stand-alone deflation, the fixed-order reduction of partial rows.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
#pragma once

namespace {

// ---- geometry -------------------------------------------------------------------------
using plsk::XTY_KCMT;  // accumulators per lane in xty_kernel (fit_route.hpp)
constexpr int DEFL_KC = 32;

struct XtyGeom {
    int G;    // row groups = number of partial rows (same for every m-tile of one product)
    int nkg;  // column groups of this m-tile
};
// All m-tiles of one X^T Y write the same number of partial rows G.  It is derived from the column groups of the
// product's FIRST tile (kc_first columns each; the first tile is the widest in m, i.e. the one with the most column
// groups): with G from the 32-column shape instead, the 8-response tile of config 4 ran 16,384 workgroups of 8 row
// chunks each and spent half its time in their 32 butterfly sums (1.0 ms = 2.1 TB/s, fp32 and fp64 alike).
XtyGeom xty_geom(i64 N, int K, int KC, int vec, int target_wgs, int kc_first) {
    XtyGeom g;
    g.nkg = (K + KC - 1) / KC;
    const int nkg32 = (K + kc_first - 1) / kc_first;
    const i64 nch = (N + (i64)plsk::WG * vec - 1) / ((i64)plsk::WG * vec);
    i64 G = std::max<i64>(1, target_wgs / nkg32);
    G = std::min<i64>(G, std::max<i64>(nch, 1));
    g.G = (int)G;
    return g;
}
// upper bound of partial rows any product of this fit can write
i64 max_partial_rows(pls_hip_context *c, i64 N, int K) { return plsk::max_partial_rows(c->num_cu, c->opt_fused_grid, N, K); }

// ---- typed launchers --------------------------------------------------------------------
template <int C0, int... Cs, typename F>
auto pick_int(int v, F &&f) -> decltype(f(std::integral_constant<int, C0>{}));  // plan_common.hpp

// the 4 x 4 x 4 MFMA kernel of a step (nullptr: the step's route is none of theirs).  No 7 or 8 column groups with fp32 storage,
// no windowed kernel of one group.
template <typename T>
const void *xb4_kernel(const plsk::XbStep &st) {
    constexpr int FV = 16 / sizeof(T);
    if (st.route != plsk::XB_MFMA4 && st.route != plsk::XB_MFMA4W && st.route != plsk::XB_MFMA4W_SPLIT) return nullptr;
    auto of = [&](auto g) -> const void * {
        constexpr int G = decltype(g)::value;
        if (st.route == plsk::XB_MFMA4) return (const void *)plsk::xb_mfma4_kernel<T, FV, G>;
        if constexpr (G >= 2) return (const void *)plsk::xb_mfma4w_kernel<T, FV, G>;
        return nullptr;
    };
    if constexpr (sizeof(T) == 8) return pick_int<1, 2, 3, 4, 5, 6, 7, 8>(st.sel, of);
    else return pick_int<1, 2, 3, 4, 5, 6>(st.sel, of);
}

// out(N x C) = X * Bm ; optionally sum of squares partials of column 0 (C must be 1 then).  Executes the steps of xb_next
// (xb_route.hpp: every route and threshold): a step whose resource is denied is asked for again without that route.
template <typename T>
int launch_xb(pls_hip_context *c, const T *X, i64 ldx, i64 N, int K, const double *Bm, i64 ldb,
              int C, T *out, i64 ldo, double *sspart, int *nss) {
    constexpr int FV = 16 / sizeof(T);
    const plsk::XbShape shape{N, K, C, ldx, ldo, (int)sizeof(T), plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), FV), plsk::vec_ok((uintptr_t)out, ldo, sizeof(T), FV), c->num_cu, c->env.xb4, sspart != nullptr};
    unsigned denied = 0;
    for (int c0 = 0; c0 < C;) {
        const plsk::XbStep st = plsk::xb_next(shape, c0, denied);
        const void *fn4 = xb4_kernel<T>(st);
        if (st.gy > 65535 || (fn4 && !plsk::raise_dynamic_lds(fn4, (int)st.lds)) ||
            (st.part_bytes && ensure(c, c->xbpart, st.part_bytes) != PLS_HIP_OK)) {
            if (st.part_bytes) c->err.clear();
            denied |= plsk::xb_bit(st.route);
            if (plsk::XB_WHOLE_CALL & plsk::xb_bit(st.route)) c0 = 0;  // (columns already written are written again)
            continue;
        }
        const double *b = Bm + (i64)c0 * ldb;
        T *o = out + (i64)c0 * ldo;
        double *xp = st.part_bytes ? (double *)c->xbpart.p : nullptr;
        const int fb = (int)((N + 63) / 64);  // workgroups per column of xb_split_finish_kernel
        const dim3 grid(st.gx, st.gy), blk(plsk::WG);
        int use = st.use;
        Scope s(c, st.fam, st.bytes);
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, blk, 0, c->stream, X, ldx, N, K, b, ldb, use, o, ldo); };
        auto vec = [&](auto &&f) { pick_int<1, FV>(st.vec, f); };  // f(rows per lane)
        switch (st.route) {
            case plsk::XB_MFMA4:
            case plsk::XB_MFMA4W:
            case plsk::XB_MFMA4W_SPLIT: {
                int sw = st.sw, kp = st.kper;
                i64 lp = st.ldp;  // (xb_mfma4_kernel takes the first nine)
                void *args[] = {(void *)&X, (void *)&ldx, (void *)&N, (void *)&K, (void *)&b, (void *)&ldb, (void *)&use, (void *)&o, (void *)&ldo,
                                (void *)&sw, (void *)&kp, (void *)&xp, (void *)&lp};
                if (hipLaunchKernel(fn4, grid, dim3(plsk::XB4_WG), args, st.lds, c->stream) != hipSuccess) {
                    c->err = st.route == plsk::XB_MFMA4 ? "kernel launch: xb_mfma4"
                                                        : st.route == plsk::XB_MFMA4W ? "kernel launch: xb_mfma4w" : "kernel launch: xb_mfma4w (split)";
                    (void)hipGetLastError();
                    return PLS_HIP_ERR_DEVICE;
                }
                if (st.route != plsk::XB_MFMA4W_SPLIT) break;
                hipLaunchKernelGGL((plsk::xb_split_finish_kernel<T>), dim3(fb, use), blk, 0, c->stream, (const double *)xp, st.ldp, st.ks, 4 * st.sel, N,
                                   o, ldo, (double *)nullptr);
                LAUNCH_CHECK(c);
                break;
            }
            case plsk::XB_SPLIT:
                vec([&](auto v) {
                    pick_int<1, 2, 4>(st.sel, [&](auto m) {
                        hipLaunchKernelGGL((plsk::xb_split_kernel<T, decltype(v)::value, decltype(m)::value>), grid, blk, 0, c->stream, X, ldx, N, K,
                                           st.kper, b, ldb, use, xp, st.ldp);
                    });
                });
                LAUNCH_CHECK(c);
                hipLaunchKernelGGL((plsk::xb_split_finish_kernel<T>), dim3(fb, use), blk, 0, c->stream, (const double *)xp, st.ldp, st.ks, st.sel, N, o,
                                   ldo, C == 1 ? sspart : (double *)nullptr);
                LAUNCH_CHECK(c);
                if (C == 1 && sspart && nss) *nss = fb;
                break;
            case plsk::XB_MFMA_LDS: {  // (fp64 storage runs 3 or 4 tiles of 16 columns, fp32 1 or 2 -- and has no more)
                auto tiles = [&](auto nt) { go(plsk::xb_mfma_lds_kernel<T, FV, decltype(nt)::value>); };
                if constexpr (sizeof(T) == 8) pick_int<1, 2, 3, 4>(st.sel, tiles);
                else pick_int<1, 2>(st.sel, tiles);
                LAUNCH_CHECK(c);
                break;
            }
            case plsk::XB_WIDE2:
                if constexpr (FV == 2) pick_int<16, 20>(st.sel, [&](auto m) { go(plsk::xb_wide_kernel<T, 2, decltype(m)::value, 2>); });
                LAUNCH_CHECK(c);
                break;
            case plsk::XB_WIDE:
                vec([&](auto v) {
                    constexpr int V = decltype(v)::value;
                    auto tile = [&](auto m) { go(plsk::xb_wide_kernel<T, V, decltype(m)::value>); };
                    if constexpr (V == 4) tile(std::integral_constant<int, 8>{});  // (fp32 at 4 rows per lane: 8 columns, xb_next)
                    else pick_int<8, 12, 16, 20, 24, 28, 32>(st.sel, tile);
                });
                LAUNCH_CHECK(c);
                break;
            case plsk::XB_KERNEL:
                vec([&](auto v) {
                    constexpr int V = decltype(v)::value;
                    if (st.ss) {
                        hipLaunchKernelGGL((plsk::xb_kernel<T, V, 1, true>), grid, blk, 0, c->stream, X, ldx, N, K, b, ldb, use, o, ldo, sspart);
                        *nss = (int)st.gx;
                    } else {
                        pick_int<1, 2, 4>(st.sel, [&](auto m) {
                            hipLaunchKernelGGL((plsk::xb_kernel<T, V, decltype(m)::value, false>), grid, blk, 0, c->stream, X, ldx, N, K, b, ldb, use, o,
                                               ldo, (double *)nullptr);
                        });
                    }
                });
                LAUNCH_CHECK(c);
                break;
        }
        c0 += use;
        denied &= plsk::XB_WHOLE_CALL;  // (the next columns may be another kernel: they ask for theirs)
    }
    return PLS_HIP_OK;
}

template <typename T, int VEC, int KC, int MT>
void launch_xty_t(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M,
                  int m0, double *part, const XtyGeom &g) {
    hipLaunchKernelGGL((plsk::xty_kernel<T, VEC, KC, MT>), dim3(g.G, g.nkg), dim3(plsk::WG), 0,
                       c->stream, X, ldx, Y, ldy, N, K, M, m0, part);
}

// part[G][K*M] = per-row-group partials of X^T Y; returns G through *nb
template <typename T>
int launch_xty(pls_hip_context *c, const T *X, i64 ldx, const T *Y, i64 ldy, i64 N, int K, int M,
               double *part, int *nb) {
    constexpr int FV = 16 / sizeof(T);
    const bool wide = plsk::vec_ok((uintptr_t)X, ldx, sizeof(T), FV) && plsk::vec_ok((uintptr_t)Y, ldy, sizeof(T), FV);
    // workgroups per CU aimed at: 8; 4 with 8-response tiles, whose 32 butterfly sums per workgroup want longer walks
    // (config 4, fp32: 0.55 ms at 4, 0.59 at 8, 0.77 at 32 -- tools/xty_m8.py)
    const int target = (M >= 8 ? 4 : 8) * c->num_cu;
    int m0 = 0;
    const int kc_first = XTY_KCMT / ((M >= 8) ? 8 : (M >= 4 ? 4 : (M >= 2 ? 2 : 1)));
    while (m0 < M) {
        const int mt = (M - m0 >= 8) ? 8 : (M - m0 >= 4 ? 4 : (M - m0 >= 2 ? 2 : 1));
        // 8 responses: 8 columns per workgroup (64 accumulators per lane) -- the Y packs of a row chunk are loaded once
        // per column group, so 4 columns meant twice as many bytes of Y as of X through L2 (1.0 ms = 2.1 TB/s at config 4)
        const int kc = XTY_KCMT / mt;
        const XtyGeom g = xty_geom(N, K, kc, wide ? FV : 1, target, kc_first);
        *nb = g.G;
        const i64 bytes = (i64)N * K * sizeof(T) + (i64)N * mt * sizeof(T) + (i64)K * mt * 8;
        Scope s(c, PLS_HIP_FAM_XTY, bytes);
        // 8 responses in one go: the copy-and-product sweep WITHOUT its copy (retile_xty_kernel, dst == nullptr) -- the Y block of
        // a tile goes through LDS once instead of 8 packs per lane and 4 columns (xty8_kernel: 0.49 / 0.60 of peak in fp32 / fp64)
        int rx_nb = 0;
        // ... and 1, 2 or 4 responses up to 2,048 columns: the tile walk streams X at 0.85 of peak where xty_kernel's row chunks
        // reach 0.76 (config 3, one response: 0.708 -> 0.631 ms; 131,072 x 4,096 is faster on the chunks: tools/probe/xty1.py)
        if (wide && ((mt == 8 && M == 8) || (mt == M && K <= 2048)) && m0 == 0 && K >= 256 && plsk::cols_aligned((uintptr_t)X, ldx, sizeof(T)) &&
            plsk::launch_retile_xty<T, 32>(c->stream, c->num_cu, X, ldx, Y, ldy, (T *)nullptr, 0, 0, 0, N, K, M, part,
                                           (int)max_partial_rows(c, N, K), &rx_nb) == 0) {
            *nb = rx_nb;
        } else if (wide && mt == 8 && K % 4 == 0) {
            hipLaunchKernelGGL((plsk::xty8_kernel<T, FV>), dim3(g.G, g.nkg), dim3(plsk::WG), 0, c->stream, X, ldx, Y, ldy, N, K,
                               M, m0, part);
        } else {
            pick_int<1, FV>(wide ? FV : 1, [&](auto v) {
                pick_int<1, 2, 4, 8>(mt, [&](auto m) {
                    constexpr int MT = decltype(m)::value;
                    launch_xty_t<T, decltype(v)::value, XTY_KCMT / MT, MT>(c, X, ldx, Y, ldy, N, K, M, m0, part, g);
                });
            });
        }
        LAUNCH_CHECK(c);
        m0 += mt;
    }
    return PLS_HIP_OK;
}

template <typename T>
int launch_deflate(pls_hip_context *c, const T *src, i64 lds, T *dst, i64 ldd, i64 N, int K,
                   const T *t, const double *p) {
    constexpr int FV = 16 / sizeof(T);
    const bool wide = plsk::vec_ok((uintptr_t)src, lds, sizeof(T), FV) && plsk::vec_ok((uintptr_t)dst, ldd, sizeof(T), FV) && plsk::vec_ok((uintptr_t)t, FV, sizeof(T), FV);
    const int nkg = (K + DEFL_KC - 1) / DEFL_KC;
    const int vec = wide ? FV : 1;
    const i64 nch = (N + (i64)plsk::WG * vec - 1) / ((i64)plsk::WG * vec);
    const i64 G = std::min<i64>(std::max<i64>(nch, 1), std::max<i64>(1, (16 * c->num_cu) / nkg));
    const i64 bytes = 2 * (i64)N * K * sizeof(T) + (i64)N * sizeof(T) + (i64)K * 8;
    Scope s(c, PLS_HIP_FAM_DEFLATE, bytes);
    const i64 nrb = (N + (i64)plsk::WG * FV - 1) / ((i64)plsk::WG * FV);
    if (wide && K <= 65535 && nrb >= 1 && nrb < (1ll << 31)) {  // one 4 KB column piece per workgroup
        hipLaunchKernelGGL((plsk::deflate_piece_kernel<T, FV>), dim3((unsigned)nrb, (unsigned)K), dim3(plsk::WG), 0,
                           c->stream, src, lds, dst, ldd, N, t, p);
        LAUNCH_CHECK(c);
        return PLS_HIP_OK;
    }
    if (wide)
        hipLaunchKernelGGL((plsk::deflate_kernel<T, FV, DEFL_KC>), dim3((unsigned)G, nkg),
                           dim3(plsk::WG), 0, c->stream, src, lds, dst, ldd, N, K, t, p);
    else
        hipLaunchKernelGGL((plsk::deflate_kernel<T, 1, DEFL_KC>), dim3((unsigned)G, nkg),
                           dim3(plsk::WG), 0, c->stream, src, lds, dst, ldd, N, K, t, p);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

int launch_reduce(pls_hip_context *c, const double *part, int nb, int L, const double *sspart,
                  int nss, double *red, i64 out_stride = 0) {
    Scope s(c, PLS_HIP_FAM_SMALL, ((i64)nb * L + nss + (i64)plsk::RED_SLICES * (L + 1)) * 8);
    hipLaunchKernelGGL(plsk::reduce_partials_kernel, dim3((L + 63) / 64, plsk::RED_SLICES),
                       dim3(plsk::WG), 0, c->stream, part, nb, L, sspart, nss, red, out_stride);
    LAUNCH_CHECK(c);
    return PLS_HIP_OK;
}

}  // namespace
