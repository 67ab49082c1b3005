// The body of fused_pass_kernel's tile loop (fused_kernels.hpp): one tile -- loads, [deflation + stores,] score, loading
// partials.  Included once per cache-policy pair of the loop, inside a block that declares
//     constexpr int LA, SA;   // cache-policy bits of the tile's loads / stores
// and has `tile` (the tile's index) in scope.  The policy is an immediate of the buffer instructions, so a sweep whose
// edges take another policy than its bulk needs one copy of the body per pair; the text is shared through the preprocessor,
// not through a function: wrapped in an inlined lambda the same statements compiled to other register allocations -- the
// 128-register read-only shapes went from 24 to 44 bytes of scratch per lane (profiles/turnaround/resources.txt).
        const i64 i0 = tile * R + (i64)rp * V;
        const bool rowok = (i0 < N);  // N % V == 0 (launcher): a pack is all-valid or all-invalid
        const uint32_t xo = rowok ? xoff : OOR, dof = rowok ? doff : OOR;
        // LDS operands (v, p_prev) are re-read every tile: an index the compiler cannot prove
        // loop-invariant keeps 2*CPT fp64 values out of the register file
        int cgz = cg;
        asm volatile("" : "+v"(cgz));
        if constexpr (TILED && DEFL && STORE) {
            // pacing: `rdst` x 64 cycles of s_sleep before a tile's loads go out (launcher)
            if (!LATE_FILL || !first_tile)  // (nothing is in flight before the first tile)
                for (int q = 0; q < pace; ++q) __builtin_amdgcn_s_sleep(1);
        }
        Pack<T, V> x[CPT];
        constexpr int GSTEP = CG * R * (int)sizeof(T);  // TILED: bytes between the column groups of a tile
        const int trec = K * R * (int)sizeof(T);        // TILED: bytes of a tile
        if constexpr (TILED) {
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(X + tile * tsx), (short)0, trec, BUF_WORD3);
#pragma unroll
            for (int j = 0; j < CPT; ++j) x[j] = buf_ld_so<T, V, LA>(rs, xo, j * GSTEP);
            __builtin_amdgcn_sched_barrier(0);  // all CPT loads in flight before anything consumes the first
            if constexpr (LATE_OK) {
                if (LATE_FILL && first_tile) {  // (uniform)
                    first_tile = false;
                    if (tid < CG * CPT) {
                        vs[tid] = v_late;
                        ps[tid] = p_late;
                    }
                    __syncthreads();
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int cols = min(CGD, K - CG * j - cgw);  // columns of this group that exist (may be <= 0)
                const uint32_t nrec = cols > 0 ? (uint32_t)((i64)cols * ldx * (i64)sizeof(T)) : 0u;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<T *>(X + tile * tsx + (i64)(j * CG + cgw) * ldx), (short)0, (int)nrec, BUF_WORD3);
                x[j] = buf_ld<T, V, LA>(rs, xo);
                __builtin_amdgcn_sched_barrier(0);  // build one descriptor, issue its load, repeat
            }
        }
        if (DEFL) {
            double tp[V];
            {
                // t_prev of the lane's rows; behind row NV (padded sweeps) zeros.  Two forms, chosen per instantiation by
                // measurement (same box, A/B): through a range-checked buffer descriptor -- the headline shape: 701 vs 693
                // components/s at config 3 -- or as a plain 16-byte load with an element-wise branch for the one straddling
                // pack -- every other shape: +0.3 ... +0.7 % (config 4, the shards of configs 3 and 5).
                Pack<T, V> tpk;
                if constexpr (TBUF) {
                    tpk = buf_ld<T, V>(rs_tin, rowok ? (uint32_t)(i0 * (i64)sizeof(T)) : OOR);
                } else if (rowok && i0 + V <= NV) {
                    tpk = ld_pack_u<T, V>(tprev + i0);
                } else {  // (rows the sweep does not cover must contribute nothing: the tail kernel owns row NV - 1 of an odd matrix)
#pragma unroll
                    for (int e = 0; e < V; ++e) tpk.v[e] = (rowok && i0 + e < NV) ? tprev[i0 + e] : (T)0;
                }
#pragma unroll
                for (int e = 0; e < V; ++e) tp[e] = -(double)tpk.v[e];
            }
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const double pk = ps[cgz + CG * j];
#pragma unroll
                for (int e = 0; e < V; ++e) x[j].v[e] = (T)fma(tp[e], pk, (double)x[j].v[e]);
                if constexpr (!STORE) {
                    continue;  // the deflated tile lives in registers only
                } else if constexpr (TILED) {
                    const __amdgpu_buffer_rsrc_t rd =
                        __builtin_amdgcn_make_buffer_rsrc(dst + tile * tsd, (short)0, trec, BUF_WORD3);
                    // (write-through stores -- sc1 | nt, sc0 | sc1 | nt: nothing dirty in L2 when the launch ends -- measured in
                    // round 5: the pass +2.5 us on a shard, +23 us at config 3, the boundary behind it no shorter)
                    buf_st_so<T, V, SA>(rd, dof, j * GSTEP, x[j]);
                } else if constexpr (RDST) {  // lane offsets span several destination tiles: columns >= K masked per lane
                    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                        dst + tile * dtile + (i64)j * CG * ldd, (short)0, 0x7fffffff, BUF_WORD3);
                    buf_st<T, V, SA>(rd, (cg + CG * j < K) ? dof : OOR, x[j]);
                } else {
                    const int cols = min(CG, K - CG * j);
                    const uint32_t nrec = cols > 0 ? (uint32_t)((i64)cols * ldd * (i64)sizeof(T)) : 0u;
                    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
                        dst + tile * tsd + (i64)j * CG * ldd, (short)0, (int)nrec, BUF_WORD3);
                    buf_st<T, V, SA>(rd, dof, x[j]);
                }
            }
        }
        // the deflated tile goes out BEFORE the score arithmetic (left to itself the compiler sinks the stores behind the
        // score FMAs and the first butterfly level: 1.387 instead of 1.354 ms per launch at config 3)
        if constexpr (DEFL && STORE) __builtin_amdgcn_sched_barrier(0);
        // score: partial over this lane's columns, then over the lanes / waves sharing the rows
        double tp2[V];
#pragma unroll
        for (int e = 0; e < V; ++e) tp2[e] = 0.0;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const double vk = vs[cgz + CG * j];
#pragma unroll
            for (int e = 0; e < V; ++e) tp2[e] = fma((double)x[j].v[e], vk, tp2[e]);
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
            tp2[e] = xor_range_sum<RP, WAVE>(tp2[e]);
        if (lane < RP)
#pragma unroll
            for (int e = 0; e < V; ++e) tred[buf][wv][rp * V + e] = tp2[e];
        __syncthreads();
        double t[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += tred[buf][w][rp * V + e];
            t[e] = (double)(T)s;  // the score as stored
        }
        if (cg == 0 && rowok) {
            Pack<T, V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = (T)t[e];
            if (i0 + V <= NV) {
                st_pack_u<T, V>(tout + i0, o);
            } else {  // the pack that straddles the last valid row (padded sweeps only)
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (i0 + e < NV) tout[i0 + e] = o.v[e];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) ss = fma(t[e], t[e], ss);
        }
        // loading: p_raw[k] += sum over the lane's rows of x[i,k] * t[i]   (rows >= N hold x = 0)
        // fp32 storage: the tile is converted to fp64 again here -- the empty asm hides the stored values from
        // common-subexpression elimination, which would otherwise keep the fp64 copies of the whole tile made for
        // the score alive across the barrier (2x the registers of the tile: 135-217 spilled VGPRs, 2.3 TB/s)
        if (sizeof(T) < sizeof(double)) {
#pragma unroll
            for (int j = 0; j < CPT; ++j)
#pragma unroll
                for (int e = 0; e < V; ++e) asm volatile("" : "+v"(x[j].v[e]));
        }
#pragma unroll
        for (int j = 0; j < CPT; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) pacc[j] = fma((double)x[j].v[e], t[e], pacc[j]);
