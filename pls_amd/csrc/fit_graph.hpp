// fit_graph.hpp -- PLS_HIP_OPT_GRAPH: a repeated device-memory pls_hip_fit replayed as one graph launch.
// Part of libpls_hip.so: included by pls_hip.hip (one translation unit), in the order given there.
//
// First occurrence of a call: eager (it also sizes every workspace); second: the same enqueue sequence under stream capture
// (nothing allocates any more), instantiated and launched; from the third on: hipGraphLaunch.  The kernel arguments are baked
// into the graph, so the key is everything they derive from.  pls_hip_fit calls fit_graph_begin, then (unless replayed) the
// A-loop, then fit_graph_end.
#pragma once

namespace {

struct FitGraph {
    bool graphable = false, capture = false, replayed = false;
    std::vector<uint64_t> key;
};

// Builds the key of the call and decides: replayed (the stored graph has been launched, the call is done), capture (the stream
// now captures what the caller enqueues) or neither (eager).
// (a DUAL fit is never captured: it simply runs; the legacy default stream cannot be captured)
int fit_graph_begin(pls_hip_context *h, FitGraph &g, const void *X, i64 ldx, const void *Y, i64 ldy, i64 N, i64 K, i64 M, i64 A,
                    int method, int dtype, int mem, const double *W, const double *P, const double *Q, const double *R, const void *T,
                    i64 ldt, const double *B, bool dual) {
    g.graphable = h->opt_graph && mem == PLS_HIP_MEM_DEVICE && !h->reducer && h->opt_profile == 0 && !h->user_red &&
                  h->stream != nullptr && !dual;
    if (!g.graphable) return PLS_HIP_OK;
    g.key = {(uint64_t)(uintptr_t)X, (uint64_t)ldx, (uint64_t)(uintptr_t)Y, (uint64_t)ldy, (uint64_t)N, (uint64_t)K, (uint64_t)M,
             (uint64_t)A, (uint64_t)method, (uint64_t)dtype, (uint64_t)(uintptr_t)W, (uint64_t)(uintptr_t)P, (uint64_t)(uintptr_t)Q,
             (uint64_t)(uintptr_t)R, (uint64_t)(uintptr_t)T, (uint64_t)ldt, (uint64_t)(uintptr_t)B, (uint64_t)h->opt_algo,
             (uint64_t)h->opt_fuse, (uint64_t)h->opt_power_iters, (uint64_t)h->opt_fused_grid, (uint64_t)h->opt_work_layout,
             (uint64_t)h->opt_defer, (uint64_t)(uintptr_t)h->stream, (uint64_t)(uintptr_t)h->pre_xx, (uint64_t)(uintptr_t)h->pre_xy};
    if (h->graph_exec && g.key == h->graph_key) {
        HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));
        g.replayed = true;
        return PLS_HIP_OK;
    }
    g.capture = g.key == h->graph_seen;
    if (g.capture) {
        if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; h->graph_key.clear(); }
        HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    }
    return PLS_HIP_OK;
}

// Behind the A-loop, rc its status: ends a capture, instantiates the graph and launches it (this call's work); an eager graphable
// call is remembered, so that its repetition is captured.  Returns the status of the call so far.
int fit_graph_end(pls_hip_context *h, FitGraph &g, int rc) {
    if (g.capture) {
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(h->stream, &graph);
        if (rc == PLS_HIP_OK && ce == hipSuccess && graph && hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            h->graph_key = g.key;
            (void)hipGraphDestroy(graph);
            HIPCHK(h, hipGraphLaunch(h->graph_exec, h->stream));
        } else {
            if (graph) (void)hipGraphDestroy(graph);
            h->graph_exec = nullptr;
            h->graph_seen.clear();
            (void)hipGetLastError();
            if (rc != PLS_HIP_OK) return rc;
            return fail(h, PLS_HIP_ERR_DEVICE, "stream capture of the fit failed");
        }
    } else if (g.graphable) {
        h->graph_seen = g.key;
    }
    return rc;
}

}  // namespace
