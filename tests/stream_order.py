"""Stream order: what "the call only enqueues work on the handle's stream" promises (include/pls_hip.h, "Stream order").

  1. no input is read before the work already queued on the handle's stream has run;
  2. every output is complete for whatever is queued behind the call on that stream;
  3. an *enqueues* call does not wait for the device.

THE SANDWICH holds one library call to all three.  Everything runs on ONE non-blocking torch.cuda.Stream `s`, the handle created
with stream = s.cuda_stream:

    live inputs = decoy, outputs = NaN, synchronise; then, with no synchronisation in between,
        torch.cuda._sleep(window) | event `opened` | live <- true | THE CALL | event `closed` | snap <- outputs | live <- decoy |
        outputs <- another pattern
    opened.query() right after the call returns; only then s.synchronize().

`snap` must hold the bits of the synchronous baseline on `true` (SHA-256 over every output).  A call that reads an input before
the stream reaches it sees `decoy` (or writes from the wrong stream and is overwritten by the trailing fill); one that writes
late leaves NaN or the trailing pattern in `snap`.  The two baselines (true, decoy) must differ in every output, or the case could
not notice.  `opened.query()` is also read just BEFORE the call: the stream was still held when the call was made, for every
case.  For a case marked *enqueues* on a warm handle it must still be False when the call returns.

A CASE is one call of one entry point on one route: fixed shapes, the handle kind (environment at pls_hip_create and options),
a generator of its inputs from a seed, its output buffers, `call(h, live, out, seed)` -- one library call through ctypes with no
transfer and no synchronisation of its own -- and the launch counts (profile level 2) that show the route.  Every case calls
pls_amd._lib directly: the Handle methods allocate their outputs, and the sandwich needs the same output buffers for every run
(the header lets the bits depend on pointer alignment).  The Python wrappers have a test of their own.

The catalogue (CASES) is built without a GPU: tests/test_stream_order_cover.py holds it to the header's table."""
import contextlib
import ctypes
import hashlib
import os
import time
import zlib
from dataclasses import dataclass, field

import numpy as np

ENQUEUES, COMPLETES = "enqueues", "completes"
MIN_WINDOW_MS = 20.0
WINDOW_FACTOR = 20.0


def _torch():
    import torch
    return torch


def _pls():
    import pls_amd
    return pls_amd


# ---- handles ---------------------------------------------------------------------------------------------------------------------
# kind -> (environment at pls_hip_create, options): tools/history_probe.py KINDS, and the switches the routes below need
def _kinds():
    L = _pls()._lib
    gen = {"PLS_HIP_TINY": 0, "PLS_HIP_RESIDENT": 0}
    return {
        "default": ({}, {}),
        "default-auto": ({}, {L.OPT_ALGO: L.ALGO_AUTO}),
        "default-rounds": ({"PLS_HIP_BATCH_ROUND": 1}, {}),
        "general": (gen, {}),
        "general-nipals": (gen, {L.OPT_ALGO: L.ALGO_NIPALS}),
        "general-gram": (gen, {L.OPT_ALGO: L.ALGO_GRAM}),
        "general-unfused": (gen, {L.OPT_FUSE: 0}),
        "general-defer3": (gen, {L.OPT_DEFER: 3}),
        "general-layout0": (gen, {L.OPT_WORK_LAYOUT: 0}),
        "general-graph": (gen, {L.OPT_GRAPH: 1}),
        "radix": ({}, {L.OPT_VALIDATION_LDS_ROWS: 0}),
        "cv-refit": ({"PLS_HIP_TINY": 0, "PLS_HIP_CV_REFIT": 1}, {}),
        "dual": ({}, {L.OPT_ALGO: L.ALGO_DUAL}),
        "dual-refit": ({"PLS_HIP_CVBATCH_REFIT": 1}, {L.OPT_ALGO: L.ALGO_DUAL}),
        "xdiagmiss-stream": ({"PLS_HIP_XDIAGMISS_ROUTE": "stream"}, {}),
        "misscv-round1": ({"PLS_HIP_MISSCV_ROUND": 1}, {}),
    }


KIND_NAMES = ("default", "default-auto", "default-rounds", "general", "general-nipals", "general-gram", "general-unfused", "general-defer3",
              "general-layout0", "general-graph", "radix", "cv-refit", "dual", "dual-refit", "xdiagmiss-stream", "misscv-round1")


def make_handle(kind, stream, profile=0):
    """a pls_amd.Handle of `kind` on `stream` (a torch stream)"""
    pls_amd = _pls()
    env, opts = _kinds()[kind]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        h = pls_amd.Handle(stream=stream.cuda_stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    for o, v in opts.items():
        h.set_option(o, v)
    h.set_option(pls_amd.OPT_PROFILE, profile)
    return h


def digest(out):
    """SHA-256 over every output: name, dtype, shape and bytes (as tools/history_probe.py digest)"""
    s = hashlib.sha256()
    for k in sorted(out):
        a = np.ascontiguousarray(out[k].cpu().numpy())
        s.update(f"{k}:{a.dtype}:{a.shape}".encode())
        s.update(a.tobytes())
    return s.hexdigest()


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).tobytes()


# ---- the window --------------------------------------------------------------------------------------------------------------------
class Window:
    """torch.cuda._sleep counts device clock ticks of a rate nobody here has measured: timed once per session with two events"""
    _rate = None   # ticks per millisecond

    @classmethod
    def rate(cls):
        if cls._rate is None:
            torch = _torch()
            s = torch.cuda.current_stream()
            c0 = 20_000_000
            torch.cuda._sleep(1000); s.synchronize()   # (the kernel's first launch loads its code object)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); torch.cuda._sleep(c0); e1.record(s); s.synchronize()
            ms = e0.elapsed_time(e1)
            assert ms > 0.5, f"_sleep({c0}) took {ms} ms: too short to scale from"
            cls._rate = c0 / ms
            print(f"stream_order: torch.cuda._sleep runs at {cls._rate:.0f} ticks/ms ({c0} ticks in {ms:.2f} ms)", flush=True)
        return cls._rate

    largest_ms = 0.0

    @classmethod
    def ms_for(cls, host_ms):
        w = max(MIN_WINDOW_MS, WINDOW_FACTOR * host_ms)
        cls.largest_ms = max(cls.largest_ms, w)
        return w

    @classmethod
    def hold(cls, ms):
        """one thread spinning for a bounded count on the current stream"""
        _torch().cuda._sleep(int(ms * cls.rate()))


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def like(t):
    """an uninitialised tensor with the shape, strides, dtype and offset into its allocation (the alignment) of t, in an allocation
    of its own"""
    torch = _torch()
    off = int(t.storage_offset())
    span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) if t.numel() else 1
    flat = torch.empty(off + span + 8, dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()), off)


def scribble(t, which):
    """NaN (which = 0) or a finite pattern (which = 1) into every cell of an output; integers: -7 or 0x5A5A5A5A"""
    if t.dtype.is_floating_point:
        t.fill_(float("nan") if which == 0 else -1.25e300 if t.element_size() == 8 else -1.25e30)
    else:
        t.fill_(-7 if which == 0 else 0x5A5A5A5A)


def placed(rows, cols, dtype, ld_extra=0, off=0):
    """(rows, cols) column-major view with ld = rows + ld_extra, `off` elements into its allocation (tests/test_gpu_edge.py _place)"""
    torch = _torch()
    ld = rows + ld_extra
    flat = torch.empty(cols * ld + off + 8, dtype=dtype, device="cuda")
    return flat[off:off + cols * ld].view(cols, ld)[:, :rows].t()


def cm(rows, cols, dtype=None, ld=None):
    return _pls().colmajor_empty(rows, cols, dtype or _torch().float64, "cuda", ld=ld)


def normal(seed, key, *shape):
    """seeded standard-normal fp64 values on the device; two dimensions: column-major, packed"""
    torch = _torch()
    a = np.random.default_rng(zlib.crc32(f"{key}:{seed}".encode())).standard_normal(shape)
    t = torch.from_numpy(np.ascontiguousarray(a))
    if len(shape) == 2:
        return cm(shape[0], shape[1], ld=shape[0]).copy_(t)
    return t.cuda()


def p(t):
    return None if t is None else t.data_ptr()


def ld(t):
    return max(int(t.stride(1)) if t.shape[1] > 1 else 0, int(t.shape[0]), 1)


def dt_of(t):
    L = _pls()._lib
    return L.F64 if t.dtype == _torch().float64 else L.F32


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    entry: str            # the C symbol
    row: str              # the row of the header's table the case answers to
    route: str
    kind: str
    mark: str             # ENQUEUES / COMPLETES: copied from the header's table by hand, held to it by the cover test
    f32: bool
    gen: object           # gen(util, seed) -> dict of input tensors
    outs: object          # outs(inputs) -> dict of output tensors (may name a live input: in place)
    call: object          # call(h, live, out, seed) -> status
    shows: object         # shows(launches) -> None, asserting the route
    group: str = ""       # the test function's parameter
    idx: object = None    # idx(seed) -> host index array (cross-validation entries)
    repeat: int = 1       # OPT_GRAPH: the sandwich for the eager, the capturing and the replayed call
    extra: dict = field(default_factory=dict)


CASES = []


def add(name, entry, route, kind, mark, gen, outs, call, shows, f32=False, row=None, group=None, **kw):
    assert kind in KIND_NAMES and mark in (ENQUEUES, COMPLETES), (name, kind, mark)
    CASES.append(Case(name + (" f32" if f32 else ""), entry, row or entry, route, kind, mark, f32, gen, outs, call, shows,
                      group or entry, **kw))


def _lib():
    return _pls()._lib.lib()


def _dt(f32):
    torch = _torch()
    return torch.float32 if f32 else torch.float64


def gen_xy(N, K, M, f32=False, place=(0, 0)):
    def gen(u, seed):
        X, Y = u.synth_x(0, N, K, seed, dtype=_dt(f32)), u.synth_y(0, N, M, seed, dtype=_dt(f32))
        if place != (0, 0):
            X = placed(N, K, X.dtype, *place).copy_(X)
            Y = placed(N, M, Y.dtype, *place).copy_(Y)
        return {"X": X, "Y": Y}
    return gen


def with_nan(X, seed, frac=0.10):
    """NaN in a seeded tenth of the cells, no row or column emptied (the first cell of each stays)"""
    torch = _torch()
    N, K = X.shape
    m = np.random.default_rng(seed ^ 0x5EED).random((N, K)) < frac
    m[:, 0] = False
    m[0, :] = False
    X[torch.from_numpy(m).cuda()] = float("nan")
    return X


# ---- pls_hip_fit
def _fit_case(name, route, kind, N, K, M, A, shows, f32=False, method=0, place=(0, 0), group="pls_hip_fit", repeat=1):
    def outs(i):
        f64 = _torch().float64
        o = {k: cm(K, A, f64, ld=K) for k in "WPR"}
        o["Q"] = cm(M, A, f64, ld=M)
        o["B"] = cm(K, M, f64, ld=K)
        if method == 0:
            o["T"] = placed(N, A, i["X"].dtype, *place) if place != (0, 0) else cm(N, A, i["X"].dtype)
        return o

    def call(h, i, o, seed):
        X, Y, T = i["X"], i["Y"], o.get("T")
        return _lib().pls_hip_fit(h.h, p(X), ld(X), p(Y), ld(Y), N, K, M, A, method, dt_of(X), 1, p(o["W"]), p(o["P"]), p(o["Q"]), p(o["R"]),
                                  p(T), ld(T) if T is not None else N, p(o["B"]))
    add(f"fit {name} {N}x{K} m{M} a{A}", "pls_hip_fit", route, kind, ENQUEUES, gen_xy(N, K, M, f32, place), outs, call, shows, f32=f32,
        group=group, repeat=repeat)


def _total(l):
    return sum(l.values())


def _one_launch(l):
    assert _total(l) == 1 and l["small"] == 1, l


def _fused(A):
    def f(l):
        assert _total(l) > 1 and l["fused"] + l["xb"] >= A and l["deflate"] == 0, l
    return f


def _nipals(A):
    def f(l):
        assert _total(l) > 1 and l["fused"] + l["deflate"] >= A - 1, l
    return f


def _gram(l):
    assert l["fused"] == 0 and l["deflate"] == 0 and l["xb"] <= 1 and l["xty"] >= 1, l


def _type2(l):
    assert l["fused"] == 0 and l["deflate"] == 0 and l["xb"] == 0 and l["xty"] >= 1, l


def _edge(N, K, A, nipals, unaligned):
    def f(l):   # tools/history_probe.py _edge_fit
        if K <= 1024:
            assert l["fused"] == A and l["xb"] == 0, l
            assert l["deflate"] == (1 if (not nipals and unaligned and A >= 4) else 0) and (nipals or l["xty"] == 0), l
        elif K <= 8192:
            assert l["fused"] == A and l["deflate"] == 1 and l["xty"] == 0, l
        else:
            assert l["fused"] == 0 and _total(l) > A, l
    return f


def _build_fit():
    g1, g2, g3, g4 = "pls_hip_fit: single launch", "pls_hip_fit: general", "pls_hip_fit: wide", "pls_hip_fit: options"
    for f32 in (False, True):
        _fit_case("single-launch", "one workgroup", "default", 60, 400, 2, 6, _one_launch, f32=f32, group=g1)
        _fit_case("resident", "resident, one response", "default", 1301, 48, 1, 6, _one_launch, f32=f32, group=g1)
        _fit_case("kernel-fused", "general fused KERNEL", "general", 1301, 48, 3, 6, _fused(6), f32=f32, group=g2)
        _fit_case("nipals", "general NIPALS", "general-nipals", 1301, 48, 3, 6, _nipals(6), f32=f32, group=g2)
        _fit_case("gram", "GRAM: matrix-core SYRK", "general-gram", 2051, 513, 3, 5, _gram, f32=f32, group=g2)
        _fit_case("dual", "DUAL: sample space", "dual", 60, 400, 2, 6, _type2, f32=f32, group=g2)
    _fit_case("micro", "one wave", "default", 40, 12, 1, 4, _one_launch, group=g1)
    _fit_case("single-launch", "one workgroup, one response", "default", 60, 400, 1, 6, _one_launch, group=g1)
    _fit_case("resident", "resident, several responses", "default", 1301, 48, 3, 6, _one_launch, group=g1)
    _fit_case("resident-auto", "resident X^T X, one response", "default-auto", 1301, 48, 1, 6, _one_launch, group=g1)
    _fit_case("resident-auto", "resident X^T X, several responses", "default-auto", 1301, 48, 3, 6, _one_launch, group=g1)
    _fit_case("type2", "KERNEL_TYPE2", "general", 1301, 48, 3, 6, _type2, method=1, group=g2)
    _fit_case("dual", "DUAL: sample space, wide", "dual", 200, 5000, 3, 5, _type2, group=g2)
    for N, K, M, A, lde, off, what in ((515, 1500, 2, 5, 0, 0, "short tiles"), (261, 5000, 1, 4, 0, 0, "row-pack tiles"),
                                       (75, 9000, 1, 4, 0, 0, "one-product kernels"), (100, 20000, 5, 4, 0, 0, "beyond the cooperative update"),
                                       (1001, 37, 2, 6, 0, 1, "copy into aligned tiles")):
        _fit_case("kernel", "kernel: " + what, "general", N, K, M, A, _edge(N, K, A, False, off % 2 != 0), place=(lde, off), group=g3)
    _fit_case("nipals", "nipals: short tiles", "general-nipals", 515, 1500, 2, 5, _edge(515, 1500, 5, True, False), group=g3)
    _fit_case("unfused", "OPT_FUSE = 0", "general-unfused", 1301, 48, 3, 6,
              lambda l: _check(l["fused"] == 0 and l["xb"] >= 6 and l["deflate"] == 0, l), group=g4)
    _fit_case("defer3", "OPT_DEFER = 3", "general-defer3", 1301, 48, 3, 6, _fused(6), group=g4)
    _fit_case("layout0", "OPT_WORK_LAYOUT = 0", "general-layout0", 1301, 48, 3, 6, _fused(6), group=g4)
    _fit_case("m40", "M-sized work in global memory", "general", 1301, 48, 40, 6, _fused(6), group=g4)
    # OPT_GRAPH = 1: the baseline handle profiles (a profiled fit is never captured: it shows the eager route); the sandwich runs
    # three times on the same pointers -- eager, capturing, replayed
    _fit_case("graph", "OPT_GRAPH: eager, capturing, replayed", "general-graph", 3000, 96, 2, 5, _fused(5), group=g4, repeat=3)


# ---- steps and utilities
def _some(l):
    assert _total(l) >= 1, l


def _fam(name):
    def f(l):
        assert l[name] >= 1, l
    return f


def _build_steps():
    f64 = None
    for N, K in ((1001, 37), (130, 6000)):
        for C in (1, 3, 7, 45):
            for f32 in ((False, True) if (N, C) == (1001, 3) else (False,)):
                def gen(u, seed, N=N, K=K, C=C, f32=f32):
                    return {"X": u.synth_x(0, N, K, seed, dtype=_dt(f32)), "Bm": normal(seed, "xbB", K, C)}

                def call(h, i, o, seed, N=N, K=K, C=C):
                    return _lib().pls_hip_xb(h.h, p(i["X"]), ld(i["X"]), N, K, p(i["Bm"]), K, C, dt_of(i["X"]), 1, p(o["XB"]), ld(o["XB"]))
                add(f"xb {N}x{K} c{C}", "pls_hip_xb", "X B", "default", ENQUEUES, gen, lambda i, N=N, C=C: {"XB": cm(N, C, i["X"].dtype)}, call,
                    _fam("xb"), f32=f32)
    N, K, M, A = 1001, 37, 2, 6
    for f32 in (False, True):
        def call_xty(h, i, o, seed):
            return _lib().pls_hip_xty(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, dt_of(i["X"]), p(o["XY"]))
        add("xty 1001x37 m2", "pls_hip_xty", "X^T Y", "default", ENQUEUES, gen_xy(N, K, M, f32), lambda i: {"XY": cm(K, M, f64, ld=K)}, call_xty,
            _fam("xty"), f32=f32)

        def gen_defl(u, seed, f32=f32):
            return {"X": u.synth_x(0, N, K, seed, dtype=_dt(f32)), "t": normal(seed, "deflt", N).to(_dt(f32)), "pv": normal(seed, "deflp", K)}
        for inplace in (False, True):
            def call_defl(h, i, o, seed):
                return _lib().pls_hip_deflate(h.h, p(i["X"]), ld(i["X"]), p(o["D"]), ld(o["D"]), N, K, p(i["t"]), p(i["pv"]), dt_of(i["X"]))
            add("deflate 1001x37" + (" in place" if inplace else ""), "pls_hip_deflate", "in place" if inplace else "out of place", "default",
                ENQUEUES, gen_defl, (lambda i: {"D": i["X"]}) if inplace else (lambda i: {"D": like(i["X"])}), call_defl, _fam("deflate"), f32=f32)

            def call_z(h, i, o, seed):
                return _lib().pls_hip_colwise_z_scores(h.h, p(i["X"]), ld(i["X"]), N, N, K, dt_of(i["X"]), p(o["Z"]), ld(o["Z"]), p(o["mean"]),
                                                       p(o["sd"]))

            def outs_z(i, inplace=inplace):
                torch = _torch()
                return {"Z": i["X"] if inplace else like(i["X"]), "mean": torch.empty(K, dtype=torch.float64, device="cuda"),
                        "sd": torch.empty(K, dtype=torch.float64, device="cuda")}
            add("colwise_z_scores 1001x37" + (" in place" if inplace else ""), "pls_hip_colwise_z_scores", "in place" if inplace else "out of place",
                "default", ENQUEUES, lambda u, seed, f32=f32: {"X": u.synth_x(0, N, K, seed, dtype=_dt(f32))}, outs_z, call_z, _some, f32=f32)

        def gen_sse(u, seed, f32=f32):
            S = normal(seed, "sseS", N, A)
            return {"S": cm(N, A, _dt(f32)).copy_(S), "Y": u.synth_y(0, N, M, seed, dtype=_dt(f32)), "Q": normal(seed, "sseQ", M, A)}

        def call_sse(h, i, o, seed):
            return _lib().pls_hip_sse_by_components(h.h, p(i["S"]), ld(i["S"]), p(i["Y"]), ld(i["Y"]), N, A, M, p(i["Q"]), dt_of(i["S"]), p(o["SSE"]))
        add("sse_by_components 1001 a6 m2", "pls_hip_sse_by_components", "one sweep", "default", ENQUEUES, gen_sse,
            lambda i: {"SSE": cm(M, A, f64, ld=M)}, call_sse, _some, f32=f32)

        def gen_msse(u, seed, f32=f32):
            d = gen_xy(N, K, M, f32)(u, seed)
            d.update(R=normal(seed, "msR", K, A), Q=normal(seed, "msQ", M, A))
            return d

        def call_msse(h, i, o, seed):
            return _lib().pls_hip_model_sse(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, p(i["R"]), p(i["Q"]), dt_of(i["X"]), 1,
                                            p(o["SSE"]))
        add("model_sse 1001x37 m2 a6", "pls_hip_model_sse", "X R, then one sweep", "default", ENQUEUES, gen_msse,
            lambda i: {"SSE": cm(M, A, f64, ld=M)}, call_msse, _fam("xb"), f32=f32)

        for new_rows in (False, True):
            if f32 and new_rows:
                continue

            def gen_xd(u, seed, f32=f32, new_rows=new_rows):
                d = {"X": u.synth_x(0, N, K, seed, dtype=_dt(f32)), "R": normal(seed, "xdR", K, A), "P": normal(seed, "xdP", K, A)}
                if new_rows:
                    d["tvar"] = normal(seed, "xdtv", A).abs_().add_(1.0)
                return d

            def outs_xd(i):
                torch = _torch()
                return {"Q": cm(N, A), "T2": cm(N, A), "S": cm(N, A, i["X"].dtype), "ssx": torch.empty(A + 1, dtype=torch.float64, device="cuda"),
                        "sst": torch.empty(A, dtype=torch.float64, device="cuda")}

            def call_xd(h, i, o, seed):
                return _lib().pls_hip_x_diagnostics(h.h, p(i["X"]), ld(i["X"]), N, N, K, A, p(i["R"]), p(i["P"]), p(i.get("tvar")), dt_of(i["X"]), 1,
                                                    p(o["Q"]), ld(o["Q"]), p(o["T2"]), ld(o["T2"]), p(o["S"]), ld(o["S"]), p(o["ssx"]), p(o["sst"]))
            add("x_diagnostics 1001x37 a6 " + ("new rows, device tvar" if new_rows else "training rows"), "pls_hip_x_diagnostics", "one sweep",
                "default", ENQUEUES, gen_xd, outs_xd, call_xd, _some, f32=f32)

    def gen_co(u, seed):
        return {"R": normal(seed, "coR", K, A), "Q": normal(seed, "coQ", M, A)}
    add("coefficients 37x6 m2 c4", "pls_hip_coefficients", "one launch", "default", ENQUEUES, gen_co, lambda i: {"B": cm(K, M, f64, ld=K)},
        lambda h, i, o, seed: _lib().pls_hip_coefficients(h.h, p(i["R"]), p(i["Q"]), K, M, A, 4, 1, p(o["B"])), lambda l: None)

    # validation: E is (M, A, nobs) contiguous; the smallest PRESS of response m sits in column (seed + m) % A, so that `ref`
    # differs between the two data sets as surely as the sums do
    VM, VA, VN = 2, 5, 1001

    def gen_val(u, seed):
        torch = _torch()
        a = np.random.default_rng(zlib.crc32(f"valE:{seed}".encode())).standard_normal((VM, VA, VN))
        for m in range(VM):
            a[m, (seed + m) % VA] *= 0.5
        return {"E": torch.from_numpy(a).cuda()}

    def outs_val(i):
        torch = _torch()
        o = {k: cm(VM, VA, ld=VM) for k in ("press", "D", "probw")}
        o["ref"] = torch.empty(VM, dtype=torch.int64, device="cuda")
        return o

    def call_val(h, i, o, seed):
        return _lib().pls_hip_validation(h.h, p(i["E"]), VN, VA, VM, 1, p(o["press"]), p(o["D"]), p(o["probw"]), p(o["ref"]))
    add("validation m2 a5 nobs1001 LDS", "pls_hip_validation", "one workgroup per pair", "default", ENQUEUES, gen_val, outs_val, call_val,
        lambda l: _check(l["small"] <= 3 and _total(l) >= 1, l))
    add("validation m2 a5 nobs1001 radix", "pls_hip_validation", "radix sort (OPT_VALIDATION_LDS_ROWS = 0)", "radix", ENQUEUES, gen_val, outs_val,
        call_val, lambda l: _check(l["small"] >= 8, l))

    for which, cols in (("x", 37), ("y", 3)):
        for f32 in (False, True):
            def call_syn(h, i, o, seed, which=which, cols=cols):
                fn = getattr(_lib(), "pls_hip_synth_" + which)
                return fn(h.h, p(o["out"]), ld(o["out"]), 5, 1001, cols, seed, dt_of(o["out"]))
            add(f"synth_{which} 1001x{cols}", "pls_hip_synth_" + which, "generator", "default", ENQUEUES, lambda u, seed: {},
                lambda i, cols=cols, f32=f32: {"out": cm(1001, cols, _dt(f32))}, call_syn, lambda l: None, f32=f32)


def _check(ok, l):
    assert ok, l


# ---- batched entries
def cv_idx(N, nf, ts, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(N)[:nf * ts].reshape(nf, ts).astype(np.int64))


def _idx_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _build_batched():
    f64 = None

    def batch(name, route, kind, N, K, M, A, nprob, shows, f32=False):
        def outs(i):
            torch = _torch()
            e = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
            return {"R": e(nprob, A, K), "Q": e(nprob, A, M), "tt": e(nprob, A), "B": e(nprob, M, K), "ssy": e(nprob, M)}

        def call(h, i, o, seed):
            return _lib().pls_hip_fit_batch(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, nprob, dt_of(i["X"]), 1,
                                            p(o["R"]), p(o["Q"]), p(o["tt"]), p(o["B"]), p(o["ssy"]))
        add(f"fit_batch {name} {N}x{K} m{M} x{nprob}", "pls_hip_fit_batch", route, kind, ENQUEUES, gen_xy(N, K, M * nprob, f32), outs, call, shows, f32=f32)
    is_batch = lambda l: _check(l["fused"] + l["xb"] + l["deflate"] == 0 and l["xty"] >= 1 and l["small"] >= 1, l)
    for f32 in (False, True):
        batch("batched", "batched on the shared X^T X", "default", 1301, 48, 1, 6, 3, is_batch, f32=f32)
        batch("dual", "DUAL: every problem from one X X^T", "dual", 60, 400, 2, 6, 3, _type2, f32=f32)
    batch("rounds", "batched, PLS_HIP_BATCH_ROUND = 1 (three rounds)", "default-rounds", 1301, 48, 1, 6, 3,
          lambda l: _check(l["fused"] + l["xb"] + l["deflate"] == 0 and l["xty"] >= 1 and l["small"] >= 3, l))

    def resampled(route, kind, N, K, M, A, nrep, shows, f32=False):
        def gen(u, seed):
            torch = _torch()
            d = gen_xy(N, K, M, f32)(u, seed)
            d["Wt"] = cm(N, nrep, ld=N).copy_(torch.from_numpy(np.ascontiguousarray(_pls().bootstrap_weights(N, nrep, seed))))
            return d

        def outs(i):
            torch = _torch()
            e = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
            return {"Q": e(nrep, A, M), "tt": e(nrep, A), "B": e(nrep, M, K), "B0": e(M, K), "Bmean": e(M, K), "Bm2": e(M, K)}

        def call(h, i, o, seed):
            return _lib().pls_hip_fit_resampled(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, p(i["Wt"]), N, nrep, dt_of(i["X"]), 1,
                                                *[p(o[k]) for k in ("Q", "tt", "B", "B0", "Bmean", "Bm2")])
        add(f"fit_resampled {N}x{K} m{M} a{A} x{nrep}", "pls_hip_fit_resampled", route, kind, ENQUEUES, gen, outs, call, shows, f32=f32)
    for f32 in (False, True):
        resampled("DUAL: sample space", "dual", 60, 400, 2, 5, 7,
                  lambda l: _check(l["fused"] + l["xb"] + l["deflate"] == 0 and 1 <= l["xty"] <= 3, l), f32=f32)
    resampled("one refit per replicate", "general", 300, 40, 2, 5, 5, lambda l: _check(l["fused"] + l["xb"] + l["deflate"] >= 5, l))

    def cvb(route, kind, shows, f32=False):
        N, K, M, A, nprob, nf, ts = 60, 400, 2, 4, 3, 6, 5

        def outs(i):
            torch = _torch()
            e = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
            return {"PRESS": e(nprob, A, M), "ssy": e(nprob, M), "E": e(nprob, M, A, nf * ts)}

        def call(h, i, o, seed, idx=None):
            idx = cv_idx(N, nf, ts, 6) if idx is None else idx
            return _lib().pls_hip_cv_press_batch(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, nprob, _idx_ptr(idx), ts, nf,
                                                 dt_of(i["X"]), 1, p(o["PRESS"]), p(o["ssy"]), p(o["E"]))
        add("cv_press_batch 60x400 m2 a4 x3: " + route, "pls_hip_cv_press_batch", route, kind, COMPLETES, gen_xy(N, K, M * nprob, f32), outs, call,
            shows, f32=f32, idx=lambda seed: cv_idx(N, nf, ts, seed))
    for f32 in (False, True):
        cvb("DUAL: sample space", "dual", lambda l: _check(l["xb"] + l["deflate"] + l["fused"] == 0 and l["xty"] == 1, l), f32=f32)
    cvb("PLS_HIP_CVBATCH_REFIT = 1", "dual-refit", lambda l: _check(l["xb"] + l["deflate"] + l["fused"] == 0 and l["xty"] >= 3, l))

    def cv(route, kind, N, K, M, A, nf, ts, shows, f32=False, missing=False):
        entry = "pls_hip_cv_folds_missing" if missing else "pls_hip_cv_folds"

        def gen(u, seed):
            d = gen_xy(N, K, M, f32)(u, seed)
            if missing:
                with_nan(d["X"], seed)
            return d

        def outs(i):
            torch = _torch()
            o = {"E": torch.empty((M, A, nf * ts), dtype=torch.float64, device="cuda")}
            if missing:
                o["iters"] = torch.empty((nf, A), dtype=torch.int64, device="cuda")
            return o

        def call(h, i, o, seed, idx=None):
            idx = cv_idx(N, nf, ts, 6) if idx is None else idx
            a = (h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, _idx_ptr(idx), ts, nf, dt_of(i["X"]), 1, p(o["E"]))
            return _lib().pls_hip_cv_folds_missing(*a, p(o["iters"])) if missing else _lib().pls_hip_cv_folds(*a)
        add(f"{entry[8:]} {N}x{K} m{M} a{A}: {route}", entry, route, kind, COMPLETES, gen, outs, call, shows, f32=f32,
            idx=lambda seed: cv_idx(N, nf, ts, seed))
    cv("one single-launch fit per fold", "default", 40, 12, 1, 4, 5, 4, lambda l: _check(_total(l) == 1 and l["small"] == 1, l))
    for f32 in (False, True):
        cv("batched on the shared X^T X", "general", 1301, 48, 3, 6, 3, 20,
           lambda l: _check(l["fused"] + l["xb"] + l["deflate"] == 0 and l["xty"] >= 1 and l["small"] >= 1, l), f32=f32)
    cv("one refit per fold (PLS_HIP_CV_REFIT = 1)", "cv-refit", 1301, 48, 3, 6, 3, 20, lambda l: _check(l["fused"] + l["xb"] + l["deflate"] >= 3, l))
    cv("DUAL: every fold from one X X^T", "dual", 60, 400, 2, 6, 3, 5, lambda l: _check(l["xty"] == 1 and l["fused"] + l["xb"] + l["deflate"] == 0, l))
    for f32 in (False, True):
        cv("one round", "default", 120, 30, 2, 3, 4, 6, _some, f32=f32, missing=True)
    cv("rounds of one fold (PLS_HIP_MISSCV_ROUND = 1)", "misscv-round1", 120, 30, 2, 3, 4, 6, _some, missing=True)


# ---- missing values
def _build_missing():
    f64 = None

    def fit_missing(M, mark, row, f32=False):
        N, K, A = 300, 40, 4

        def gen(u, seed):
            d = gen_xy(N, K, M, f32)(u, seed)
            with_nan(d["X"], seed)
            return d

        def outs(i):
            torch = _torch()
            o = {k: cm(K, A, f64, ld=K) for k in "WPR"}
            o.update(Q=cm(M, A, f64, ld=M), B=cm(K, M, f64, ld=K), T=cm(N, A, i["X"].dtype))
            if M > 1:   # (one response converges in its first iteration whatever the data: the counts could not differ)
                o["iters"] = torch.empty(A, dtype=torch.int64, device="cuda")
            return o

        def call(h, i, o, seed):
            return _lib().pls_hip_fit_missing(h.h, p(i["X"]), ld(i["X"]), p(i["Y"]), ld(i["Y"]), N, K, M, A, dt_of(i["X"]), 1, p(o["W"]), p(o["P"]),
                                              p(o["Q"]), p(o["R"]), p(o["T"]), ld(o["T"]), p(o["B"]), p(o.get("iters")))
        add(f"fit_missing 300x40 m{M} a4", "pls_hip_fit_missing", "one response" if M == 1 else "several responses: the host reads the convergence word",
            "default", mark, gen, outs, call, _some, f32=f32, row=row)
    for f32 in (False, True):
        fit_missing(1, ENQUEUES, "pls_hip_fit_missing, M = 1", f32=f32)
    fit_missing(2, COMPLETES, "pls_hip_fit_missing, M > 1")

    def gen_model(N, K, A, f32, tvar):
        def gen(u, seed):
            d = {"X": with_nan(u.synth_x(0, N, K, seed, dtype=_dt(f32)), seed), "W": normal(seed, "mW", K, A), "P": normal(seed, "mP", K, A)}
            if tvar:
                d["tvar"] = normal(seed, "mtv", A).abs_().add_(1.0)
            return d
        return gen
    for f32 in (False, True):
        N, K, A = 300, 40, 4

        def call_sm(h, i, o, seed, N=N, K=K, A=A):
            return _lib().pls_hip_scores_missing(h.h, p(i["X"]), ld(i["X"]), N, K, A, p(i["W"]), p(i["P"]), dt_of(i["X"]), 1, p(o["S"]), ld(o["S"]))
        add("scores_missing 300x40 a4", "pls_hip_scores_missing", "sequential deflation", "default", ENQUEUES, gen_model(N, K, A, f32, False),
            lambda i, N=N, A=A: {"S": cm(N, A, i["X"].dtype)}, call_sm, _some, f32=f32)

        def call_zm(h, i, o, seed, N=N, K=K):
            return _lib().pls_hip_colwise_z_scores_missing(h.h, p(i["X"]), ld(i["X"]), N, K, dt_of(i["X"]), 1, p(o["Z"]), ld(o["Z"]), p(o["mean"]),
                                                           p(o["sd"]), p(o["nobs"]))

        def outs_zm(i, K=K):
            torch = _torch()
            return {"Z": like(i["X"]), "mean": torch.empty(K, dtype=torch.float64, device="cuda"), "sd": torch.empty(K, dtype=torch.float64, device="cuda"),
                    "nobs": torch.empty(K, dtype=torch.int64, device="cuda")}
        add("colwise_z_scores_missing 300x40", "pls_hip_colwise_z_scores_missing", "observed cells", "default", ENQUEUES,
            lambda u, seed, f32=f32, N=N, K=K: {"X": with_nan(u.synth_x(0, N, K, seed, dtype=_dt(f32)), seed)}, outs_zm, call_zm, _some, f32=f32)

    XN, XK, XA = 2048, 24, 2

    def outs_xm(i):
        torch = _torch()
        e = lambda n, dt=torch.float64: torch.empty(n, dtype=dt, device="cuda")
        return {"Q": cm(XN, XA), "T2": cm(XN, XA), "S": cm(XN, XA, i["X"].dtype), "ssx": e(XA + 1), "sst": e(XA), "nobs": e(XN, torch.int64)}

    def call_xm(h, i, o, seed):
        return _lib().pls_hip_x_diagnostics_missing(h.h, p(i["X"]), ld(i["X"]), XN, XK, XA, p(i["W"]), p(i["P"]), p(i["tvar"]), dt_of(i["X"]), 1,
                                                    p(o["Q"]), ld(o["Q"]), p(o["T2"]), ld(o["T2"]), p(o["S"]), ld(o["S"]), p(o["ssx"]), p(o["sst"]),
                                                    p(o["nobs"]))
    for f32 in (False, True):
        add("x_diagnostics_missing 2048x24 a2", "pls_hip_x_diagnostics_missing", "resident: one read of X", "default", ENQUEUES,
            gen_model(XN, XK, XA, f32, True), outs_xm, call_xm, lambda l: _check(l["xb"] == 1, l), f32=f32)
    add("x_diagnostics_missing 2048x24 a2 streaming", "pls_hip_x_diagnostics_missing", "PLS_HIP_XDIAGMISS_ROUTE = stream: A + 1 sweeps",
        "xdiagmiss-stream", ENQUEUES, gen_model(XN, XK, XA, False, True), outs_xm, call_xm, lambda l: _check(l["xb"] == XA + 1, l))


_build_fit()
_build_steps()
_build_batched()
_build_missing()
GROUPS = list(dict.fromkeys(c.group for c in CASES))


def by_name(name):
    hit = [c for c in CASES if c.name == name]
    assert len(hit) == 1, name
    return hit[0]


# ---- running a case ----------------------------------------------------------------------------------------------------------------
TRUE_SEED, DECOY_SEED = 101, 202


class Bench:
    """the stream, the handle that only generates inputs, and the staged inputs of the cases (made once, never written again)"""

    def __init__(self):
        torch = _torch()
        torch.cuda.set_device(0)
        self.s = torch.cuda.Stream()
        with torch.cuda.stream(self.s):
            self.util = _pls().Handle(stream=self.s.cuda_stream)
            Window.rate()
        self._staged = {}

    def close(self):
        self.s.synchronize()
        self.util.close()

    def staged(self, case):
        """(true, decoy): the case's inputs from the two seeds"""
        key = case.name
        if key not in self._staged:
            self._staged[key] = tuple(case.gen(self.util, seed) for seed in (TRUE_SEED, DECOY_SEED))
            self.util.synchronize()
            self.s.synchronize()
        return self._staged[key]


class Rig:
    """the live inputs and the outputs of one case, allocated once and reused by every run of it"""

    def __init__(self, bench, case, s=None):
        self.bench, self.case, self.s = bench, case, s or bench.s
        self.true, self.decoy = bench.staged(case)
        self.live = {k: like(v) for k, v in self.true.items()}
        self.out = case.outs(self.live)
        self.s.synchronize()

    def fill(self, src):
        for k, v in self.live.items():
            v.copy_(src[k])

    def baseline(self, h, which):
        """synchronous: fill, synchronise, call, synchronise -> (digest, bits per output, launch counts, host ms of the call)"""
        src, seed = (self.true, TRUE_SEED) if which == "true" else (self.decoy, DECOY_SEED)
        for v in self.out.values():
            scribble(v, 0)
        self.fill(src)
        self.s.synchronize()
        h.timing()
        t0 = time.perf_counter()
        rc = self.case.call(h, self.live, self.out, seed)
        host_ms = (time.perf_counter() - t0) * 1e3
        _pls()._lib.check(rc, h.h)
        h.synchronize()
        self.s.synchronize()
        return digest(self.out), {k: bits(v) for k, v in self.out.items()}, h.timing()["launches"], host_ms

    def queue(self, call, window_ms, hold=True, after=None):
        """everything of the sandwich that is queued, nothing synchronised: -> a dict the caller reads AFTER its own synchronisation.
        The caller has filled the live inputs with decoy and the outputs with NaN and synchronised (prepare()), and torch's current
        stream is the rig's.  hold=False: the caller holds the stream itself.  after(): queued behind the trailing fill."""
        torch = _torch()
        r = {"opened": torch.cuda.Event(), "closed": torch.cuda.Event(), "window_ms": window_ms}
        if hold:
            Window.hold(window_ms)
        r["opened"].record(self.s)
        self.fill(self.true)
        r["held_before"] = not r["opened"].query()
        t0 = time.perf_counter()
        r["rc"] = call()
        r["host_ms"] = (time.perf_counter() - t0) * 1e3
        r["held_after"] = not r["opened"].query()
        r["closed"].record(self.s)
        r["snap"] = {k: v.clone() for k, v in self.out.items()}
        self.fill(self.decoy)
        for v in self.out.values():
            scribble(v, 1)
        if after:
            after()
        return r

    def prepare(self):
        self.fill(self.decoy)
        for v in self.out.values():
            scribble(v, 0)
        self.s.synchronize()

    def sandwich(self, h, window_ms, call=None):
        self.prepare()
        r = self.queue(call or (lambda: self.case.call(h, self.live, self.out, TRUE_SEED)), window_ms)
        self.s.synchronize()
        return r


def judge(r, want_digest, what, asynchronous):
    """the verdict on one sandwich, as a list of failures (empty: passed)"""
    bad = []
    if r["rc"] != 0:
        bad.append(f"{what}: status {r['rc']}")
    if not r["held_before"]:
        bad.append(f"{what}: the window of {r['window_ms']:.1f} ms had closed before the call was made: nothing to judge")
    if digest(r["snap"]) != want_digest:
        worst = [k for k in sorted(r["snap"])]
        bad.append(f"{what}: the outputs snapshotted behind the call are not the baseline's bits (outputs {worst})")
    if asynchronous:
        if not r["held_after"]:
            bad.append(f"{what}: the call returned only after the stream had been released ({r['host_ms']:.2f} ms on the host, window "
                       f"{r['window_ms']:.1f} ms): it waited for the device")
        elif r["host_ms"] > 0.5 * r["window_ms"]:
            bad.append(f"{what}: the call took {r['host_ms']:.2f} ms on the host, more than half its window of {r['window_ms']:.1f} ms: "
                       "window too short to judge")
    return bad


def report(case, temp, r):
    print(f"  {case.name} [{case.kind}] route {case.route}; {case.mark}; {temp}; window {r['window_ms']:.1f} ms; host {r['host_ms']:.3f} ms; "
          f"returned with the stream held: {'yes' if r['held_after'] else 'no'}", flush=True)


def run_case(bench, case):
    """baselines, the warm sandwich(es) and the fresh-handle sandwich of one case -> list of failures"""
    torch = _torch()
    pls_amd = _pls()
    bad = []
    with torch.cuda.stream(bench.s):
        rig = Rig(bench, case)
        h = make_handle(case.kind, bench.s, profile=2)
        try:
            want, wbits, lau, host_ms = rig.baseline(h, "true")
            case.shows(lau)
            _, dbits, _, _ = rig.baseline(h, "decoy")
            for k in wbits:
                assert wbits[k] != dbits[k], f"{case.name}: output {k} has the same bits on both data sets: the case cannot notice an early read"
            again, _, _, host_ms = rig.baseline(h, "true")
            assert again == want, f"{case.name}: two synchronous calls on the same inputs differ"
            window = Window.ms_for(host_ms)
            if case.repeat == 1:
                h.set_option(pls_amd.OPT_PROFILE, 0)
                r = rig.sandwich(h, window)
                report(case, "warm", r)
                bad += judge(r, want, f"{case.name} (warm)", case.mark == ENQUEUES)
                bad += _sync_ok(h, case.name)
        finally:
            h.close()
        h = make_handle(case.kind, bench.s, profile=0)
        try:
            for n in range(case.repeat):
                r = rig.sandwich(h, window)
                temp = "fresh" if n == 0 else ("capturing" if n == 1 else "replayed")
                report(case, temp, r)
                # a fresh handle sizes its workspaces inside the window: the bits only.  OPT_GRAPH: the replayed call is the warm one
                bad += judge(r, want, f"{case.name} ({temp})", case.mark == ENQUEUES and n == 2)
                bad += _sync_ok(h, case.name)
        finally:
            h.close()
    return bad


def _sync_ok(h, what):
    rc = h._lib.pls_hip_synchronize(h.h)
    return [] if rc == 0 else [f"{what}: pls_hip_synchronize returned {rc}: {_pls()._lib.last_error(h.h)}"]


# ---- the header's table ------------------------------------------------------------------------------------------------------------
def header_table(text):
    """{row: (device mark, host mark)} from the "Stream order" paragraph of include/pls_hip.h"""
    import re
    start = text.index(" * Stream order:")
    rows = {}
    for line in text[start:text.index("*/", start)].splitlines():
        m = re.match(r"^ \*\s{3,}(pls_hip_[a-z_0-9]+(?:, M [=>] 1)?)\s{2,}(enqueues|completes|-)\s+(enqueues|completes|-)(?:\s|$)", line)
        if m:
            rows[m.group(1)] = (m.group(2), m.group(3))
    return rows
