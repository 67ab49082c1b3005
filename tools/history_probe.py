"""The bits a call returns are a function of its arguments, the handle's options and the environment at pls_hip_create -- not of
any earlier call on this handle or on another (include/pls_hip.h, "History").  This driver checks that, bit for bit, in one
process per group of handles (tests/test_gpu_history.py runs the four groups one after another):

    python tools/history_probe.py default|general|dual|host [--bytes ff,7f,01] [--orders fwd,rev]

It needs pls_amd/csrc/testing/libpls_hip.so (PLS_AMD_LIBRARY, read when pls_amd is imported) for
pls_hip_test_poison_workspace, which fills every scratch workspace of a handle -- and, while its switch is on, every workspace
allocated later -- with one byte value (pls_amd/csrc/ctx.hpp, PLS_HIP_WORKSPACES).

A PROBE is one call (or a few) of the library on fixed inputs from the seeded generator, on a handle of a given kind; it asserts
that the route it is named after was taken (the launch counters at profile level 2) and returns all its outputs, of which the
driver keeps the SHA-256, and the launch counts.
  a. baseline      every probe on a fresh handle of its kind: digest and launch counts are its reference
  b. poisoned      one long-lived handle per kind; before every probe all scratch is filled with 0xFF (NaN in both precisions,
                   -1 / huge as integers), then 0x7F (1.4e306: finite, survives comparisons that swallow NaN), then 0x01 (tiny
                   positive values, non-zero counts); the probes in catalogue order, then in reverse, so that each meets
                   workspaces sized by other predecessors.  Digest and launch counts must be the baseline's.
  c. host state    (group "host", no poison) options toggled and restored, the graph cache, X^T X taken during an upload, a
                   changed stream, refused calls, the resident fits' counters and epochs, two handles taking turns
Every probe is listed with its route, its baseline digest and the bytes poisoned before it; the last line is
"done: <group>: <probes> probes, <runs> runs, <n> differ".  Exit status 1 when anything differs."""
import argparse
import contextlib
import ctypes
import hashlib
import zlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import pls_amd
from pls_amd import _lib as L
from oracle import pls_oracle as po
import hard_data as hd
from test_gpu_hard_data import FIT_ROUTES, F32_ROUTES, run_fit, run_batch, run_cv, _launch_check
from test_gpu_edge import _place

# ---- handles -------------------------------------------------------------------------------------------------------------------
# kind -> (environment at pls_hip_create, OPT_ALGO, the key run_fit / run_batch / run_cv know the handle by)
KINDS = {
    "default": ({}, pls_amd.ALGO_KERNEL, "default"),
    "default-rounds": ({"PLS_HIP_BATCH_ROUND": 1}, pls_amd.ALGO_KERNEL, "default"),
    "general": ({"PLS_HIP_TINY": 0}, pls_amd.ALGO_KERNEL, "general"),
    "dual": ({}, pls_amd.ALGO_DUAL, "dual"),
    "dual-refit": ({"PLS_HIP_CVBATCH_REFIT": 1}, pls_amd.ALGO_DUAL, "dual"),
}
GROUPS = {"default": ("default", "default-rounds"), "general": ("general",), "dual": ("dual", "dual-refit"), "host": ()}


def make_handle(kind, stream=None):
    env, algo, _ = KINDS[kind]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        h = pls_amd.Handle(stream=stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    h.set_option(pls_amd.OPT_ALGO, algo)
    h.set_option(pls_amd.OPT_PROFILE, 2)
    h.kind = kind
    return h


@contextlib.contextmanager
def fresh(kind, stream=None):
    h = make_handle(kind, stream)
    try:
        yield h
    finally:
        h.close()


def as_handles(h):
    return {KINDS[h.kind][2]: h}


_poison = None


def poison(h, byte, also_new=1):
    global _poison
    if _poison is None:
        _poison = L.lib().pls_hip_test_poison_workspace   # (AttributeError: not the testing build)
        _poison.restype = ctypes.c_longlong
        _poison.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    n = int(_poison(h.h, byte, also_new))
    assert n >= 0, "pls_hip_test_poison_workspace failed"
    return n


def counted(h, f):
    """f() with the launches it made, by kernel family"""
    h.timing()
    out = f()
    h.synchronize()
    return out, h.timing()["launches"]


def digest(out):
    s = hashlib.sha256()
    for k in sorted(out):
        v = out[k]
        if v is None:
            s.update(f"{k}:none".encode())
            continue
        a = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v))
        s.update(f"{k}:{a.dtype}:{a.shape}".encode())
        s.update(a.tobytes())
    return s.hexdigest()


# ---- inputs: made once, by a handle that runs no probe ----------------------------------------------------------------------------
_cache = {}
_util = None


def util():
    global _util
    if _util is None:
        _util = pls_amd.Handle()
    return _util


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        util().synchronize()
    return _cache[key]


def hard(N, K, M, f32=False):
    """family `plain` of tests/hard_data.py"""
    return cached(("hard", N, K, M, f32), lambda: hd.hard_inputs(po, "plain", N, K, M, f32=f32))


def synth(N, K, M, seed, f32=False):
    dt = torch.float32 if f32 else torch.float64
    return cached(("synth", N, K, M, seed, f32), lambda: (util().synth_x(0, N, K, seed, dtype=dt), util().synth_y(0, N, M, seed, dtype=dt)))


def host(N, K, M, seed):
    X, Y = synth(N, K, M, seed)
    return cached(("host", N, K, M, seed), lambda: (np.asfortranarray(X.cpu().numpy()), np.asfortranarray(Y.cpu().numpy())))


def normal(key, *shape):
    """seeded standard-normal values on the device, column-major"""
    def make():
        a = np.random.default_rng(zlib.crc32(str(key).encode())).standard_normal(shape)
        return pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(a)).cuda()) if len(shape) == 2 else torch.from_numpy(a).cuda()
    return cached(("normal", key) + shape, make)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
PROBES = []   # (name, kind, route, fn): fn(h) -> (dict of outputs, launch counts)


def probe(name, kind, route):
    def deco(fn):
        PROBES.append((name, kind, route, fn))
        return fn
    return deco


# 1. the fit routes of tests/test_gpu_hard_data.py on its four shapes, fp32 storage for three of them
ROUTE_KIND = {"default": "default", "general": "general", "dual": "dual"}
OTHER_KIND = {"batch": "default", "batch-dual": "dual", "cv": "general", "cv-dual": "dual"}


def _fit_route(route, N, K, M, f32):
    def fn(h):
        X, Y = hard(N, K, M, f32)
        out, lau = run_fit(as_handles(h), route, X, Y, f32)
        _launch_check(route, lau, N, K, None)
        return out, lau
    return fn


def _other_route(route, N, K, M):
    def fn(h):
        X, Y = hard(N, K, M)
        if route.startswith("batch"):
            out, lau = run_batch(as_handles(h), route, X, Y)
        else:
            E, lau = run_cv(as_handles(h), route, X, Y)
            out = {"E": E}
        _launch_check(route, lau, N, K, None)
        return out, lau
    return fn


for N, K, M in hd.SHAPES:
    for route in FIT_ROUTES:
        probe(f"fit {route} {N}x{K} m{M}", ROUTE_KIND[FIT_ROUTES[route][1]], route)(_fit_route(route, N, K, M, False))
    for route in OTHER_KIND:
        probe(f"{route} {N}x{K} m{M}", OTHER_KIND[route], route)(_other_route(route, N, K, M))
for N, K, M in ((1301, 48, 1), (60, 400, 2)):
    for route in F32_ROUTES:
        probe(f"fit {route} {N}x{K} m{M} f32", ROUTE_KIND[FIT_ROUTES[route][1]], route + " f32")(_fit_route(route, N, K, M, True))


# 2. the wider fit plans of tests/test_gpu_edge.py, laid out as there (ld = N + ld_extra, base_off elements into the allocation,
#    the scores in the same layout), with its launch-count assertions
def _edge_fit(N, K, M, A, ld_extra, base_off, algo):
    def fn(h):
        Xh, Yh = host(N, K, M, 7)
        X, _kx = cached(("placed", N, K, ld_extra, base_off), lambda: _place(Xh, torch.float64, ld_extra, base_off))
        Y, _ky = cached(("placedY", N, M, ld_extra, base_off), lambda: _place(Yh, torch.float64, ld_extra, base_off))
        ldt = N + ld_extra
        tflat = torch.full((A * ldt + base_off + 8,), 7.0, dtype=torch.float64, device="cuda")
        out = {k: pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K) for k in "WPR"}
        out["Q"] = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M)
        out["B"] = pls_amd.colmajor_empty(K, M, torch.float64, "cuda", ld=K)
        out["T"] = tflat[base_off:base_off + A * ldt].view(A, ldt)[:, :N].t()
        h.set_option(pls_amd.OPT_ALGO, algo)
        try:
            _, lau = counted(h, lambda: h.fit_device(X, Y, A, out=out))
        finally:
            h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
        nipals = algo == pls_amd.ALGO_NIPALS
        unaligned = (N + ld_extra) % 2 != 0 or base_off % 2 != 0
        if K <= 1024:
            assert lau["fused"] == A and lau["xb"] == 0, lau
            assert lau["deflate"] == (1 if (not nipals and unaligned and A >= 4) else 0) and (nipals or lau["xty"] == 0), lau
        elif K <= 4096:
            assert lau["fused"] == A and lau["deflate"] == 1 and lau["xty"] == 0, lau
        elif K <= 8192:
            assert lau["fused"] == A and lau["deflate"] == 1 and lau["xty"] == 0, lau
        else:
            assert lau["fused"] == 0 and sum(lau.values()) > A, lau
        out["guard"] = tflat   # (the cells between the score columns as well: nothing may be written there)
        return out, lau
    return fn


EDGE = [(515, 1500, 2, 5, 0, 0, "short tiles"), (261, 5000, 1, 4, 0, 0, "row-pack tiles"), (75, 9000, 1, 4, 0, 0, "one-product kernels"),
        (100, 20000, 5, 4, 0, 0, "beyond the cooperative update"), (1001, 37, 2, 6, 0, 1, "copy into aligned tiles")]
for N, K, M, A, lde, off, what in EDGE:
    for algo, an in ((pls_amd.ALGO_KERNEL, "kernel"), (pls_amd.ALGO_NIPALS, "nipals")):
        probe(f"fit {an} {N}x{K} m{M} a{A} ({what})", "general", f"{an}: {what}")(_edge_fit(N, K, M, A, lde, off, algo))


@probe("fit gram 2051x513 m3 a5 (several SYRK blocks)", "general", "gram: matrix-core SYRK")
def _gram_syrk(h):
    X, Y = synth(2051, 513, 3, 7)
    h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_GRAM)
    try:
        out, lau = counted(h, lambda: h.fit_device(X, Y, 5))
    finally:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
    assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] <= 1 and lau["xty"] >= 1, lau
    return out, lau


# 3. every other entry point, once per route
def _resampled(N, K, M, A, nrep):
    def fn(h):
        X, Y = synth(N, K, M, 11)
        Wt = cached(("boot", N, nrep), lambda: torch.from_numpy(pls_amd.bootstrap_weights(N, nrep, 5)).cuda())
        out, lau = counted(h, lambda: h.fit_resampled(X, Y, A, Wt, want=("Q", "tt", "B", "B0", "Bmean", "Bm2")))
        passes = lau["fused"] + lau["xb"] + lau["deflate"]
        if h.kind.startswith("dual"):   # everything from one X X^T: G, B0 and the round's B are its three sweeps
            assert passes == 0 and 1 <= lau["xty"] <= 3, lau
        else:                           # one refit per replicate on row-scaled copies: passes over X for each
            assert passes >= nrep, lau
        return out, lau
    return fn


probe("fit_resampled 60x400 m2 a5 x7", "dual", "sample space")(_resampled(60, 400, 2, 5, 7))
probe("fit_resampled 300x40 m2 a5 x5", "general", "one refit per replicate")(_resampled(300, 40, 2, 5, 5))


def _cvb_idx(N, nf, ts):
    return np.random.default_rng(nf).permutation(N)[:nf * ts].reshape(nf, ts)


def _cv_press_batch(N, K, M, A, nprob, nf, ts):
    def fn(h):
        X, Ys = synth(N, K, M * nprob, 13)
        out, lau = counted(h, lambda: h.cv_press_batch(X, Ys, M, A, _cvb_idx(N, nf, ts), want=("PRESS", "ssy", "E")))
        assert lau["xb"] == 0 and lau["deflate"] == 0 and lau["fused"] == 0, lau
        if h.kind == "dual":
            assert lau["xty"] == 1, lau          # one sweep over X and G for the whole call
        else:
            assert lau["xty"] >= nprob, lau      # PLS_HIP_CVBATCH_REFIT=1: one cross-validation per problem
        return out, lau
    return fn


probe("cv_press_batch 60x400 m2 a4 x3", "dual", "sample space")(_cv_press_batch(60, 400, 2, 4, 3, 6, 5))
probe("cv_press_batch 60x400 m2 a4 x3 refit", "dual-refit", "PLS_HIP_CVBATCH_REFIT=1")(_cv_press_batch(60, 400, 2, 4, 3, 6, 5))


@probe("fit_batch 1301x48 m1 x3 rounds of 1", "default-rounds", "batch, PLS_HIP_BATCH_ROUND=1")
def _batch_rounds(h):
    X, Ys = synth(1301, 48, 3, 17)
    out, lau = counted(h, lambda: h.fit_batch(X, Ys, 1, 6, want=("R", "Q", "tt", "B", "ssy")))
    _launch_check("batch", lau, 1301, 48, None)
    assert lau["small"] >= 3, lau                # three rounds
    return out, lau


def _xdiag(new_rows, f32):
    def fn(h):
        N, K, A = 1001, 37, 6
        X, _ = synth(N, K, 1, 19 if new_rows else 7, f32)
        R, P = normal("xdR", K, A), normal("xdP", K, A)
        tv = np.linspace(1.0, 2.0, A) if new_rows else None
        out, lau = counted(h, lambda: h.x_diagnostics(X, R, P, tvar=tv, want=("Q", "T2", "S", "ssx", "sst")))
        assert sum(lau.values()) >= 1, lau
        return out, lau
    return fn


for new_rows in (False, True):
    for f32 in (False, True):
        probe(f"x_diagnostics 1001x37 a6 {'new' if new_rows else 'training'} rows{' f32' if f32 else ''}", "default", "one sweep")(_xdiag(new_rows, f32))


def _validation(lds):
    def fn(h):
        E = normal("valE", 2, 5, 1001).permute(0, 2, 1)   # (M, nobs, A) over the C layout (M, A, nobs)
        keep = h.get_option(pls_amd.OPT_VALIDATION_LDS_ROWS)
        if not lds:
            h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, 0)
        try:
            o, lau = counted(h, lambda: h.validation(E))
        finally:
            h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, keep)
        # LDS route: the end of PRESS and one signed-rank launch; radix route: a bracket per 8-bit pass of the sort besides
        assert (lau["small"] <= 3) if lds else (lau["small"] >= 8), lau
        return dict(zip(("press", "D", "probw", "ref"), o)), lau
    return fn


probe("validation m2 a5 nobs1001 LDS", "default", "one workgroup per pair")(_validation(True))
probe("validation m2 a5 nobs1001 radix", "default", "radix sort (OPT_VALIDATION_LDS_ROWS=0)")(_validation(False))


def _xb(N, K, C):
    def fn(h):
        X, _ = synth(N, K, 1, 7)
        Bm = normal(f"xbB{K}", K, 45)[:, :C]
        out, lau = counted(h, lambda: h.xb(X, Bm))
        assert lau["xb"] >= 1, lau
        return {"XB": out}, lau
    return fn


for N, K in ((130, 6000), (1001, 37)):
    for C in (1, 3, 7, 45):
        probe(f"xb {N}x{K} c{C}", "default", "X B")(_xb(N, K, C))


@probe("xty 1001x37 m2", "default", "X^T Y")
def _xty(h):
    X, Y = synth(1001, 37, 2, 7)
    out, lau = counted(h, lambda: h.xty(X, Y))
    assert lau["xty"] >= 1, lau
    return {"XY": out}, lau


@probe("deflate 1001x37", "default", "deflate")
def _deflate(h):
    X, _ = synth(1001, 37, 2, 7)
    t, p = normal("deflt", 1001), normal("deflp", 37)
    out, lau = counted(h, lambda: h.deflate(X, t, p))
    assert lau["deflate"] >= 1, lau
    return {"D": out}, lau


def _zscores(inplace):
    def fn(h):
        X, _ = synth(1001, 37, 2, 7)
        Xc = pls_amd.colmajor_empty(1001, 37, torch.float64, "cuda").copy_(X) if inplace else X
        (Z, mean, sd), lau = counted(h, lambda: h.colwise_z_scores(Xc, inplace=inplace))
        assert sum(lau.values()) >= 1, lau
        return {"Z": Z, "mean": mean, "sd": sd}, lau
    return fn


probe("colwise_z_scores 1001x37", "default", "out of place")(_zscores(False))
probe("colwise_z_scores 1001x37 in place", "default", "in place")(_zscores(True))


@probe("sse_by_components 1001 a6 m2", "default", "one sweep")
def _sse(h):
    _, Y = synth(1001, 37, 2, 7)
    S, Q = normal("sseS", 1001, 6), normal("sseQ", 2, 6)
    out, lau = counted(h, lambda: h.sse_by_components(S, Y, Q))
    assert sum(lau.values()) >= 1, lau
    return {"SSE": out}, lau


@probe("coefficients 37x6 m2 c4", "default", "one launch (not bracketed)")
def _coefficients(h):
    R, Q = normal("coR", 37, 6), normal("coQ", 2, 6)
    out, lau = counted(h, lambda: h.coefficients(R, Q, 4))
    return {"B": out}, lau


@probe("fit_host 200x5000 then 97x33", "default", "host staging, the smaller after the larger")
def _fit_host_pair(h):
    big, small = host(200, 5000, 1, 23), host(97, 33, 2, 23)
    h.timing()
    a = h.fit_host(big[0], big[1], 4)
    b = h.fit_host(small[0], small[1], 5)
    lau = h.timing()["launches"]
    assert sum(lau.values()) >= 2, lau
    out = {"big_" + k: v for k, v in a.items()}
    out.update({"small_" + k: v for k, v in b.items()})
    return out, lau


def model_sse(h, X, Y, R, Q):
    """pls_hip_model_sse on device matrices (pls_amd.Handle has no method of its own for it)"""
    N, K = X.shape
    M, A = Q.shape
    out = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M)
    L.check(L.lib().pls_hip_model_sse(h.h, X.data_ptr(), int(X.stride(1)), Y.data_ptr(), int(Y.stride(1)), N, K, M, A, R.data_ptr(), Q.data_ptr(),
                                      L.F64, L.MEM_DEVICE, out.data_ptr()), h.h)
    return out


@probe("model_sse 1001x37 m2 a6", "default", "X R, then one sweep")
def _model_sse(h):
    X, Y = synth(1001, 37, 2, 7)
    R, Q = normal("msR", 37, 6), normal("msQ", 2, 6)
    Rk = pls_amd.colmajor_empty(37, 6, torch.float64, "cuda", ld=37).copy_(R)
    Qk = pls_amd.colmajor_empty(2, 6, torch.float64, "cuda", ld=2).copy_(Q)
    out, lau = counted(h, lambda: model_sse(h, X, Y, Rk, Qk))
    assert lau["xb"] >= 1, lau
    return {"SSE": out}, lau


def by_name(name):
    hit = [p for p in PROBES if p[0] == name]
    assert len(hit) == 1, name
    return hit[0]


def run(p, h):
    out, lau = p[3](h)
    return digest(out), tuple(sorted(lau.items()))


# ---- a, b ----------------------------------------------------------------------------------------------------------------------
class Tally:
    def __init__(self):
        self.runs = 0
        self.bad = []

    def check(self, what, got, want):
        self.runs += 1
        if got != want:
            self.bad.append(what)
            which = "digest" if got[0] != want[0] else "launch counts"
            print(f"DIFFERS ({which}): {what}: {got[0][:16]} {dict(got[1])} != baseline {want[0][:16]} {dict(want[1])}", flush=True)


def baselines(kinds, tally):
    base = {}
    for p in PROBES:
        if p[1] not in kinds:
            continue
        with fresh(p[1]) as h:
            base[p[0]] = run(p, h)
        tally.runs += 1
        print(f"probe [{p[1]}] {p[0]}: route {p[2]}; baseline {base[p[0]][0][:16]}; launches {dict(base[p[0]][1])}", flush=True)
    return base


def poisoned(kinds, base, bytes_, orders, tally):
    for kind in kinds:
        mine = [p for p in PROBES if p[1] == kind]
        h = make_handle(kind)
        last, nth = 0, 0
        for order in orders:
            for p in (mine if order == "fwd" else mine[::-1]):
                for byte in bytes_:
                    n = poison(h, byte, 1)
                    assert n >= last, f"the poisoned bytes shrank from {last} to {n} before {p[0]}: a workspace left the list"
                    assert n > 0 or nth == 0, f"nothing to poison before {p[0]}"
                    last, nth = n, nth + 1
                    got = run(p, h)
                    print(f"poison [{kind}] {order} 0x{byte:02X} {p[0]}: {n} bytes poisoned before it; {got[0][:16]}", flush=True)
                    tally.check(f"[{kind}] {order} 0x{byte:02X} {p[0]}", got, base[p[0]])
        poison(h, 0, 0)
        h.close()


# ---- c: host-side state, no poison ------------------------------------------------------------------------------------------------
def host_checks(tally):
    dev_fit = by_name("fit kernel-fused 1301x48 m3")
    wide_fit = by_name("fit nipals 515x1500 m2 a5 (short tiles)")
    with fresh("general") as h:
        want = {p[0]: run(p, h) for p in (dev_fit, wide_fit)}
    for p in (dev_fit, wide_fit):
        with fresh("general") as h:
            want2 = run(p, h)
        tally.check(f"two fresh handles: {p[0]}", want2, want[p[0]])

    # an option toggled, used, and restored
    X, Y = synth(1301, 48, 3, 29)
    toggles = [(pls_amd.OPT_ALGO, v, pls_amd.ALGO_KERNEL, f"OPT_ALGO={v}") for v in
               (pls_amd.ALGO_KERNEL, pls_amd.ALGO_NIPALS, pls_amd.ALGO_GRAM, pls_amd.ALGO_AUTO, pls_amd.ALGO_DUAL)]
    toggles += [(pls_amd.OPT_FUSE, 0, 1, "OPT_FUSE=0"), (pls_amd.OPT_WORK_LAYOUT, 0, 1, "OPT_WORK_LAYOUT=0"), (pls_amd.OPT_DEFER, 3, 1, "OPT_DEFER=3"),
                (pls_amd.OPT_FUSED_GRID, 48, 0, "OPT_FUSED_GRID=48"), (pls_amd.OPT_POWER_ITERS, 7, 48, "OPT_POWER_ITERS=7")]
    with fresh("general") as h:
        Xw, Yw = synth(515, 1500, 2, 29)
        for opt, v, back, what in toggles:
            assert h.get_option(opt) == back, what
            h.set_option(opt, v)
            h.fit_device(X, Y, 6); h.fit_device(Xw, Yw, 5); h.synchronize()
            h.set_option(opt, back)
            for p in (dev_fit, wide_fit):
                tally.check(f"{what} used and restored, then {p[0]}", run(p, h), want[p[0]])
                print(f"host: {what} used and restored, then {p[0]}", flush=True)

    # the graph cache: A, A (captured), B, A, then graph off and A -- all A equal, and equal to a fresh handle's eager A
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        XA, YA = synth(3000, 96, 2, 31)
        XB, YB = synth(3000, 96, 2, 37)
        side.wait_stream(torch.cuda.default_stream())
        res = []
        with fresh("general", stream=side.cuda_stream) as h:
            h.set_option(pls_amd.OPT_PROFILE, 0)   # (a profiled fit is never captured)
            h.set_option(pls_amd.OPT_GRAPH, 1)
            oA = h.fit_device(XA, YA, 5); side.synchronize(); res.append(digest(oA))
            for X_, Y_, keep in ((XA, YA, True), (XA, YA, True), (XB, YB, False), (XA, YA, True), (XA, YA, True)):
                o = h.fit_device(X_, Y_, 5, out=oA if keep else None); side.synchronize()
                if keep:
                    res.append(digest(o))
            h.set_option(pls_amd.OPT_GRAPH, 0)
            o = h.fit_device(XA, YA, 5, out=oA); side.synchronize(); res.append(digest(o))
        with fresh("general", stream=side.cuda_stream) as h:
            o = h.fit_device(XA, YA, 5); side.synchronize()
            eager = digest(o)
        for i, d in enumerate(res):
            tally.check(f"OPT_GRAPH: fit A number {i} of A A A B A A | graph off A", (d, ()), (eager, ()))
        print(f"host: OPT_GRAPH {len(res)} fits of A, eager {eager[:16]}", flush=True)
    side.synchronize()

    # X^T X taken during an upload must not reach a later device-memory fit of other data with the same shape
    gram = by_name("fit gram 1301x48 m3")
    with fresh("general") as h:
        want_g = run(gram, h)
    with fresh("general") as h:
        Xh, Yh = host(1301, 48, 3, 41)
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_GRAM)
        _, lau = counted(h, lambda: h.fit_host(Xh, Yh, 6))
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
        _launch_check("host-gram", lau, 1301, 48, None)
        tally.check("fit_host under GRAM, then " + gram[0], run(gram, h), want_g)
        print("host: fit_host under GRAM, then a device-memory GRAM fit of other data", flush=True)

    # another stream and back
    with fresh("general") as h:
        with torch.cuda.stream(side):
            side.wait_stream(torch.cuda.default_stream())
            h.set_stream(side.cuda_stream)
            h.fit_device(X, Y, 6); h.synchronize()
        h.set_stream(torch.cuda.default_stream().cuda_stream)
        for p in (dev_fit, wide_fit):
            tally.check(f"set_stream and back, then {p[0]}", run(p, h), want[p[0]])
        print("host: set_stream to a second stream and back", flush=True)

    refused_calls(tally)
    resident_checks(tally)


def refused_calls(tally):
    """every refused call of test_bad_arguments_every_entry_point (tests/test_gpu_parity.py), each followed by a probe of the
    same entry point"""
    lib = L.lib()
    nul = ctypes.c_void_p(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    after = {"fit": "fit single-launch 60x400 m2", "xb": "xb 1001x37 c3", "xty": "xty 1001x37 m2", "deflate": "deflate 1001x37",
             "coefficients": "coefficients 37x6 m2 c4", "z": "colwise_z_scores 1001x37", "sse": "sse_by_components 1001 a6 m2",
             "model_sse": "model_sse 1001x37 m2 a6", "cv": "cv 60x400 m2"}
    kind_of = {k: by_name(v)[1] for k, v in after.items()}
    want = {}
    for k, name in after.items():
        with fresh(kind_of[k]) as h:
            want[k] = run(by_name(name), h)
    hs = {kind: make_handle(kind) for kind in set(kind_of.values())}
    X, Y = synth(64, 6, 2, 1)
    out = hs["default"].fit_device(X, Y, 3); hs["default"].synchronize()
    W, P, Q, R, T, B = (out[k] for k in "WPQRTB")
    idx = (ctypes.c_int64 * 2)(0, 99)

    def fit(h, **kw):
        return lib.pls_hip_fit(h, kw.get("X", p(X)), kw.get("ldx", 64), p(Y), 64, kw.get("N", 64), kw.get("K", 6), kw.get("M", 2), kw.get("A", 3),
                               kw.get("method", 0), kw.get("dtype", 0), kw.get("mem", 1), p(W), p(P), p(Q), p(R), p(T), 64, p(B))
    calls = [("fit", 1, lambda h: fit(h, X=nul)), ("fit", 1, lambda h: fit(h, ldx=10)), ("fit", 1, lambda h: fit(h, N=0)), ("fit", 1, lambda h: fit(h, K=0)),
             ("fit", 1, lambda h: fit(h, A=0)), ("fit", 1, lambda h: fit(h, A=7)), ("fit", 1, lambda h: fit(h, method=5)), ("fit", 1, lambda h: fit(h, dtype=9)),
             ("fit", 1, lambda h: fit(h, mem=3)), ("fit", 4, lambda h: fit(h, M=1025)),
             ("xb", 1, lambda h: lib.pls_hip_xb(h, p(X), 64, 64, 6, nul, 6, 2, 0, 1, p(T), 64)),
             ("xb", 1, lambda h: lib.pls_hip_xb(h, p(X), 10, 64, 6, p(R), 6, 2, 0, 1, p(T), 64)),
             ("xty", 1, lambda h: lib.pls_hip_xty(h, p(X), 64, p(Y), 64, 0, 6, 2, 0, p(B))),
             ("deflate", 1, lambda h: lib.pls_hip_deflate(h, p(X), 64, p(X), 64, 64, 6, nul, p(P), 0)),
             ("coefficients", 1, lambda h: lib.pls_hip_coefficients(h, p(R), p(Q), 6, 2, 3, 4, 1, p(B))),
             ("z", 1, lambda h: lib.pls_hip_colwise_z_scores(h, p(X), 64, 64, 10, 6, 0, nul, 64, p(W), p(P))),
             ("sse", 1, lambda h: lib.pls_hip_sse_by_components(h, p(T), 64, p(Y), 64, 64, 3, 2, nul, 0, p(B))),
             ("model_sse", 1, lambda h: lib.pls_hip_model_sse(h, p(X), 64, p(Y), 64, 64, 6, 2, 3, p(R), p(Q), 0, 7, p(B))),
             ("cv", 1, lambda h: lib.pls_hip_cv_folds(h, p(X), 64, p(Y), 64, 64, 6, 2, 3, idx, 1, 2, 0, 1, p(B))),
             ("cv", 1, lambda h: lib.pls_hip_cv_folds(h, p(X), 64, p(Y), 64, 64, 6, 2, 3, idx, 1, 2, 5, 1, p(B))),
             ("fit", 1, lambda h: lib.pls_hip_set_option(h, 42, 1)), ("fit", 1, lambda h: lib.pls_hip_set_option(h, L.OPT_ALGO, 9)),
             ("fit", 1, lambda h: lib.pls_hip_set_reducer(h, L.ALLREDUCE_FN(0), None, 1, 1)),
             ("fit", 1, lambda h: lib.pls_hip_synth_x(h, p(X), 3, 0, 64, 6, 1, 0))]
    for i, (entry, code, call) in enumerate(calls):
        h = hs[kind_of[entry]]
        rc = call(h.h)
        assert rc == code, (i, entry, rc)
        tally.check(f"refused call {i} ({entry}, status {code}), then {after[entry]}", run(by_name(after[entry]), h), want[entry])
    print(f"host: {len(calls)} refused calls, each followed by a probe of its entry point", flush=True)
    for h in hs.values():
        h.close()


def resident_checks(tally):
    """both single-launch resident forms (one response, several) and the X^T X form: three times in a row on one handle (both
    parities of the arrival counters, successive epochs), then two handles on two streams taking turns (resident_turns)"""
    names = ["fit single-launch 1301x48 m1", "fit single-launch 1301x48 m3", "fit single-launch-auto 1301x48 m1", "fit single-launch-auto 1301x48 m3"]
    probes = [by_name(n) for n in names]
    want = {}
    for p in probes:
        with fresh("default") as h:
            want[p[0]] = run(p, h)
    with fresh("default") as h:
        for p in probes:
            for rep in range(3):
                tally.check(f"resident, run {rep + 1} of 3 in a row: {p[0]}", run(p, h), want[p[0]])
        for rep in range(3):   # ... and interleaved: every form meets the counters the others left
            for p in probes:
                tally.check(f"resident, round {rep + 1} of the four forms in turn: {p[0]}", run(p, h), want[p[0]])
    print("host: resident fits three times in a row, and in turn", flush=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.default_stream())
    h1, h2 = make_handle("default", s1.cuda_stream), make_handle("default", s2.cuda_stream)
    for rep in range(3):
        for p in probes:
            for h, s in ((h1, s1), (h2, s2)):
                with torch.cuda.stream(s):
                    got = run(p, h)
                tally.check(f"two handles on two streams, round {rep + 1}, handle on stream {1 if h is h1 else 2}: {p[0]}", got, want[p[0]])
    h1.close(); h2.close()
    print("host: two handles on two streams alternating resident fits", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("group", choices=sorted(GROUPS))
    ap.add_argument("--bytes", default="ff,7f,01")
    ap.add_argument("--orders", default="fwd,rev")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tally = Tally()
    if a.group == "host":
        host_checks(tally)
        nprobes = 0
    else:
        kinds = GROUPS[a.group]
        base = baselines(kinds, tally)
        nprobes = len(base)
        poisoned(kinds, base, [int(b, 16) for b in a.bytes.split(",") if b], [o for o in a.orders.split(",") if o], tally)
    print(f"done: {a.group}: {nprobes} probes, {tally.runs} runs, {len(tally.bad)} differ", flush=True)
    if _util is not None:
        _util.close()
    return 1 if tally.bad else 0


if __name__ == "__main__":
    sys.exit(main())
