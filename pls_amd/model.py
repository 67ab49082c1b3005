"""Python host mirror of the reference's `PLS::Model` fit / predict surface.

Same names, argument meaning and defaults as /root/reference/include/PLS/pls.h:184-266, over
the C-ABI of include/pls_hip.h.  Differences, all at the type level only:
  * matrices are torch CUDA tensors (device path, zero copy) or numpy arrays (host path,
    copied in and out by the library) instead of Eigen matrices;
  * results are real (the reference's Mat2Dc always has zero imaginary parts);
  * shape errors raise PlsHipError(INVALID) where the reference only assert()s
    (src/pls.cpp:345-347, :440, :445).
torch is used for device memory and streams only; all arithmetic on the N-sized data is done
by the HIP kernels behind the C-ABI.
"""
from __future__ import annotations

import ctypes
import functools
import sys

import numpy as np

from . import _lib as L

try:  # torch is plumbing (device memory, streams); the host path works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

KERNEL_TYPE1 = L.KERNEL_TYPE1
KERNEL_TYPE2 = L.KERNEL_TYPE2
RESS, MSE = 0, 1  # PLS::VALIDATION_OUTPUT, reference include/PLS/pls.h:143


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


# ---------------------------------------------------------------------------------------------
# column-major device matrices as torch views
# ---------------------------------------------------------------------------------------------

def colmajor_empty(rows: int, cols: int, dtype, device, ld: int | None = None):
    """(rows, cols) view with strides (1, ld): the reference's Eigen column-major layout
    (include/PLS/pls.h:22-23).  ld defaults to rows rounded up to a 16-byte multiple."""
    es = torch.empty((), dtype=dtype).element_size()
    v = 16 // es
    if ld is None:
        ld = max(rows, 1)
        ld += (-ld) % v
    buf = torch.empty((cols, ld), dtype=dtype, device=device)
    return buf[:, :rows].t()


def as_colmajor(x, dtype=None):
    """Zero-copy if x already has strides (1, ld>=rows) and the dtype matches, else a copy."""
    if dtype is None:
        dtype = x.dtype
    if x.dim() == 1:
        x = x[:, None]
    n, k = x.shape
    ok = x.dtype == dtype and (n <= 1 or x.stride(0) == 1) and (k <= 1 or x.stride(1) >= max(n, 1))
    if ok:
        return x
    out = colmajor_empty(n, k, dtype, x.device)
    out.copy_(x)
    return out


def _ld(x) -> int:
    """leading dimension of a column-major view (a single column may report any stride)"""
    n, k = x.shape
    return max(int(x.stride(1)) if k > 1 else 0, int(n), 1)


def _np_f(x, dtype):
    a = np.asarray(x)
    if a.ndim == 1:
        a = a[:, None]
    return np.asfortranarray(a, dtype=dtype)


def pick_components(probw, ref, alpha: float = 0.1):
    """per response: 1 + the first alt < ref[m] with probw[m, alt] > alpha, else ref[m] + 1 (src/pls.cpp:278-287) from
    the probw (M x A) and 0-based ref (M) of Handle.validation"""
    probw, ref = np.asarray(probw), np.asarray(ref, dtype=np.int64)
    best = ref + 1
    for m, r in enumerate(ref):
        hits = np.flatnonzero(probw[m, :r] > alpha)
        if hits.size:
            best[m] = hits[0] + 1
    return best



def r2y_by_components(Q, tt, ssy):
    """Cumulative R^2 Y of batched fits from the outputs of fit_batch: Q (nprob, M, A), tt (nprob, A), ssy (nprob, M) ->
    (nprob, M, A) with R2[b, m, c] = sum_{a<=c} Q[b, m, a]^2 tt[b, a] / ssy[b, m] (the explained sum of squares of the
    orthogonal scores over the total).  Pure array code: numpy arrays or torch tensors, no GPU needed."""
    if _is_torch(Q):
        Q = Q if Q.dim() == 3 else Q[None]
        tt = tt.reshape(Q.shape[0], 1, Q.shape[2])
        ssy = ssy.reshape(Q.shape[0], Q.shape[1], 1)
        return torch.cumsum(Q * Q * tt, dim=2) / ssy
    Q = np.asarray(Q, dtype=np.float64)
    Q = Q if Q.ndim == 3 else Q[None]
    tt = np.asarray(tt, dtype=np.float64).reshape(Q.shape[0], 1, Q.shape[2])
    ssy = np.asarray(ssy, dtype=np.float64).reshape(Q.shape[0], Q.shape[1], 1)
    return np.cumsum(Q * Q * tt, axis=2) / ssy


def q2_by_components(PRESS, ssy):
    """Cross-validated Q^2 Y from the outputs of cv_press_batch: PRESS (nprob, M, A), ssy (nprob, M) -> (nprob, M, A) with
    Q2[b, m, c] = 1 - PRESS[b, m, c] / ssy[b, m].  Pure array code: numpy arrays or torch tensors, no GPU needed."""
    if _is_torch(PRESS):
        return 1.0 - PRESS / ssy.reshape(PRESS.shape[0], PRESS.shape[1], 1)
    PRESS = np.asarray(PRESS, dtype=np.float64)
    return 1.0 - PRESS / np.asarray(ssy, dtype=np.float64).reshape(PRESS.shape[0], PRESS.shape[1], 1)


def permutation_pvalues(r2_real, r2_perm):
    """(1 + #{b : r2_perm[b] >= r2_real}) / (nperm + 1), elementwise over (M, A): the permutation p-value of every
    (response, component count) with the real model counted among the permutations.  r2_perm: (nperm, M, A)."""
    r2_real = np.asarray(r2_real, dtype=np.float64)
    r2_perm = np.asarray(r2_perm, dtype=np.float64)
    if r2_perm.ndim == r2_real.ndim:
        r2_perm = r2_perm[None]
    return (1.0 + np.sum(r2_perm >= r2_real[None], axis=0)) / (r2_perm.shape[0] + 1.0)


_BATCH_OUT = ("R", "Q", "tt", "B", "ssy")


def _batch_want(want):
    want = set(want)
    bad = want - set(_BATCH_OUT)
    if bad:
        raise L.PlsHipError(L.ERR_INVALID, f"fit_batch: unknown output(s) {sorted(bad)}")
    return want


def _batch_shapes(K, M, A, nprob):
    # logical shapes; every problem's block is column-major (K x A ld K, M x A ld M, K x M ld K) inside a C-ordered stack
    return {"R": (nprob, A, K), "Q": (nprob, A, M), "tt": (nprob, A), "B": (nprob, M, K), "ssy": (nprob, M)}


def _batch_view(name, a):
    """stack of column-major blocks -> (nprob, rows, cols) views"""
    if name in ("R", "Q", "B"):
        return a.permute(0, 2, 1) if _is_torch(a) else a.transpose(0, 2, 1)
    return a

_RESAMPLE_OUT = ("Q", "tt", "B", "B0", "Bmean", "Bm2")
_CVB_OUT = ("PRESS", "ssy", "E")
_MISSING_OUT = ("W", "P", "Q", "R", "T", "B", "iters")


def bootstrap_weights(N: int, nrep: int, seed: int = 0):
    """(N, nrep) fp64, column-major: column b holds the multinomial counts of one bootstrap draw of N rows out of N (how often
    each row was drawn; every column sums to N).  Reproducible by seed.  Pure numpy, no GPU needed."""
    rng = np.random.default_rng(seed)
    counts = rng.multinomial(int(N), np.full(int(N), 1.0 / int(N)), size=int(nrep))
    return np.asfortranarray(counts.T, dtype=np.float64)


def jackknife_weights(N: int, groups=None):
    """(N, g) fp64 0/1, column-major: column j leaves group j out.  groups=None: leave-one-out (g = N, column j drops row
    j); otherwise an array of N group labels, the columns in the order of the sorted distinct labels."""
    if groups is None:
        return np.asfortranarray(1.0 - np.eye(int(N)))
    groups = np.asarray(groups).reshape(-1)
    if groups.shape[0] != int(N):
        raise L.PlsHipError(L.ERR_INVALID, "jackknife_weights: one group label per row")
    labels = np.unique(groups)
    return np.asfortranarray((groups[:, None] != labels[None, :]).astype(np.float64))


def resample_se(Bm2, nrep: int, kind: str = "bootstrap"):
    """standard errors from the Bm2 = sum_b (B_b - Bbar)^2 of fit_resampled over nrep replicates: kind "bootstrap" ->
    sqrt(Bm2 / (nrep - 1)), "jackknife" (delete-a-group over g = nrep groups) -> sqrt((g - 1) / g * Bm2).  Rounding can
    leave Bm2 a hair below zero where the replicates agree: clamped at 0."""
    if kind not in ("bootstrap", "jackknife"):
        raise L.PlsHipError(L.ERR_INVALID, f"resample_se: kind={kind!r}: 'bootstrap' or 'jackknife'")
    if kind == "bootstrap" and nrep < 2:
        raise L.PlsHipError(L.ERR_INVALID, "resample_se: a bootstrap standard error needs nrep >= 2")
    f = 1.0 / (nrep - 1) if kind == "bootstrap" else (nrep - 1.0) / nrep
    if _is_torch(Bm2):
        return torch.sqrt(torch.clamp(Bm2, min=0.0) * f)
    return np.sqrt(np.maximum(np.asarray(Bm2, dtype=np.float64), 0.0) * f)


# ---------------------------------------------------------------------------------------------
# handle
# ---------------------------------------------------------------------------------------------

def _on_handle_stream(method):
    """The method's own torch work -- conversions, copies, the allocation of its outputs -- runs on the HANDLE's stream, where the
    library's kernels run, whatever torch's current stream is (include/pls_hip.h, "Stream order"): a handle made with
    Handle(stream=s) and called under another current stream would otherwise race with its own temporaries."""
    @functools.wraps(method)
    def on_stream(self, *args, **kwargs):
        st = self._tstream
        if st is None or torch.cuda.current_stream(self.device).cuda_stream == self._stream_ptr:
            return method(self, *args, **kwargs)
        with torch.cuda.stream(st):
            return method(self, *args, **kwargs)
    return on_stream


class Handle:
    """One pls_hip context: a device, a stream, its workspace and (optionally) a reducer."""

    def __init__(self, device: int | None = None, stream: int | None = None):
        self._lib = L.lib()
        if device is None:
            device = torch.cuda.current_device() if (torch is not None and torch.cuda.is_available()) else 0
        if stream is None and torch is not None and torch.cuda.is_available():
            stream = torch.cuda.current_stream(device).cuda_stream
        self.device = int(device)
        h = ctypes.c_void_p()
        L.check(self._lib.pls_hip_create(ctypes.byref(h), self.device, ctypes.c_void_p(stream or 0)))
        self.h = h
        self._keep = []  # objects the C side points at (callbacks, reduce buffers)
        self._view_stream(stream)

    def _view_stream(self, stream):
        """torch's view of the handle's stream (None without a GPU): what _on_handle_stream runs the methods' torch work under"""
        self._stream_ptr = int(stream or 0)
        self._tstream = None
        if torch is not None and torch.cuda.is_available():
            self._tstream = (torch.cuda.ExternalStream(self._stream_ptr, device=self.device) if self._stream_ptr
                             else torch.cuda.default_stream(self.device))

    def close(self):
        if getattr(self, "h", None):
            self._lib.pls_hip_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int):
        L.check(self._lib.pls_hip_set_option(self.h, opt, int(value)), self.h)

    def get_option(self, opt: int) -> int:
        v = ctypes.c_int64()
        L.check(self._lib.pls_hip_get_option(self.h, opt, ctypes.byref(v)), self.h)
        return int(v.value)

    def set_stream(self, stream: int | None):
        L.check(self._lib.pls_hip_set_stream(self.h, ctypes.c_void_p(stream or 0)), self.h)
        self._view_stream(stream)

    def synchronize(self):
        L.check(self._lib.pls_hip_synchronize(self.h), self.h)

    def clear_reducer(self):
        """back to a single-rank handle (the reducer installed by pls_amd.distributed.attach_reducer is dropped)"""
        self.synchronize()
        L.check(self._lib.pls_hip_set_reduce_buffer(self.h, None, 0), self.h)
        L.check(self._lib.pls_hip_set_reducer(self.h, L.ALLREDUCE_FN(), None, 0, 1), self.h)

    def timing(self) -> dict:
        t = L.Timing()
        L.check(self._lib.pls_hip_get_timing(self.h, ctypes.byref(t)), self.h)
        return {"fit_ms": t.fit_ms, "fits": int(t.fits),
                "ms": {n: t.fam_ms[i] for i, n in enumerate(L.FAM_NAMES)},
                "launches": {n: int(t.fam_launches[i]) for i, n in enumerate(L.FAM_NAMES)},
                "bytes": {n: int(t.fam_bytes[i]) for i, n in enumerate(L.FAM_NAMES)}}

    # ---- raw steps on device tensors (tests, bench) -----------------------------------------
    def _dt(self, x):
        return L.F64 if x.dtype == torch.float64 else L.F32

    @_on_handle_stream
    def fit_device(self, X, Y, A: int, method: int = KERNEL_TYPE1, want_B: bool = True, out=None):
        """X (N,K), Y (N,M) column-major CUDA tensors of one dtype.  Enqueues the fit and
        returns dict(W,P,Q,R,T,B) of device tensors (column-major views).  `out`: a dict
        returned by an earlier call with the same shapes, to be overwritten in place."""
        X = as_colmajor(X)
        Y = as_colmajor(Y, X.dtype)
        N, K = X.shape
        M = Y.shape[1]
        dev = X.device
        f64 = torch.float64
        if out is not None:
            W, P, Q, R, T, B = (out[k] for k in "WPQRTB")
            want_B = B is not None
        else:
            W = colmajor_empty(K, A, f64, dev, ld=K); P = colmajor_empty(K, A, f64, dev, ld=K)
            R = colmajor_empty(K, A, f64, dev, ld=K); Q = colmajor_empty(M, A, f64, dev, ld=M)
            # the scores exist for KERNEL_TYPE1 only (reference src/pls.cpp:394,434): None for KERNEL_TYPE2
            T = colmajor_empty(N, A, X.dtype, dev) if method == KERNEL_TYPE1 else None
            B = colmajor_empty(K, M, f64, dev, ld=K) if want_B else None
        if method == KERNEL_TYPE1 and T is None:
            raise L.PlsHipError(L.ERR_INVALID, "KERNEL_TYPE1 needs a T buffer in `out`")
        rc = self._lib.pls_hip_fit(self.h, X.data_ptr(), _ld(X), Y.data_ptr(), _ld(Y), N, K, M, A,
                                   method, self._dt(X), L.MEM_DEVICE, W.data_ptr(), P.data_ptr(),
                                   Q.data_ptr(), R.data_ptr(), T.data_ptr() if T is not None else None,
                                   _ld(T) if T is not None else max(N, 1), B.data_ptr() if want_B else None)
        L.check(rc, self.h)
        self._last_inputs = (X, Y)  # keep alive until the stream has consumed them
        return dict(W=W, P=P, Q=Q, R=R, T=T if method == KERNEL_TYPE1 else None, B=B)

    def fit_host(self, X, Y, A: int, method: int = KERNEL_TYPE1, dtype=np.float64):
        X = _np_f(X, dtype); Y = _np_f(Y, dtype)
        N, K = X.shape
        M = Y.shape[1]
        W = np.zeros((K, A), order="F"); P = np.zeros((K, A), order="F")
        R = np.zeros((K, A), order="F"); Q = np.zeros((M, A), order="F")
        B = np.zeros((K, M), order="F")
        T = np.zeros((N, A), dtype=dtype, order="F")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.pls_hip_fit(self.h, p(X), max(N, 1), p(Y), max(N, 1), N, K, M, A, method,
                                   L.F64 if dtype == np.float64 else L.F32, L.MEM_HOST,
                                   p(W), p(P), p(Q), p(R), p(T), max(N, 1), p(B))
        L.check(rc, self.h)
        return dict(W=W, P=P, Q=Q, R=R, T=T if method == KERNEL_TYPE1 else None, B=B)

    @_on_handle_stream
    def xb(self, X, Bm):
        """X (N,K) @ Bm (K,C): fitted_values / scores product."""
        if _is_torch(X):
            X = as_colmajor(X)
            Bm = as_colmajor(Bm.to(torch.float64))
            N, K = X.shape
            C = Bm.shape[1]
            out = colmajor_empty(N, C, X.dtype, X.device)
            rc = self._lib.pls_hip_xb(self.h, X.data_ptr(), _ld(X), N, K, Bm.data_ptr(), _ld(Bm), C,
                                      self._dt(X), L.MEM_DEVICE, out.data_ptr(), _ld(out))
            L.check(rc, self.h)
            self._last_inputs = (X, Bm)
            return out
        dtype = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dtype); Bm = _np_f(Bm, np.float64)
        N, K = X.shape
        C = Bm.shape[1]
        out = np.zeros((N, C), dtype=dtype, order="F")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.pls_hip_xb(self.h, p(X), max(N, 1), N, K, p(Bm), K, C,
                                  L.F64 if dtype == np.float64 else L.F32, L.MEM_HOST, p(out), max(N, 1))
        L.check(rc, self.h)
        return out

    @_on_handle_stream
    def coefficients(self, R, Q, c: int):
        if _is_torch(R):
            R = as_colmajor(R); Q = as_colmajor(Q)
            K, A = R.shape
            M = Q.shape[0]
            if _ld(R) != K or _ld(Q) != M:
                R = colmajor_empty(K, A, torch.float64, R.device, ld=K).copy_(R)
                Q = colmajor_empty(M, A, torch.float64, Q.device, ld=M).copy_(Q)
            B = colmajor_empty(K, M, torch.float64, R.device, ld=K)
            rc = self._lib.pls_hip_coefficients(self.h, R.data_ptr(), Q.data_ptr(), K, M, A, c,
                                                L.MEM_DEVICE, B.data_ptr())
            L.check(rc, self.h)
            self._last_inputs = (R, Q)
            return B
        R = _np_f(R, np.float64); Q = _np_f(Q, np.float64)
        K, A = R.shape
        M = Q.shape[0]
        B = np.zeros((K, M), order="F")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        L.check(self._lib.pls_hip_coefficients(self.h, p(R), p(Q), K, M, A, c, L.MEM_HOST, p(B)), self.h)
        return B

    @_on_handle_stream
    def xty(self, X, Y):
        X = as_colmajor(X); Y = as_colmajor(Y, X.dtype)
        N, K = X.shape
        M = Y.shape[1]
        out = colmajor_empty(K, M, torch.float64, X.device, ld=K)
        L.check(self._lib.pls_hip_xty(self.h, X.data_ptr(), _ld(X), Y.data_ptr(), _ld(Y), N, K, M,
                                      self._dt(X), out.data_ptr()), self.h)
        self._last_inputs = (X, Y)
        return out

    @_on_handle_stream
    def deflate(self, src, t, p, dst=None):
        src = as_colmajor(src)
        N, K = src.shape
        if dst is None:
            dst = colmajor_empty(N, K, src.dtype, src.device)
        t = t.to(src.dtype).contiguous()
        p = p.to(torch.float64).contiguous()
        L.check(self._lib.pls_hip_deflate(self.h, src.data_ptr(), _ld(src), dst.data_ptr(), _ld(dst),
                                          N, K, t.data_ptr(), p.data_ptr(), self._dt(src)), self.h)
        self._last_inputs = (src, t, p)
        return dst

    @_on_handle_stream
    def colwise_z_scores(self, X, n_total: int | None = None, inplace: bool = False):
        """(Z, mean, sd) of a device matrix: colwise_z_scores of the reference (src/pls.cpp:107-111)."""
        X = as_colmajor(X)
        N, K = X.shape
        Z = X if inplace else colmajor_empty(N, K, X.dtype, X.device)
        mean = torch.empty(K, dtype=torch.float64, device=X.device)
        sd = torch.empty(K, dtype=torch.float64, device=X.device)
        L.check(self._lib.pls_hip_colwise_z_scores(self.h, X.data_ptr(), _ld(X), N, n_total or N, K, self._dt(X),
                                                   Z.data_ptr(), _ld(Z), mean.data_ptr(), sd.data_ptr()), self.h)
        self._last_inputs = (X,)
        return Z, mean, sd

    @_on_handle_stream
    def sse_by_components(self, S, Y, Q):
        """SSE (M x A) for 1..A components from the scores S = X R (one sweep)."""
        S = as_colmajor(S); Y = as_colmajor(Y, S.dtype)
        N, A = S.shape
        M = Y.shape[1]
        Q = as_colmajor(Q.to(torch.float64))
        if _ld(Q) != M:
            Q = colmajor_empty(M, A, torch.float64, Q.device, ld=M).copy_(Q)
        out = colmajor_empty(M, A, torch.float64, S.device, ld=M)
        L.check(self._lib.pls_hip_sse_by_components(self.h, S.data_ptr(), _ld(S), Y.data_ptr(), _ld(Y), N, A, M,
                                                    Q.data_ptr(), self._dt(S), out.data_ptr()), self.h)
        self._last_inputs = (S, Y, Q)
        return out

    @_on_handle_stream
    def cv_folds(self, X, Y, A: int, test_idx):
        """Residuals of batched cross-validation folds (cv_LOO / cv_LSO of the reference in one launch).
        test_idx: (num_folds, test_size) integer array of held-out rows.  Returns E with shape (M, nobs, A),
        nobs = num_folds * test_size: E[m] is what Residual.errors()[m] holds.
        The handle's plan decides the route: with OPT_ALGO = ALGO_DUAL (no reducer, N <= 8192, M <= 32) every fold runs from
        one G = X X^T -- one sweep over X for the whole call, whatever A and the number of folds are; the route for short,
        wide X.  Every other handle routes by shape: single-launch fits per fold for small data,
        the shared X^T X for K <= 16384, one refit per fold beyond.
        On a row-sharded handle (attach_reducer / attach_ipc_exchange) the call is a collective: every rank calls it with
        its own block of rows (possibly none) and the same A and test_idx, whose entries are GLOBAL row indices (blocks
        contiguous in rank order, as pls_amd.distributed.row_partition makes them); every rank receives the full E."""
        idx = np.ascontiguousarray(np.asarray(test_idx, dtype=np.int64))
        if idx.ndim == 1:
            idx = idx[:, None]
        nf, ts = idx.shape
        if _is_torch(X):
            X = as_colmajor(X); Y = as_colmajor(Y, X.dtype)
            N, K = X.shape
            M = Y.shape[1]
            E = torch.empty((M, A, nf * ts), dtype=torch.float64, device=X.device)
            rc = self._lib.pls_hip_cv_folds(self.h, X.data_ptr(), _ld(X), Y.data_ptr(), _ld(Y), N, K, M, A,
                                            idx.ctypes.data_as(ctypes.c_void_p), ts, nf, self._dt(X), L.MEM_DEVICE,
                                            E.data_ptr())
            L.check(rc, self.h)
            return E.permute(0, 2, 1)
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); Y = _np_f(Y, dt)
        N, K = X.shape
        M = Y.shape[1]
        E = np.zeros((M, A, nf * ts))
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.pls_hip_cv_folds(self.h, p(X), max(N, 1), p(Y), max(N, 1), N, K, M, A, p(idx), ts, nf,
                                        L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, p(E))
        L.check(rc, self.h)
        return E.transpose(0, 2, 1)

    @_on_handle_stream
    def validation(self, E):
        """(press, D, probw, ref) of cross-validation residuals E, shape (M, nobs, A) as cv_folds returns them
        (pls_hip_validation): press (M, A) = column sums of squares, ref (M,) int64 = 0-based column of the PRESS minimum,
        D / probw (M, A) = Wilcoxon signed-rank sum and p-value of every alt < ref[m] against column ref[m] (0 / NaN
        elsewhere).  A torch CUDA tensor stays on the device (the permuted view cv_folds returns is passed on without a
        copy), numpy goes through the library's host path.  Local on a row-sharded handle: no message is sent."""
        if _is_torch(E):
            E = E if E.dim() == 3 else E[None]
            M, nobs, A = E.shape
            base = E.permute(0, 2, 1)  # the C layout: (M, A, nobs) contiguous
            if base.dtype != torch.float64 or not base.is_contiguous():
                base = base.to(torch.float64).contiguous()
            press, D, probw = (colmajor_empty(M, A, torch.float64, E.device, ld=M) for _ in range(3))
            ref = torch.empty(M, dtype=torch.int64, device=E.device)
            rc = self._lib.pls_hip_validation(self.h, base.data_ptr(), nobs, A, M, L.MEM_DEVICE, press.data_ptr(),
                                              D.data_ptr(), probw.data_ptr(), ref.data_ptr())
            L.check(rc, self.h)
            self._last_inputs = (base,)
            return press, D, probw, ref
        a = np.asarray(E)
        a = a if a.ndim == 3 else a[None]
        M, nobs, A = a.shape
        base = np.ascontiguousarray(a.transpose(0, 2, 1), dtype=np.float64)
        press, D, probw = (np.zeros((M, A), order="F") for _ in range(3))
        ref = np.zeros(M, dtype=np.int64)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        L.check(self._lib.pls_hip_validation(self.h, p(base), nobs, A, M, L.MEM_HOST, p(press), p(D), p(probw), p(ref)),
                self.h)
        return press, D, probw, ref

    @_on_handle_stream
    def x_diagnostics(self, X, R, P, tvar=None, want=("Q", "T2", "ssx"), n_total: int | None = None):
        """X-space diagnostics of a model (R, P: K x A) on data X (N x K) for every component count 1..A
        (pls_hip_x_diagnostics).  `want` picks from "Q" (Q residuals, N x A), "T2" (Hotelling T^2, N x A), "S" (scores,
        N x A in the dtype of X), "ssx" (A + 1: sum X^2, then the sums of the Q columns), "sst" (A: column sums of squares of
        the scores); the result is a dict of those.  tvar (A) = t_a^T t_a / (n_train - 1) of the training scores; None means
        X IS the training data.  Torch CUDA tensors stay on the device, numpy arrays take the library's host path.
        Row-sharded handle: a collective, n_total = rows over all ranks."""
        want = set(want)
        bad = want - {"Q", "T2", "S", "ssx", "sst"}
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"x_diagnostics: unknown output(s) {sorted(bad)}")
        if _is_torch(X):
            X = as_colmajor(X)
            N, K = X.shape
            dev, f64 = X.device, torch.float64
            R = as_colmajor(R.to(f64)); P = as_colmajor(P.to(f64))
            A = R.shape[1]
            if _ld(R) != K:
                R = colmajor_empty(K, A, f64, dev, ld=K).copy_(R)
            if _ld(P) != K:
                P = colmajor_empty(K, A, f64, dev, ld=K).copy_(P)
            tv = None if tvar is None else torch.as_tensor(tvar, dtype=f64, device=dev).contiguous()
            out = {}
            if "Q" in want: out["Q"] = colmajor_empty(N, A, f64, dev)
            if "T2" in want: out["T2"] = colmajor_empty(N, A, f64, dev)
            if "S" in want: out["S"] = colmajor_empty(N, A, X.dtype, dev)
            if "ssx" in want: out["ssx"] = torch.empty(A + 1, dtype=f64, device=dev)
            if "sst" in want: out["sst"] = torch.empty(A, dtype=f64, device=dev)
            ptr = lambda k: out[k].data_ptr() if k in out else None
            ldo = lambda k: _ld(out[k]) if k in out else 1
            rc = self._lib.pls_hip_x_diagnostics(self.h, X.data_ptr(), _ld(X), N, n_total or N, K, A, R.data_ptr(), P.data_ptr(),
                                                 tv.data_ptr() if tv is not None else None, self._dt(X), L.MEM_DEVICE,
                                                 ptr("Q"), ldo("Q"), ptr("T2"), ldo("T2"), ptr("S"), ldo("S"), ptr("ssx"), ptr("sst"))
            L.check(rc, self.h)
            self._last_inputs = (X, R, P, tv)
            return out
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); R = _np_f(R, np.float64); P = _np_f(P, np.float64)
        N, K = X.shape
        A = R.shape[1]
        tv = None if tvar is None else np.ascontiguousarray(tvar, dtype=np.float64)
        out = {}
        if "Q" in want: out["Q"] = np.zeros((N, A), order="F")
        if "T2" in want: out["T2"] = np.zeros((N, A), order="F")
        if "S" in want: out["S"] = np.zeros((N, A), dtype=dt, order="F")
        if "ssx" in want: out["ssx"] = np.zeros(A + 1)
        if "sst" in want: out["sst"] = np.zeros(A)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ptr = lambda k: p(out[k]) if k in out else None
        rc = self._lib.pls_hip_x_diagnostics(self.h, p(X), max(N, 1), N, n_total or N, K, A, p(R), p(P),
                                             p(tv) if tv is not None else None, L.F64 if dt == np.float64 else L.F32, L.MEM_HOST,
                                             ptr("Q"), max(N, 1), ptr("T2"), max(N, 1), ptr("S"), max(N, 1), ptr("ssx"), ptr("sst"))
        L.check(rc, self.h)
        return out

    @_on_handle_stream
    def var_diagnostics(self, X, W=None, R=None, P=None, Q=None, tt=None, want=("VIP", "ssxk")):
        """Variable-space diagnostics of a model on data X (N x K) for every component count 1..A (pls_hip_var_diagnostics).
        `want` picks from "VIP" (K x A: variable importance in projection; needs W, Q and either tt = t_a^T t_a of the training
        scores or X and R, whose scores then stand in), "ssxk" (K x (A + 1): sum_i X[i,k]^2, then the residual sums of squares of
        variable k after 1..A components -- R^2 X of the variable is 1 - ssxk[:, c] / ssxk[:, 0]; needs X, R, P) and "sst" (A:
        column sums of squares of the scores of X; needs X, R); the result is a dict of those.  X may be None when only "VIP" is
        asked for and tt is given.  Torch CUDA tensors are passed as they are and the call only enqueues; numpy inputs are
        uploaded with torch and numpy arrays come back.  Row-sharded handle: a collective whenever X is needed."""
        want = set(want)
        bad = want - {"VIP", "ssxk", "sst"}
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"var_diagnostics: unknown output(s) {sorted(bad)}")
        given = [m for m in (X, W, R, P, Q) if m is not None]
        on_dev = any(_is_torch(m) for m in given)
        if not on_dev and not torch.cuda.is_available():
            raise L.PlsHipError(L.ERR_DEVICE, "var_diagnostics: numpy inputs are uploaded with torch, which finds no device")
        dev = next((m.device for m in given if _is_torch(m)), torch.device("cuda", self.device))
        f64 = torch.float64

        def mat(m):
            """the K x A (M x A) model matrix m as fp64 on the device, its columns packed (ld = its row count)"""
            if m is None:
                return None
            t = as_colmajor(m.to(f64) if _is_torch(m) else torch.as_tensor(_np_f(m, np.float64)).to(dev))
            if _ld(t) != t.shape[0]:
                t = colmajor_empty(t.shape[0], t.shape[1], f64, dev, ld=t.shape[0]).copy_(t)
            return t
        if X is not None and not _is_torch(X):
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            Xh = _np_f(X, dt)
            X = colmajor_empty(Xh.shape[0], Xh.shape[1], torch.float32 if dt == np.float32 else f64, dev)
            X.copy_(torch.from_numpy(np.ascontiguousarray(Xh)))
        elif X is not None:
            X = as_colmajor(X)
        W, R, P, Q = mat(W), mat(R), mat(P), mat(Q)
        shaped = next((m for m in (W, R, P) if m is not None), None)
        if shaped is None:
            raise L.PlsHipError(L.ERR_INVALID, "var_diagnostics: one of W, R, P must be given")
        K, A = shaped.shape
        N = X.shape[0] if X is not None else 0
        M = Q.shape[0] if Q is not None else 0
        tv = None if tt is None else torch.as_tensor(tt, dtype=f64).to(dev).contiguous()
        out = {}
        if "VIP" in want: out["VIP"] = colmajor_empty(K, A, f64, dev)
        if "ssxk" in want: out["ssxk"] = colmajor_empty(K, A + 1, f64, dev)
        if "sst" in want: out["sst"] = torch.empty(A, dtype=f64, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self._lib.pls_hip_var_diagnostics(self.h, ptr(X), _ld(X) if X is not None else 1, N, K, M, A, ptr(W), ptr(R), ptr(P), ptr(Q),
                                               ptr(tv), self._dt(X) if X is not None else L.F64, ptr(out.get("ssxk")),
                                               _ld(out["ssxk"]) if "ssxk" in out else K, ptr(out.get("VIP")),
                                               _ld(out["VIP"]) if "VIP" in out else K, ptr(out.get("sst")))
        L.check(rc, self.h)
        self._last_inputs = (X, W, R, P, Q, tv)
        if on_dev:
            return out
        self.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    @_on_handle_stream
    def fit_batch(self, X, Ys, M: int, A: int, want=("B", "Q", "tt", "ssy")):
        """Many response sets against one X (pls_hip_fit_batch): Ys is N x (nprob * M), problem b owning columns
        [b*M, (b+1)*M); every problem is the KERNEL_TYPE2 model of (X, Y_b) on the shared X^T X.  Returns a dict of the
        outputs `want` names: "R" (nprob, K, A), "Q" (nprob, M, A), "tt" (nprob, A), "B" (nprob, K, M), "ssy" (nprob, M) --
        torch tensors on the device of X for torch inputs (the call only enqueues), numpy arrays for numpy inputs.
        W, P and T are not available here: fit one problem with fit_device / fit_host for those.
        With OPT_ALGO = ALGO_DUAL (no reducer, N <= 8192, M <= 32) every problem runs from one X X^T instead: any K, one sweep
        over X for Q, tt and ssy, one wide product per output for R and B.
        Row-sharded handle: a collective, X and Ys the rank's own rows; every rank receives identical outputs."""
        want = _batch_want(want)
        if _is_torch(X):
            X = as_colmajor(X); Ys = as_colmajor(Ys, X.dtype)
            N, K = X.shape
            C = Ys.shape[1]
            if M < 1 or C % M:
                raise L.PlsHipError(L.ERR_INVALID, "fit_batch: the columns of Ys are not a multiple of M")
            nprob = C // M
            shp = _batch_shapes(K, M, A, nprob)
            out = {k: torch.empty(shp[k], dtype=torch.float64, device=X.device) for k in _BATCH_OUT if k in want}
            ptr = lambda k: out[k].data_ptr() if k in out else None
            rc = self._lib.pls_hip_fit_batch(self.h, X.data_ptr() or None, _ld(X), Ys.data_ptr() or None, _ld(Ys), N, K, M, A,
                                             nprob, self._dt(X), L.MEM_DEVICE, ptr("R"), ptr("Q"), ptr("tt"), ptr("B"), ptr("ssy"))
            L.check(rc, self.h)
            self._last_inputs = (X, Ys)
            return {k: _batch_view(k, v) for k, v in out.items()}
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); Ys = _np_f(Ys, dt)
        N, K = X.shape
        C = Ys.shape[1]
        if M < 1 or C % M:
            raise L.PlsHipError(L.ERR_INVALID, "fit_batch: the columns of Ys are not a multiple of M")
        nprob = C // M
        shp = _batch_shapes(K, M, A, nprob)
        out = {k: np.zeros(shp[k]) for k in _BATCH_OUT if k in want}
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ptr = lambda k: p(out[k]) if k in out else None
        rc = self._lib.pls_hip_fit_batch(self.h, p(X), max(N, 1), p(Ys), max(N, 1), N, K, M, A, nprob,
                                         L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, ptr("R"), ptr("Q"), ptr("tt"), ptr("B"),
                                         ptr("ssy"))
        L.check(rc, self.h)
        return {k: _batch_view(k, v) for k, v in out.items()}

    @_on_handle_stream
    def fit_resampled(self, X, Y, A: int, weights, want=("B0", "Bmean", "Bm2")):
        """The same (X, Y) fitted under many sets of non-negative row weights (pls_hip_fit_resampled): weights is N x nrep,
        replicate b the KERNEL_TYPE1 model of (diag(s) X, diag(s) Y) with s = sqrt(weights[:, b]) -- bootstrap_weights,
        jackknife_weights, or one column of case weights.  No centring.  Returns a dict of the outputs `want` names: "Q"
        (nrep, M, A), "tt" (nrep, A), "B" (nrep, K, M: coefficients for unscaled rows), "B0" (K, M: the unit-weight fit),
        "Bmean" and "Bm2" (K, M: mean and sum of squared deviations of B over the replicates; resample_se scales Bm2) --
        torch tensors on the device of X for torch inputs (the call only enqueues), numpy arrays for numpy inputs.
        With OPT_ALGO = ALGO_DUAL (N <= 8192, M <= 32) every replicate runs from one X X^T: one sweep over X, plus one per
        round of replicates for B; every other handle refits row-scaled copies per replicate.
        The weights are not inspected: a negative weight gives NaN.  A handle with a reducer: PLS_HIP_ERR_UNSUPPORTED."""
        want = set(want)
        bad = want - set(_RESAMPLE_OUT)
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"fit_resampled: unknown output(s) {sorted(bad)}")
        if _is_torch(X):
            X = as_colmajor(X); Y = as_colmajor(Y, X.dtype)
            N, K = X.shape
            M = Y.shape[1]
            Wt = as_colmajor(torch.as_tensor(weights, device=X.device), torch.float64)
            if Wt.shape[0] != N:
                raise L.PlsHipError(L.ERR_INVALID, "fit_resampled: weights must have one row per row of X")
            nrep = Wt.shape[1]
            shp = {"Q": (nrep, A, M), "tt": (nrep, A), "B": (nrep, M, K), "B0": (M, K), "Bmean": (M, K), "Bm2": (M, K)}
            out = {k: torch.empty(shp[k], dtype=torch.float64, device=X.device) for k in _RESAMPLE_OUT if k in want}
            ptr = lambda k: out[k].data_ptr() if k in out else None
            rc = self._lib.pls_hip_fit_resampled(self.h, X.data_ptr() or None, _ld(X), Y.data_ptr() or None, _ld(Y), N, K, M, A,
                                                 Wt.data_ptr() or None, _ld(Wt), nrep, self._dt(X), L.MEM_DEVICE,
                                                 *[ptr(k) for k in _RESAMPLE_OUT])
            L.check(rc, self.h)
            self._last_inputs = (X, Y, Wt)
            return {k: (v.permute(0, 2, 1) if k in ("Q", "B") else v.t() if k != "tt" else v) for k, v in out.items()}
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); Y = _np_f(Y, dt)
        Wt = _np_f(weights, np.float64)
        N, K = X.shape
        M = Y.shape[1]
        if Wt.shape[0] != N:
            raise L.PlsHipError(L.ERR_INVALID, "fit_resampled: weights must have one row per row of X")
        nrep = Wt.shape[1]
        shp = {"Q": (nrep, A, M), "tt": (nrep, A), "B": (nrep, M, K), "B0": (M, K), "Bmean": (M, K), "Bm2": (M, K)}
        out = {k: np.zeros(shp[k]) for k in _RESAMPLE_OUT if k in want}
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ptr = lambda k: p(out[k]) if k in out else None
        rc = self._lib.pls_hip_fit_resampled(self.h, p(X), max(N, 1), p(Y), max(N, 1), N, K, M, A, p(Wt), max(N, 1), nrep,
                                             L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, *[ptr(k) for k in _RESAMPLE_OUT])
        L.check(rc, self.h)
        return {k: (v.transpose(0, 2, 1) if k in ("Q", "B") else v.T if k != "tt" else v) for k, v in out.items()}

    @_on_handle_stream
    def cv_press_batch(self, X, Ys, M: int, A: int, test_idx, want=("PRESS", "ssy")):
        """Cross-validated fits of many response sets against one X, reduced to PRESS (pls_hip_cv_press_batch): Ys is
        N x (nprob * M) as in fit_batch, test_idx (num_folds, test_size) as in cv_folds, the same folds for every problem.
        Returns a dict of the outputs `want` names: "PRESS" (nprob, M, A) = the column sums of squares of the problem's
        cross-validation residuals, "ssy" (nprob, M) = the sum of squares of the responses over the same held-out
        observations (q2_by_components: Q^2 = 1 - PRESS / ssy), "E" (nprob, M, nobs, A) = the residuals themselves, what
        cv_folds returns per problem -- torch tensors on the device of X for torch inputs, numpy arrays for numpy inputs.
        The call returns after the work has completed.
        With OPT_ALGO = ALGO_DUAL (no reducer, N <= 8192, M <= 32) every problem and fold runs from one G = X X^T: one sweep
        over X for the whole call; every other handle runs one cross-validation per problem.
        A handle with a reducer: PLS_HIP_ERR_UNSUPPORTED."""
        want = set(want)
        bad = want - set(_CVB_OUT)
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"cv_press_batch: unknown output(s) {sorted(bad)}")
        idx = np.ascontiguousarray(np.asarray(test_idx, dtype=np.int64))
        if idx.ndim == 1:
            idx = idx[:, None]
        nf, ts = idx.shape
        on_dev = _is_torch(X)
        if on_dev:
            X = as_colmajor(X); Ys = as_colmajor(Ys, X.dtype)
        else:
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            X = _np_f(X, dt); Ys = _np_f(Ys, dt)
        N, K = X.shape
        C = Ys.shape[1]
        if M < 1 or C % M:
            raise L.PlsHipError(L.ERR_INVALID, "cv_press_batch: the columns of Ys are not a multiple of M")
        nprob = C // M
        # every problem's block in the library's layout (M x A ld M; M matrices of nobs x A) inside a C-ordered stack
        shp = {"PRESS": (nprob, A, M), "ssy": (nprob, M), "E": (nprob, M, A, nf * ts)}
        view = {"PRESS": (0, 2, 1), "ssy": (0, 1), "E": (0, 1, 3, 2)}
        if on_dev:
            out = {k: torch.empty(shp[k], dtype=torch.float64, device=X.device) for k in _CVB_OUT if k in want}
            ptr = lambda k: out[k].data_ptr() if k in out else None
            rc = self._lib.pls_hip_cv_press_batch(self.h, X.data_ptr() or None, _ld(X), Ys.data_ptr() or None, _ld(Ys), N, K, M, A,
                                                  nprob, idx.ctypes.data_as(ctypes.c_void_p), ts, nf, self._dt(X), L.MEM_DEVICE,
                                                  *[ptr(k) for k in _CVB_OUT])
            L.check(rc, self.h)
            return {k: v.permute(*view[k]) for k, v in out.items()}
        out = {k: np.zeros(shp[k]) for k in _CVB_OUT if k in want}
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ptr = lambda k: p(out[k]) if k in out else None
        rc = self._lib.pls_hip_cv_press_batch(self.h, p(X), max(N, 1), p(Ys), max(N, 1), N, K, M, A, nprob, p(idx), ts, nf,
                                              L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, *[ptr(k) for k in _CVB_OUT])
        L.check(rc, self.h)
        return {k: v.transpose(*view[k]) for k, v in out.items()}

    # ---- X with missing values -----------------------------------------------------------------------
    @_on_handle_stream
    def fit_missing(self, X, Y, A: int, want=("W", "P", "Q", "R", "T", "B", "iters")):
        """NIPALS fit of X whose NaN cells are missing values (pls_hip_fit_missing): every inner product runs over the
        observed cells only.  Y must be complete.  Returns a dict of the outputs `want` names -- W, P, R (K, A), Q (M, A), T
        (N, A, dtype of X), B (K, M) = R Q^T, iters (A, int64: the iterations each component took) -- torch tensors on the
        device of X for torch inputs, numpy arrays for numpy inputs.  R is the recursion r_a = w_a - sum_j r_j (p_j^T w_a),
        not W (P^T W)^-1.  M <= 32; a handle with a reducer: PLS_HIP_ERR_UNSUPPORTED."""
        want = set(want)
        bad = want - set(_MISSING_OUT)
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"fit_missing: unknown output(s) {sorted(bad)}")
        if _is_torch(X):
            X = as_colmajor(X); Y = as_colmajor(Y, X.dtype)
            N, K = X.shape
            M = Y.shape[1]
            dev, f64 = X.device, torch.float64
            W = colmajor_empty(K, A, f64, dev, ld=K); P = colmajor_empty(K, A, f64, dev, ld=K)
            R = colmajor_empty(K, A, f64, dev, ld=K); Q = colmajor_empty(M, A, f64, dev, ld=M)
            T = colmajor_empty(N, A, X.dtype, dev)
            B = colmajor_empty(K, M, f64, dev, ld=K) if "B" in want else None
            iters = torch.empty(A, dtype=torch.int64, device=dev) if "iters" in want else None
            rc = self._lib.pls_hip_fit_missing(self.h, X.data_ptr() or None, _ld(X), Y.data_ptr() or None, _ld(Y), N, K, M, A, self._dt(X),
                                               L.MEM_DEVICE, W.data_ptr(), P.data_ptr(), Q.data_ptr(), R.data_ptr(), T.data_ptr(), _ld(T),
                                               B.data_ptr() if B is not None else None, iters.data_ptr() if iters is not None else None)
            L.check(rc, self.h)
            self._last_inputs = (X, Y)
        else:
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            X = _np_f(X, dt); Y = _np_f(Y, dt)
            N, K = X.shape
            M = Y.shape[1]
            W = np.zeros((K, A), order="F"); P = np.zeros((K, A), order="F")
            R = np.zeros((K, A), order="F"); Q = np.zeros((M, A), order="F")
            T = np.zeros((N, A), dtype=dt, order="F")
            B = np.zeros((K, M), order="F") if "B" in want else None
            iters = np.zeros(A, dtype=np.int64) if "iters" in want else None
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
            rc = self._lib.pls_hip_fit_missing(self.h, p(X), max(N, 1), p(Y), max(N, 1), N, K, M, A, L.F64 if dt == np.float64 else L.F32,
                                               L.MEM_HOST, p(W), p(P), p(Q), p(R), p(T), max(N, 1), p(B), p(iters))
            L.check(rc, self.h)
        full = dict(W=W, P=P, Q=Q, R=R, T=T, B=B, iters=iters)
        return {k: full[k] for k in _MISSING_OUT if k in want}

    @_on_handle_stream
    def cv_folds_missing(self, X, Y, A: int, test_idx, want_iters: bool = False):
        """Residuals of cross-validation folds of X whose NaN cells are missing values (pls_hip_cv_folds_missing): fold f is
        fit_missing on all rows but test_idx[f], scores_missing on the held-out rows, E_c = Y_test - S[:, :c] Q[:, :c]^T.
        test_idx: (num_folds, test_size).  Returns E with shape (M, nobs, A) as cv_folds does -- validation takes it unchanged --
        or (E, iters) with iters (num_folds, A) int64 when want_iters.  All folds of a round run in the same launches; the
        bits of a fold do not depend on the other folds.  M <= 32; a handle with a reducer: PLS_HIP_ERR_UNSUPPORTED."""
        idx = np.ascontiguousarray(np.asarray(test_idx, dtype=np.int64))
        if idx.ndim == 1:
            idx = idx[:, None]
        nf, ts = idx.shape
        if _is_torch(X):
            X = as_colmajor(X); Y = as_colmajor(Y, X.dtype)
            N, K = X.shape
            M = Y.shape[1]
            E = torch.empty((M, A, nf * ts), dtype=torch.float64, device=X.device)
            iters = torch.empty((nf, A), dtype=torch.int64, device=X.device) if want_iters else None
            rc = self._lib.pls_hip_cv_folds_missing(self.h, X.data_ptr() or None, _ld(X), Y.data_ptr() or None, _ld(Y), N, K, M, A,
                                                    idx.ctypes.data_as(ctypes.c_void_p), ts, nf, self._dt(X), L.MEM_DEVICE,
                                                    E.data_ptr(), iters.data_ptr() if want_iters else None)
            L.check(rc, self.h)
            E = E.permute(0, 2, 1)
        else:
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            X = _np_f(X, dt); Y = _np_f(Y, dt)
            N, K = X.shape
            M = Y.shape[1]
            E = np.zeros((M, A, nf * ts))
            iters = np.zeros((nf, A), dtype=np.int64) if want_iters else None
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
            rc = self._lib.pls_hip_cv_folds_missing(self.h, p(X), max(N, 1), p(Y), max(N, 1), N, K, M, A, p(idx), ts, nf,
                                                    L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, p(E), p(iters))
            L.check(rc, self.h)
            E = E.transpose(0, 2, 1)
        return (E, iters) if want_iters else E

    @_on_handle_stream
    def scores_missing(self, X, W, P):
        """Scores of rows, new or training, that may have missing cells (pls_hip_scores_missing): sequential deflation with
        the model's W and P (K, A).  (N, A) in the dtype of X.  On complete rows it equals xb(X, R)."""
        if _is_torch(X):
            X = as_colmajor(X)
            N, K = X.shape
            A = W.shape[1]
            Wc = colmajor_empty(K, A, torch.float64, X.device, ld=K).copy_(W)
            Pc = colmajor_empty(K, A, torch.float64, X.device, ld=K).copy_(P)
            S = colmajor_empty(N, A, X.dtype, X.device)
            rc = self._lib.pls_hip_scores_missing(self.h, X.data_ptr() or None, _ld(X), N, K, A, Wc.data_ptr(), Pc.data_ptr(),
                                                  self._dt(X), L.MEM_DEVICE, S.data_ptr(), _ld(S))
            L.check(rc, self.h)
            self._last_inputs = (X, Wc, Pc)
            return S
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); W = _np_f(W, np.float64); P = _np_f(P, np.float64)
        N, K = X.shape
        A = W.shape[1]
        S = np.zeros((N, A), dtype=dt, order="F")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.pls_hip_scores_missing(self.h, p(X), max(N, 1), N, K, A, p(W), p(P), L.F64 if dt == np.float64 else L.F32,
                                              L.MEM_HOST, p(S), max(N, 1))
        L.check(rc, self.h)
        return S

    @_on_handle_stream
    def x_diagnostics_missing(self, X, W, P, tvar=None, want=("Q", "T2", "ssx")):
        """X-space diagnostics of rows, new or training, that may have missing cells (pls_hip_x_diagnostics_missing): NaN in X
        marks a missing cell, W and P (K, A) are the model's own W and P as for scores_missing.  `want` picks from "Q" (Q
        residuals over the observed cells, N x A), "T2" (Hotelling T^2, N x A), "S" (scores, N x A in the dtype of X), "ssx"
        (A + 1: the sum of the observed x^2, then the sums of the Q columns), "sst" (A: column sums of squares of the scores),
        "nobs" (N, int64: observed cells per row); the result is a dict of those.  tvar (A) = t_a^T t_a / (n_train - 1) of the
        training scores; None means X IS the training data.  Torch CUDA tensors stay on the device, numpy arrays take the
        library's host path."""
        want = set(want)
        bad = want - {"Q", "T2", "S", "ssx", "sst", "nobs"}
        if bad:
            raise L.PlsHipError(L.ERR_INVALID, f"x_diagnostics_missing: unknown output(s) {sorted(bad)}")
        if _is_torch(X):
            X = as_colmajor(X)
            N, K = X.shape
            dev, f64 = X.device, torch.float64
            A = W.shape[1]
            Wc = colmajor_empty(K, A, f64, dev, ld=K).copy_(W)
            Pc = colmajor_empty(K, A, f64, dev, ld=K).copy_(P)
            tv = None if tvar is None else torch.as_tensor(tvar, dtype=f64, device=dev).contiguous()
            out = {}
            if "Q" in want: out["Q"] = colmajor_empty(N, A, f64, dev)
            if "T2" in want: out["T2"] = colmajor_empty(N, A, f64, dev)
            if "S" in want: out["S"] = colmajor_empty(N, A, X.dtype, dev)
            if "ssx" in want: out["ssx"] = torch.empty(A + 1, dtype=f64, device=dev)
            if "sst" in want: out["sst"] = torch.empty(A, dtype=f64, device=dev)
            if "nobs" in want: out["nobs"] = torch.empty(N, dtype=torch.int64, device=dev)
            ptr = lambda k: out[k].data_ptr() if k in out else None
            ldo = lambda k: _ld(out[k]) if k in out else 1
            rc = self._lib.pls_hip_x_diagnostics_missing(self.h, X.data_ptr() or None, _ld(X), N, K, A, Wc.data_ptr(), Pc.data_ptr(),
                                                         tv.data_ptr() if tv is not None else None, self._dt(X), L.MEM_DEVICE,
                                                         ptr("Q"), ldo("Q"), ptr("T2"), ldo("T2"), ptr("S"), ldo("S"), ptr("ssx"),
                                                         ptr("sst"), ptr("nobs"))
            L.check(rc, self.h)
            self._last_inputs = (X, Wc, Pc, tv)
            return out
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        X = _np_f(X, dt); W = _np_f(W, np.float64); P = _np_f(P, np.float64)
        N, K = X.shape
        A = W.shape[1]
        tv = None if tvar is None else np.ascontiguousarray(tvar, dtype=np.float64)
        out = {}
        if "Q" in want: out["Q"] = np.zeros((N, A), order="F")
        if "T2" in want: out["T2"] = np.zeros((N, A), order="F")
        if "S" in want: out["S"] = np.zeros((N, A), dtype=dt, order="F")
        if "ssx" in want: out["ssx"] = np.zeros(A + 1)
        if "sst" in want: out["sst"] = np.zeros(A)
        if "nobs" in want: out["nobs"] = np.zeros(N, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        ptr = lambda k: p(out[k]) if k in out else None
        rc = self._lib.pls_hip_x_diagnostics_missing(self.h, p(X), max(N, 1), N, K, A, p(W), p(P), p(tv) if tv is not None else None,
                                                     L.F64 if dt == np.float64 else L.F32, L.MEM_HOST, ptr("Q"), max(N, 1),
                                                     ptr("T2"), max(N, 1), ptr("S"), max(N, 1), ptr("ssx"), ptr("sst"), ptr("nobs"))
        L.check(rc, self.h)
        return out

    @_on_handle_stream
    def z_scores_missing(self, X, inplace: bool = False):
        """(Z, mean, sd, nobs) over the observed cells of each column (pls_hip_colwise_z_scores_missing): sd with nobs - 1,
        NaN kept in Z.  A column with fewer than two observed cells, or a constant one, is NaN throughout."""
        if _is_torch(X):
            X = as_colmajor(X)
            N, K = X.shape
            Z = X if inplace else colmajor_empty(N, K, X.dtype, X.device)
            mean = torch.empty(K, dtype=torch.float64, device=X.device)
            sd = torch.empty(K, dtype=torch.float64, device=X.device)
            nobs = torch.empty(K, dtype=torch.int64, device=X.device)
            rc = self._lib.pls_hip_colwise_z_scores_missing(self.h, X.data_ptr() or None, _ld(X), N, K, self._dt(X), L.MEM_DEVICE,
                                                            Z.data_ptr(), _ld(Z), mean.data_ptr(), sd.data_ptr(), nobs.data_ptr())
            L.check(rc, self.h)
            self._last_inputs = (X,)
            return Z, mean, sd, nobs
        dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
        Xf = _np_f(X, dt)
        if inplace and Xf is not X:
            raise L.PlsHipError(L.ERR_INVALID, "z_scores_missing: inplace needs a column-major array of float32 or float64")
        N, K = Xf.shape
        Z = Xf if inplace else np.zeros((N, K), dtype=dt, order="F")
        mean = np.zeros(K); sd = np.zeros(K); nobs = np.zeros(K, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = self._lib.pls_hip_colwise_z_scores_missing(self.h, p(Xf), max(N, 1), N, K, L.F64 if dt == np.float64 else L.F32, L.MEM_HOST,
                                                        p(Z), max(N, 1), p(mean), p(sd), p(nobs))
        L.check(rc, self.h)
        return Z, mean, sd, nobs

    @_on_handle_stream
    def permutation_test(self, X, Y, A: int, nperm: int, perms=None, seed: int = 0, max_bytes: int = 1 << 30, cv=None):
        """Response-permutation (Y-randomisation) test: problem 0 is Y itself, problem b is Y[perms[b-1]] (rows permuted,
        the M responses of a row together), all fitted against the same X by fit_batch.  perms: (nperm, N) int64; drawn
        with numpy.random.default_rng(seed).permutation when not given.  The rows are gathered by the array library where
        the data lives, in chunks whose Ys stays under max_bytes.  Returns dict(r2y (M, A), r2y_perm (nperm, M, A),
        p (M, A), perms): cumulative R^2 Y per component count, and p = (1 + #{perm >= real}) / (nperm + 1).
        cv: an index array (num_folds, test_size) of held-out rows as cv_folds takes it -- the test then also cross-validates
        every problem over these folds (cv_press_batch, chunk by chunk on the same Ys) and the result gains q2y (M, A),
        q2y_perm (nperm, M, A) and p_q2: Q^2 Y = 1 - PRESS / ssy per component count and its permutation p-value.  R^2 Y of a
        model with many predictors is close to 1 under permutation too; Q^2 Y is the figure to read.
        A handle with a reducer raises ValueError: a permutation moves rows across ranks -- sharded callers build Ys
        themselves and call fit_batch."""
        if self._has_reducer():
            raise ValueError("permutation_test on a row-sharded handle: a permutation moves rows across ranks; "
                             "build Ys yourself and call fit_batch")
        on_dev = _is_torch(X)
        if on_dev:
            Y2 = Y if Y.dim() == 2 else Y[:, None]
        else:
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            X = _np_f(X, dt); Y2 = _np_f(Y, dt)
        N, M = Y2.shape
        if perms is None:
            rng = np.random.default_rng(seed)
            perms = np.stack([rng.permutation(N) for _ in range(nperm)]) if nperm else np.zeros((0, N), dtype=np.int64)
        perms = np.ascontiguousarray(np.asarray(perms, dtype=np.int64)).reshape(-1, N)
        nperm = perms.shape[0]
        es = 4 if (Y2.dtype == (torch.float32 if on_dev else np.float32)) else 8
        chunk = max(1, int(max_bytes) // max(1, N * M * es))
        r2, q2 = [], []
        for b0 in range(0, nperm + 1, chunk):  # problem index 0 = the identity
            b1 = min(nperm + 1, b0 + chunk)
            rows = [np.arange(N, dtype=np.int64)] if b0 == 0 else []
            rows += [perms[b - 1] for b in range(max(b0, 1), b1)]
            idx = np.concatenate(rows)
            nb = b1 - b0
            if on_dev:
                g = Y2[torch.as_tensor(idx, device=Y2.device)]          # (nb * N, M), problem-major
                Ys = colmajor_empty(N, nb * M, Y2.dtype, Y2.device)
                Ys.copy_(g.reshape(nb, N, M).permute(1, 0, 2).reshape(N, nb * M))
            else:
                Ys = np.asfortranarray(Y2[idx].reshape(nb, N, M).transpose(1, 0, 2).reshape(N, nb * M))
            o = self.fit_batch(X, Ys, M, A, want=("Q", "tt", "ssy"))
            part = r2y_by_components(o["Q"], o["tt"], o["ssy"])
            r2.append(part.cpu().numpy() if on_dev else part)
            if cv is not None:
                o = self.cv_press_batch(X, Ys, M, A, cv, want=("PRESS", "ssy"))
                part = q2_by_components(o["PRESS"], o["ssy"])
                q2.append(part.cpu().numpy() if on_dev else part)
        r2 = np.concatenate(r2, axis=0)
        res = dict(r2y=r2[0], r2y_perm=r2[1:], p=permutation_pvalues(r2[0], r2[1:]), perms=perms)
        if cv is not None:
            q2 = np.concatenate(q2, axis=0)
            res.update(q2y=q2[0], q2y_perm=q2[1:], p_q2=permutation_pvalues(q2[0], q2[1:]))
        return res

    def _has_reducer(self) -> bool:
        on, rank, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.check(self._lib.pls_hip_get_reducer(self.h, ctypes.byref(on), ctypes.byref(rank), ctypes.byref(n)), self.h)
        return bool(on.value)

    @_on_handle_stream
    def synth_x(self, row0: int, nrows: int, K: int, seed: int, dtype=None, device=None):
        dtype = dtype or torch.float64
        X = colmajor_empty(nrows, K, dtype, device or f"cuda:{self.device}")
        L.check(self._lib.pls_hip_synth_x(self.h, X.data_ptr(), _ld(X), row0, nrows, K, seed,
                                          L.F64 if dtype == torch.float64 else L.F32), self.h)
        return X

    @_on_handle_stream
    def synth_y(self, row0: int, nrows: int, M: int, seed: int, dtype=None, device=None):
        dtype = dtype or torch.float64
        Y = colmajor_empty(nrows, M, dtype, device or f"cuda:{self.device}")
        L.check(self._lib.pls_hip_synth_y(self.h, Y.data_ptr(), _ld(Y), row0, nrows, M, seed,
                                          L.F64 if dtype == torch.float64 else L.F32), self.h)
        return Y


# ---------------------------------------------------------------------------------------------
# one process, several GPUs (include/pls_hip.h: pls_hip_group) -- what the C++ PLS::Model drives
# ---------------------------------------------------------------------------------------------

class Group:
    """n member handles, one per entry of `devices` (an ordinal may repeat: virtual shards on one GPU), one host
    thread per member inside the library, row-sharded resident matrices, in-process fixed-order all-reduce.
    Host (numpy) matrices in, host results out."""

    def __init__(self, devices):
        self._lib = L.lib()
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        g = ctypes.c_void_p()
        L.check(self._lib.pls_hip_group_create(ctypes.byref(g), len(devices), devs))
        self.g = g
        self.n = len(devices)
        self.devices = [int(d) for d in devices]  # member r lives on device self.devices[r]

    def _check(self, rc):
        if rc != L.OK:
            raw = self._lib.pls_hip_group_last_error(self.g)
            raise L.PlsHipError(rc, raw.decode("utf-8", "replace") if raw else "")

    def close(self):
        if getattr(self, "g", None):
            self._lib.pls_hip_group_destroy(self.g)
            self.g = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int):
        self._check(self._lib.pls_hip_group_set_option(self.g, opt, int(value)))

    @property
    def exchange(self) -> str:
        """'device': the members push their partial sums into each other's inboxes (no host in a collective);
        'host': the host-synchronised exchange (members sharing a GPU, or a single member)"""
        return "device" if self._lib.pls_hip_group_exchange(self.g) else "host"

    def upload(self, a, dtype=np.float64):
        a = _np_f(a, dtype)
        m = ctypes.c_void_p()
        self._check(self._lib.pls_hip_group_upload(self.g, a.ctypes.data_as(ctypes.c_void_p), max(a.shape[0], 1), a.shape[0],
                                                   a.shape[1], L.F64 if dtype == np.float64 else L.F32, ctypes.byref(m)))
        return m

    def upload_xy(self, X, Y, dtype=np.float64):
        """X and Y of one data set; X^T X and X^T Y are accumulated on the matrix cores while X streams in and kept
        with the pair for fits under ALGO_AUTO / ALGO_GRAM / KERNEL_TYPE2"""
        X = _np_f(X, dtype); Y = _np_f(Y, dtype)
        mx, my = ctypes.c_void_p(), ctypes.c_void_p()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.pls_hip_group_upload_xy(self.g, p(X), max(X.shape[0], 1), p(Y), max(Y.shape[0], 1), X.shape[0],
                                                      X.shape[1], Y.shape[1], L.F64 if dtype == np.float64 else L.F32,
                                                      ctypes.byref(mx), ctypes.byref(my)))
        return mx, my

    def alloc(self, N: int, K: int, dtype=np.float64):
        m = ctypes.c_void_p()
        self._check(self._lib.pls_hip_group_alloc(self.g, N, K, L.F64 if dtype == np.float64 else L.F32, ctypes.byref(m)))
        return m

    def member_handle(self, r: int):
        h = ctypes.c_void_p()
        L.check(self._lib.pls_hip_group_handle(self.g, r, ctypes.byref(h)))
        return h

    def block(self, m, r: int):
        """(device pointer, ld, row0, nrows) of member r's block of a resident matrix"""
        ptr, ld, r0, nr = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.pls_hip_matrix_block(m, r, ctypes.byref(ptr), ctypes.byref(ld), ctypes.byref(r0), ctypes.byref(nr)))
        return ptr, int(ld.value), int(r0.value), int(nr.value)

    def synth(self, N: int, cols: int, seed: int, which: str = "x", dtype=np.float64):
        """resident N x cols matrix of the synthetic generator (DESIGN.md "Synthetic inputs"), every member generating
        its own rows on its device -- no host copy (config 5 at its own size: 137 GB)"""
        m = self.alloc(N, cols, dtype)
        fn = self._lib.pls_hip_synth_x if which == "x" else self._lib.pls_hip_synth_y
        for r in range(self.n):
            h = self.member_handle(r)
            ptr, ld, r0, nr = self.block(m, r)
            L.check(fn(h, ptr, ld, r0, nr, cols, seed, L.F64 if dtype == np.float64 else L.F32), h)
        for r in range(self.n):
            L.check(self._lib.pls_hip_synchronize(self.member_handle(r)))
        return m

    def gram(self, Am, Bm):
        """A^T B (cols x cols, numpy) of two resident matrices with the same row partition: each member's block product
        on its device (pls_hip_xty), summed on the host.  Size-independent checks on matrices that never leave the GPUs."""
        ka, kb = self.shape(Am)[1], self.shape(Bm)[1]
        import torch
        total = np.zeros((ka, kb))
        for r in range(self.n):
            h = self.member_handle(r)
            pa, lda, _, nr = self.block(Am, r)
            pb, ldb, _, _ = self.block(Bm, r)
            if nr == 0:
                continue
            out = torch.empty((kb, ka), dtype=torch.float64, device=f"cuda:{self.devices[r]}")  # column-major ka x kb, on the member's GPU
            L.check(self._lib.pls_hip_xty(h, pa, lda, pb, ldb, nr, ka, kb, L.F64 if self.shape(Am)[2] == np.float64 else L.F32,
                                          out.data_ptr()), h)
            L.check(self._lib.pls_hip_synchronize(h), h)
            total += out.cpu().numpy().T
        return total

    def shape(self, m):
        n, k, dt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        L.check(self._lib.pls_hip_matrix_shape(m, ctypes.byref(n), ctypes.byref(k), ctypes.byref(dt)))
        return int(n.value), int(k.value), (np.float64 if dt.value == L.F64 else np.float32)

    def blocks(self, m):
        """[(row0, nrows)] of the members"""
        out = []
        for r in range(self.n):
            r0, nr = ctypes.c_int64(), ctypes.c_int64()
            L.check(self._lib.pls_hip_matrix_block(m, r, None, None, ctypes.byref(r0), ctypes.byref(nr)))
            out.append((int(r0.value), int(nr.value)))
        return out

    def download(self, m, col0: int = 0, ncols: int | None = None):
        N, K, dt = self.shape(m)
        ncols = K - col0 if ncols is None else ncols
        out = np.zeros((N, ncols), dtype=dt, order="F")
        self._check(self._lib.pls_hip_group_download(self.g, m, col0, ncols, out.ctypes.data_as(ctypes.c_void_p), N))
        return out

    def free(self, m):
        self._check(self._lib.pls_hip_group_free(self.g, m))

    def fit(self, X, Y, A: int, method: int = KERNEL_TYPE1):
        """X, Y: resident matrices.  Returns dict(W,P,Q,R,B numpy; T resident matrix or None)."""
        N, K, dt = self.shape(X)
        M = self.shape(Y)[1]
        W = np.zeros((K, A), order="F"); P = np.zeros((K, A), order="F"); R = np.zeros((K, A), order="F")
        Q = np.zeros((M, A), order="F"); B = np.zeros((K, M), order="F")
        T = self.alloc(N, A, dt) if method == KERNEL_TYPE1 else None
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.pls_hip_group_fit(self.g, X, Y, A, method, p(W), p(P), p(Q), p(R), T, p(B)))
        return dict(W=W, P=P, Q=Q, R=R, T=T, B=B)

    def xb(self, X, Bm):
        N, K, dt = self.shape(X)
        Bm = _np_f(Bm, np.float64)
        out = self.alloc(N, Bm.shape[1], dt)
        self._check(self._lib.pls_hip_group_xb(self.g, X, Bm.ctypes.data_as(ctypes.c_void_p), K, Bm.shape[1], out))
        return out

    def model_sse(self, X, Y, R, Q):
        R = _np_f(R, np.float64); Q = _np_f(Q, np.float64)
        M, A = Q.shape
        sse = np.zeros((M, A), order="F")
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self._lib.pls_hip_group_model_sse(self.g, X, Y, A, p(R), p(Q), p(sse)))
        return sse

    def x_diagnostics(self, X, R, P, tvar=None, want=("Q", "T2", "ssx")):
        """pls_hip_group_x_diagnostics on a resident X: dict with "Q", "T2", "S" as resident N x A matrices and "ssx", "sst"
        as numpy vectors, whichever `want` names (see Handle.x_diagnostics)"""
        want = set(want)
        N, K, dt = self.shape(X)
        R = _np_f(R, np.float64); P = _np_f(P, np.float64)
        A = R.shape[1]
        tv = None if tvar is None else np.ascontiguousarray(tvar, dtype=np.float64)
        out = {}
        if "Q" in want: out["Q"] = self.alloc(N, A, np.float64)
        if "T2" in want: out["T2"] = self.alloc(N, A, np.float64)
        if "S" in want: out["S"] = self.alloc(N, A, dt)
        if "ssx" in want: out["ssx"] = np.zeros(A + 1)
        if "sst" in want: out["sst"] = np.zeros(A)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        vec = lambda k: p(out[k]) if k in out else None
        self._check(self._lib.pls_hip_group_x_diagnostics(self.g, X, A, p(R), p(P), p(tv) if tv is not None else None,
                                                          out.get("Q"), out.get("T2"), out.get("S"), vec("ssx"), vec("sst")))
        return out

    def fit_batch(self, X, Ys, M: int, A: int, want=("B", "Q", "tt", "ssy")):
        """pls_hip_group_fit_batch on resident X (N x K) and Ys (N x nprob*M): numpy outputs as Handle.fit_batch names them"""
        want = _batch_want(want)
        N, K, _ = self.shape(X)
        C = self.shape(Ys)[1]
        if M < 1 or C % M:
            raise L.PlsHipError(L.ERR_INVALID, "fit_batch: the columns of Ys are not a multiple of M")
        nprob = C // M
        shp = _batch_shapes(K, M, A, nprob)
        out = {k: np.zeros(shp[k]) for k in _BATCH_OUT if k in want}
        ptr = lambda k: out[k].ctypes.data_as(ctypes.c_void_p) if k in out else None
        self._check(self._lib.pls_hip_group_fit_batch(self.g, X, Ys, M, A, ptr("R"), ptr("Q"), ptr("tt"), ptr("B"), ptr("ssy")))
        return {k: _batch_view(k, v) for k, v in out.items()}

    def cv_folds(self, X, Y, A: int, test_idx):
        idx = np.ascontiguousarray(np.asarray(test_idx, dtype=np.int64))
        if idx.ndim == 1:
            idx = idx[:, None]
        nf, ts = idx.shape
        M = self.shape(Y)[1]
        E = np.zeros((M, A, nf * ts))
        self._check(self._lib.pls_hip_group_cv_folds(self.g, X, Y, A, idx.ctypes.data_as(ctypes.c_void_p), ts, nf,
                                                     E.ctypes.data_as(ctypes.c_void_p)))
        return E.transpose(0, 2, 1)


# ---------------------------------------------------------------------------------------------
# PLS::Model
# ---------------------------------------------------------------------------------------------

class Model:
    """Mirror of `PLS::Model` (reference include/PLS/pls.h:184-266).

    Model(X, Y, algorithm=KERNEL_TYPE1, max_components=None) fits immediately, like the
    reference's data-taking constructors (src/pls.cpp:340-359): max_components defaults to
    X.cols().  X: N x K, Y: N x M.  torch CUDA tensors stay on the device; numpy arrays go
    through the library's host path.
    """

    def __init__(self, X, Y, algorithm: int = KERNEL_TYPE1, max_components: int | None = None, *,
                 handle: Handle | None = None, missing: bool = False):
        self.handle = handle or Handle()
        self._on_device = _is_torch(X)
        K = X.shape[1]
        self.A = int(K if max_components is None else max_components)  # src/pls.cpp:356-359
        self.method = algorithm
        self.W = self.P = self.R = self.Q = self.T = None
        self._X, self._Y = X, Y  # the reference keeps _X, _Y for its cross-validation methods (pls.h:250)
        self._missing = False  # plsr_missing sets it: cross-validation then treats NaN in X as missing cells too
        if missing:  # NaN in X marks a missing cell (plsr_missing)
            self.plsr_missing(X, Y)
        else:
            self.plsr(X, Y, algorithm)

    # void plsr(const Mat2D&, const Mat2D&, const METHOD&)  include/PLS/pls.h:199
    def plsr(self, X, Y, algorithm: int = KERNEL_TYPE1):
        self.method = algorithm
        self._missing = False
        if _is_torch(X):
            out = self.handle.fit_device(X, Y, self.A, algorithm, want_B=False)
        else:
            dt = np.float32 if np.asarray(X).dtype == np.float32 else np.float64
            out = self.handle.fit_host(X, Y, self.A, algorithm, dtype=dt)
        self.W, self.P, self.Q, self.R, self.T = (out[k] for k in "WPQRT")
        self._tvar_cache = None

    def plsr_missing(self, X, Y):
        """plsr for an X whose NaN cells are missing values (Handle.fit_missing): fills the members
        plsr fills, so scores, coefficients, fitted_values and loadingsX/Y work unchanged on complete new data; rows with
        missing cells go through scores_missing / fitted_values_missing.  Model(X, Y, missing=True) fits this way."""
        self.method = KERNEL_TYPE1
        self._missing = True
        out = self.handle.fit_missing(X, Y, self.A, want=("W", "P", "Q", "R", "T", "iters"))
        self.W, self.P, self.Q, self.R, self.T = (out[k] for k in "WPQRT")
        self.iters = out["iters"]
        self._tvar_cache = None

    def scores_missing(self, X_new, comp: int | None = None):
        """scores of rows that may have missing cells: sequential deflation with W and P (equals scores() on complete rows)"""
        c = self._comp(comp)
        return self.handle.scores_missing(X_new, self.W[:, :c], self.P[:, :c])

    def fitted_values_missing(self, X_new, comp: int | None = None):
        """fitted values of rows that may have missing cells: scores_missing(X_new, comp) Q[:, :comp]^T"""
        c = self._comp(comp)
        Qc = self.Q[:, :c]
        return self.handle.xb(self.scores_missing(X_new, c), Qc.t() if _is_torch(Qc) else Qc.T)

    def _comp(self, comp):
        comp = self.A if comp is None else int(comp)
        if not (0 <= comp <= self.A):  # assert (A >= comp): src/pls.cpp:440, :445
            raise L.PlsHipError(L.ERR_INVALID, f"comp={comp} exceeds the fitted A={self.A}")
        return comp

    # const Mat2Dc scores(const Mat2D& X_new, size_t comp)   src/pls.cpp:439-442
    def scores(self, X_new, comp: int | None = None):
        c = self._comp(comp)
        return self.handle.xb(X_new, self.R[:, :c])

    # declared but never defined by the reference (include/PLS/pls.h:207-211); the natural
    # definitions, SURVEY.md section 8(b)
    def loadingsX(self, comp: int | None = None):
        return self.P[:, :self._comp(comp)]

    def loadingsY(self, comp: int | None = None):
        return self.Q[:, :self._comp(comp)]

    # const Mat2Dc coefficients(size_t comp)   src/pls.cpp:444-447
    def coefficients(self, comp: int | None = None):
        return self.handle.coefficients(self.R, self.Q, self._comp(comp))

    # const Mat2D fitted_values(const Mat2D& X, size_t comp)   src/pls.cpp:449-451
    def fitted_values(self, X, comp: int | None = None):
        return self.handle.xb(X, self.coefficients(comp))

    # residuals / SSE / explained_variance: src/pls.cpp:453-467 (thin host arithmetic on N x M)
    def residuals(self, X, Y, comp: int | None = None):
        fv = self.fitted_values(X, comp)
        if _is_torch(Y):
            Y2 = Y if Y.dim() == 2 else Y[:, None]
            return Y2.to(fv.dtype) - fv
        return _np_f(Y, fv.dtype) - fv

    def SSE(self, X, Y, comp: int | None = None):
        r = self.residuals(X, Y, comp)
        return (r * r).sum(0)

    # ---- cross-validation (reference include/PLS/pls.h:235-241, src/pls.cpp:469-549) -------------------
    # Each returns the residual tensor E of shape (M, nobs, A): E[m] is Residual.errors()[m].
    def cv_LOO(self):
        """leave-one-out: fold i refits on all rows but i (all folds in one batched device call).  The handle's plan decides
        the route (Handle.cv_folds): under ALGO_DUAL every fold runs from one X X^T."""
        n = self._X.shape[0]
        return self._cv_folds(self._X, self._Y, self.A, np.arange(n)[:, None])

    def cv_LSO(self, test_fraction: float, num_trials: int, rng=None):
        """leave-some-out: num_trials random splits with round(test_fraction*N) held-out rows each.
        The reference draws its splits from std::shuffle on a std::mt19937 (src/pls.cpp:218-227);
        here they come from a numpy Generator (pass one for reproducibility).  The handle's plan decides the route
        (Handle.cv_folds): under ALGO_DUAL every fold runs from one X X^T."""
        n = self._X.shape[0]
        ts = int(test_fraction * n + 0.5)
        if ts == 0 or ts == n:
            raise L.PlsHipError(L.ERR_INVALID, "empty train or test split")
        rng = np.random.default_rng() if rng is None else rng
        idx = np.stack([rng.permutation(n)[:ts] for _ in range(num_trials)])
        return self._cv_folds(self._X, self._Y, self.A, idx)

    def _cv_folds(self, X, Y, A, idx):
        """a model fitted with missing=True / plsr_missing cross-validates with the missing cells skipped (Handle.cv_folds_missing)"""
        return (self.handle.cv_folds_missing if self._missing else self.handle.cv_folds)(X, Y, A, idx)

    def cv_NEW_DATA(self, X_new, Y_new):
        """residuals on data outside the fit for 1..A components (src/pls.cpp:494-509); no refit.  A model fitted with
        missing=True / plsr_missing takes the scores from scores_missing: X_new may have missing cells"""
        S = self.scores_missing(X_new) if self._missing else self.scores(X_new)
        if _is_torch(S):
            Y2 = (Y_new if Y_new.dim() == 2 else Y_new[:, None]).to(torch.float64)
            fit = torch.cumsum(S.to(torch.float64)[:, :, None] * self.Q.t()[None, :, :], dim=1)  # (N, A, M)
            return (Y2[:, None, :] - fit).permute(2, 0, 1)
        Y2 = _np_f(Y_new, np.float64)
        fit = np.cumsum(np.asarray(S, dtype=np.float64)[:, :, None] * np.asarray(self.Q).T[None, :, :], axis=1)
        return (Y2[:, None, :] - fit).transpose(2, 0, 1)

    # ---- model selection (reference include/PLS/pls.h:143-150, src/pls.cpp:235-305) ----------------------
    # E is what cv_LOO / cv_LSO / cv_NEW_DATA return.
    def validation(self, E, out_type: int):
        """M x A: RESS = sum of squared residuals per (response, component count), MSE = RESS / nobs"""
        if out_type not in (RESS, MSE):
            raise L.PlsHipError(L.ERR_INVALID, f"out_type={out_type}: RESS or MSE")
        press = self.handle.validation(E)[0]
        return press / E.shape[-2] if out_type == MSE else press

    def optimal_num_components(self, E, alpha: float = 0.1):
        """per response: the smallest number of components whose errors a Wilcoxon signed-rank test (level alpha) cannot
        tell from those at the PRESS minimum; component counts from 1 (src/pls.cpp:265-289).  Ties in |del| rank in row
        order."""
        _, _, probw, ref = self.handle.validation(E)
        if _is_torch(probw):
            probw, ref = probw.cpu().numpy(), ref.cpu().numpy()
        return pick_components(probw, ref, alpha)

    def print_validation(self, E, label: str, out_type: int = MSE, file=None):
        """the lines of print_validation (src/pls.cpp:291-305); `label` is Residual::method() there ("LOO", "LSO", ...)"""
        file = sys.stderr if file is None else file
        em = self.validation(E, out_type)
        em = em.cpu().numpy() if _is_torch(em) else np.asarray(em)
        name = "RMSE " if out_type == MSE else "PRESS "
        if out_type == MSE:
            em = np.sqrt(em)
        txt = [[f"{v:.6g}" for v in row] for row in em]
        wd = max(len(t) for row in txt for t in row)
        print(f"{label} Validation:", file=file)
        print(f"{name} Matrix (rows = Y variable; cols = # of components):", file=file)
        print("\n".join(" ".join(t.rjust(wd) for t in row) for row in txt), file=file)
        print("Optimal number of components (by Y variable):\t" +
              " ".join(str(int(b)) for b in self.optimal_num_components(E)), file=file)

    # ---- X-space diagnostics (no counterpart in the reference) --------------------------------------------
    def _tvar(self):
        """t_a^T t_a / (N - 1) of the training scores: from T when the fit produced it, else (KERNEL_TYPE2) from one pass
        over the training data"""
        if getattr(self, "_tvar_cache", None) is None:
            n = self._X.shape[0]
            if self.T is not None:
                T = self.T.to(torch.float64) if _is_torch(self.T) else np.asarray(self.T, dtype=np.float64)
                self._tvar_cache = (T * T).sum(0) / (n - 1)
            else:
                sst = self.handle.x_diagnostics(self._X, self.R, self.P, want=("sst",))["sst"]
                self._tvar_cache = sst / (n - 1)
        return self._tvar_cache

    def x_diagnostics(self, X_new=None):
        """dict(Q, T2: N x A; R2X: A) for 1..A components: the Q residual (squared distance of a row from the model plane),
        Hotelling's T^2 (its distance from the centre inside the plane, scaled by the variance of the TRAINING scores) and
        the share of sum X^2 the components reproduce.  X_new=None: the training data.  New rows must be preprocessed as
        the training data was (the model does no centring of its own).  A model fitted with missing=True / plsr_missing takes
        NaN in X for missing cells (Handle.x_diagnostics_missing with the model's W and P): Q and R2X are then over the observed
        cells, and the dict has "nobs", the observed cells of each row, as well."""
        X = self._X if X_new is None else X_new
        tv = self._tvar()
        if _is_torch(X) != _is_torch(tv):
            tv = tv.cpu().numpy() if _is_torch(tv) else torch.as_tensor(tv, device=X.device)
        if self._missing:
            W, P = self.W, self.P
            if _is_torch(X) != _is_torch(W):
                W, P = ((W.cpu().numpy(), P.cpu().numpy()) if _is_torch(W) else
                        (torch.as_tensor(np.asarray(W), device=X.device), torch.as_tensor(np.asarray(P), device=X.device)))
            out = self.handle.x_diagnostics_missing(X, W, P, tvar=tv, want=("Q", "T2", "ssx", "nobs"))
            ssx = out["ssx"]
            return dict(Q=out["Q"], T2=out["T2"], R2X=1.0 - ssx[1:] / ssx[0], nobs=out["nobs"])
        R, P = self.R, self.P
        if _is_torch(X) != _is_torch(R):
            R, P = ((R.cpu().numpy(), P.cpu().numpy()) if _is_torch(R) else
                    (torch.as_tensor(np.asarray(R), device=X.device), torch.as_tensor(np.asarray(P), device=X.device)))
        out = self.handle.x_diagnostics(X, R, P, tvar=tv, want=("Q", "T2", "ssx"))
        ssx = out["ssx"]
        return dict(Q=out["Q"], T2=out["T2"], R2X=1.0 - ssx[1:] / ssx[0])

    # ---- variable-space diagnostics (no counterpart in the reference) -------------------------------------
    def vip(self):
        """K x A: the variable importance in projection of every predictor for 1..A components (Handle.var_diagnostics);
        sum_k VIP[k, c-1]^2 = K, "VIP > 1" is the usual selection rule.  t_a^T t_a comes from T when the fit produced it
        (KERNEL_TYPE1, missing=True -- sound for a missing-value model, whose T are the scores of its own fit): no pass over X.
        After KERNEL_TYPE2 it comes from the scores of the training data, one pass."""
        if self.T is not None:
            T = self.T.to(torch.float64) if _is_torch(self.T) else np.asarray(self.T, dtype=np.float64)
            return self.handle.var_diagnostics(None, W=self.W, Q=self.Q, tt=(T * T).sum(0), want=("VIP",))["VIP"]
        return self.handle.var_diagnostics(self._X, W=self.W, R=self.R, Q=self.Q, want=("VIP",))["VIP"]

    def r2x_by_variable(self, X_new=None):
        """K x A: the share of sum_i X[i,k]^2 of predictor k that 1..A components reproduce, 1 - ssxk[:, c] / ssxk[:, 0] of
        Handle.var_diagnostics.  X_new=None: the training data.  New rows must be preprocessed as the training data was.  A
        model fitted with missing=True / plsr_missing: PLS_HIP_ERR_UNSUPPORTED (NaN cells are outside the column sweep)."""
        if self._missing:
            raise L.PlsHipError(L.ERR_UNSUPPORTED, "r2x_by_variable: not for a model fitted with missing=True")
        X = self._X if X_new is None else X_new
        R, P = self.R, self.P
        if _is_torch(X) != _is_torch(R):
            R, P = ((R.cpu().numpy(), P.cpu().numpy()) if _is_torch(R) else
                    (torch.as_tensor(np.asarray(R), device=X.device), torch.as_tensor(np.asarray(P), device=X.device)))
        ssxk = self.handle.var_diagnostics(X, R=R, P=P, want=("ssxk",))["ssxk"]
        return 1.0 - ssxk[:, 1:] / ssxk[:, :1]

    def permutation_test(self, nperm: int, perms=None, seed: int = 0, max_bytes: int = 1 << 30, cv=None):
        """Handle.permutation_test on the model's own training data with the model's number of components: is the R^2 Y
        of this model better than what the same X explains of row-permuted responses?  cv (num_folds, test_size): the
        cross-validated Q^2 Y of the real and the permuted models as well (q2y, q2y_perm, p_q2)."""
        return self.handle.permutation_test(self._X, self._Y, self.A, nperm, perms=perms, seed=seed, max_bytes=max_bytes, cv=cv)

    def _resample(self, Wt, kind):
        o = self.handle.fit_resampled(self._X, self._Y, self.A, Wt, want=("B0", "Bmean", "Bm2"))
        return dict(B0=o["B0"], Bmean=o["Bmean"], se=resample_se(o["Bm2"], Wt.shape[1], kind))

    def bootstrap(self, nrep: int, seed: int = 0):
        """dict(B0, Bmean, se), each K x M: the coefficients of the model's training data, their mean over nrep bootstrap
        draws of its rows (bootstrap_weights(N, nrep, seed)) and the bootstrap standard error of every coefficient, with
        the model's number of components.  Under ALGO_DUAL every draw runs from one X X^T (Handle.fit_resampled)."""
        return self._resample(bootstrap_weights(self._X.shape[0], nrep, seed), "bootstrap")

    def jackknife(self, groups=None):
        """dict(B0, Bmean, se), each K x M: the delete-a-group jack-knife of the coefficients over the cross-validation
        segments (Martens' uncertainty test) -- leave-one-out by default, otherwise an array of N group labels
        (jackknife_weights)."""
        return self._resample(jackknife_weights(self._X.shape[0], groups), "jackknife")

    def explained_variance_by_components(self, X, Y):
        """(EV, SSE), each M x A: what print_explained_variance (src/pls.cpp:551-562) reports for
        ncomp = 1..A, from one X*R pass and one sweep over the scores instead of A X*B passes.
        Device tensors only."""
        X = as_colmajor(X)
        Y2 = as_colmajor(Y if Y.dim() == 2 else Y[:, None], X.dtype)
        N, K = X.shape
        M = Y2.shape[1]
        sse = colmajor_empty(M, self.A, torch.float64, X.device, ld=M)
        L.check(L.lib().pls_hip_model_sse(self.handle.h, X.data_ptr(), _ld(X), Y2.data_ptr(), _ld(Y2), N, K, M,
                                          self.A, self.R.data_ptr(), self.Q.data_ptr(), self.handle._dt(X),
                                          L.MEM_DEVICE, sse.data_ptr()), self.handle.h)
        Yd = Y2.to(torch.float64)
        sst = ((Yd - Yd.mean(0, keepdim=True)) ** 2).sum(0) if Yd.shape[0] >= 2 else torch.zeros(Yd.shape[1], device=Yd.device)
        return 1.0 - sse / sst[:, None], sse

    def explained_variance(self, X, Y, comp: int | None = None):
        sse = self.SSE(X, Y, comp)
        Y2 = Y if Y.ndim == 2 else Y[:, None]
        if _is_torch(Y2):
            Yd = Y2.to(torch.float64)
            sst = ((Yd - Yd.mean(0, keepdim=True)) ** 2).sum(0) if Yd.shape[0] >= 2 else torch.zeros_like(sse)
            return 1.0 - sse.to(torch.float64) / sst
        Yd = np.asarray(Y2, dtype=np.float64)
        sst = ((Yd - Yd.mean(0)) ** 2).sum(0) if Yd.shape[0] >= 2 else np.zeros(Yd.shape[1])  # SST: :69-73
        return 1.0 - np.asarray(sse, dtype=np.float64) / sst
