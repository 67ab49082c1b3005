"""Host-memory calls against device-memory calls of the same staged layout.

Every entry point of include/pls_hip.h that takes `mem` stages a host-memory call in device buffers of the handle with a
leading dimension of its own rule (host_entry.hpp: even, quad, exact) and then runs what a device-memory call runs.  So a
host-memory call must return, bit for bit, what a device-memory call returns whose matrices have that leading dimension --
on the same handle, with the same options.  N = 37, 38, 40 pads by 0, 1 and 3 rows under the rules.

CASES and run_case() are also what tools/host_entry_trace.py drives (one SHA-256 per call, profiles/host_stage).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, A = 9, 3
NS = (37, 38, 40)
FOLDS, TS = 3, 5
NPROB, NREP = 3, 4

LD = {
    "even": lambda n: n + (n & 1),     # 16-byte columns of fp64
    "quad": lambda n: n + (-n) % 4,    # 16-byte columns of either type
    "exact": lambda n: n,
}

# entry -> (leading-dimension rule of its host staging, the response counts it is run with)
ENTRIES = {
    "fit": ("even", (2, 1)),
    "fit_type2": ("even", (2, 1)),
    "coefficients": ("exact", (2,)),
    "xb": ("even", (2, 1)),
    "model_sse": ("even", (2, 1)),
    "x_diagnostics": ("even", (2,)),
    "cv_folds": ("quad", (2, 1)),
    "cv_folds_sharded": ("quad", (2, 1)),
    "fit_batch": ("quad", (2, 1)),
    "fit_resampled": ("quad", (2, 1)),
    "cv_press_batch": ("quad", (2, 1)),
    "validation": ("exact", (2,)),
    "fit_missing": ("quad", (2, 1)),
    "cv_folds_missing": ("quad", (2, 1)),
    "scores_missing": ("quad", (2,)),
    "z_scores_missing": ("exact", (2,)),
}
# KERNEL_TYPE2 works from X^T X, which a host-memory fit accumulates block by block while X is uploaded (upload_accumulate):
# another order of summation than the device-memory fit's, whatever the algo option.  Measured on the commit before HostCall:
# fp64 outputs differ by up to 1.2e-14.  Held to the tolerance of test_gpu_parity.py's fit_host test instead of to the bit.
ACCUMULATING = {"fit_type2"}
CASES = [(e, dt, N, M) for e, (_, Ms) in ENTRIES.items() for dt in ("f64", "f32") for N in NS for M in Ms]


def make_data(N, M, dt):
    """the inputs of every entry for one shape, the same for both kinds of memory"""
    rng = np.random.default_rng(1000 * N + 10 * M + (dt == "f32"))
    npdt = np.float64 if dt == "f64" else np.float32
    F = np.asfortranarray
    lat = rng.standard_normal((N, 3))
    X = lat @ rng.standard_normal((3, K)) + 0.3 * rng.standard_normal((N, K))
    d = dict(X=F(X.astype(npdt)))
    d["Y"] = F((lat @ rng.standard_normal((3, M)) + 0.1 * rng.standard_normal((N, M))).astype(npdt))
    d["Ys"] = F(np.concatenate([d["Y"]] + [rng.standard_normal((N, M)).astype(npdt) for _ in range(NPROB - 1)], axis=1))
    Xm = d["X"].copy(order="F")
    Xm[rng.random((N, K)) < 0.1] = np.nan
    Xm[:, 0] = d["X"][:, 0]  # (a complete column: every row keeps an observed cell)
    d["Xm"] = Xm
    d["R"] = F(rng.standard_normal((K, A)))
    d["P"] = F(rng.standard_normal((K, A)))
    d["W"] = F(rng.standard_normal((K, A)))
    d["Q"] = F(rng.standard_normal((M, A)))
    d["Bm"] = F(rng.standard_normal((K, M)))
    d["Wt"] = F(rng.integers(0, 3, (N, NREP)).astype(np.float64) + 0.5)
    d["idx"] = np.ascontiguousarray(rng.permutation(N)[:FOLDS * TS].reshape(FOLDS, TS).astype(np.int64))
    d["E"] = np.ascontiguousarray(rng.standard_normal((M, A, FOLDS * TS)))
    return d


class Stage:
    """The arguments of one call in host memory (numpy, column-major, ld = rows) or in device memory (torch, ld as given)."""

    def __init__(self, mem_device):
        self.dev = mem_device
        self.outs = []
        self.keep = []

    def inm(self, a, ld=None):
        """input matrix a -> (pointer, ld)"""
        a = np.asfortranarray(a if a.ndim == 2 else a[:, None])
        rows, cols = a.shape
        if not self.dev:
            self.keep.append(a)
            return a.ctypes.data_as(ctypes.c_void_p), max(rows, 1)
        import torch
        ld = ld or rows
        buf = torch.zeros((cols, ld), dtype=torch.from_numpy(a[:1, :1]).dtype, device="cuda")
        buf[:, :rows].copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
        self.keep.append(buf)
        return ctypes.c_void_p(buf.data_ptr()), ld

    def outm(self, rows, cols, npdt=np.float64, ld=None, alias=None):
        """output matrix -> (pointer, ld); alias: the input buffer it overwrites in place (device memory only)"""
        if not self.dev:
            a = np.zeros((rows, cols), dtype=npdt, order="F")
            self.outs.append((a, rows))
            return a.ctypes.data_as(ctypes.c_void_p), max(rows, 1)
        import torch
        ld = ld or rows
        buf = alias if alias is not None else torch.zeros((cols, ld), dtype=torch.from_numpy(np.zeros(1, npdt)).dtype, device="cuda")
        self.outs.append((buf, rows))
        return ctypes.c_void_p(buf.data_ptr()), ld

    def results(self):
        if not self.dev:
            return [a for a, _ in self.outs]
        return [np.asfortranarray(b.cpu().numpy()[:, :rows].T) for b, rows in self.outs]


def run_case(h, entry, dt, N, M, device, want=None):
    """One call of `entry` in host memory or (device = True) in device memory with the staged leading dimension of the entry's
    rule; the list of its outputs as numpy arrays.  want: the names of the optional outputs to ask for (None: all)."""
    from pls_amd import _lib as L
    lib = h._lib
    d = make_data(N, M, dt)
    npdt = np.float64 if dt == "f64" else np.float32
    dtype = L.F64 if dt == "f64" else L.F32
    mem = L.MEM_DEVICE if device else L.MEM_HOST
    ld = LD[ENTRIES[entry][0]](N)
    s = Stage(device)
    ip = d["idx"].ctypes.data_as(ctypes.c_void_p)
    nobs = FOLDS * TS
    opt = lambda name, *a, **k: s.outm(*a, **k)[0] if want is None or name in want else None
    if entry in ("fit", "fit_type2"):
        method = L.KERNEL_TYPE1 if entry == "fit" else L.KERNEL_TYPE2
        (X, ldx), (Y, ldy) = s.inm(d["X"], ld), s.inm(d["Y"], ld)
        W, P, Q, R = s.outm(K, A)[0], s.outm(K, A)[0], s.outm(M, A)[0], s.outm(K, A)[0]
        T, ldt = s.outm(N, A, npdt, ld) if entry == "fit" else (None, N)
        B = s.outm(K, M)[0]
        rc = lib.pls_hip_fit(h.h, X, ldx, Y, ldy, N, K, M, A, method, dtype, mem, W, P, Q, R, T, ldt, B)
    elif entry == "coefficients":
        rc = lib.pls_hip_coefficients(h.h, s.inm(d["R"])[0], s.inm(d["Q"])[0], K, M, A, A, mem, s.outm(K, M)[0])
    elif entry == "xb":
        (X, ldx), (Bm, ldb) = s.inm(d["X"], ld), s.inm(d["Bm"])
        O, ldo = s.outm(N, M, npdt, ld)
        rc = lib.pls_hip_xb(h.h, X, ldx, N, K, Bm, ldb, M, dtype, mem, O, ldo)
    elif entry == "model_sse":
        (X, ldx), (Y, ldy) = s.inm(d["X"], ld), s.inm(d["Y"], ld)
        rc = lib.pls_hip_model_sse(h.h, X, ldx, Y, ldy, N, K, M, A, s.inm(d["R"])[0], s.inm(d["Q"])[0], dtype, mem, s.outm(M, A)[0])
    elif entry == "x_diagnostics":
        X, ldx = s.inm(d["X"], ld)
        R, P = s.inm(d["R"])[0], s.inm(d["P"])[0]
        Qr, T2 = opt("Q", N, A, np.float64, ld), opt("T2", N, A, np.float64, ld)
        S = opt("S", N, A, npdt, ld)
        ssx, sst = opt("ssx", A + 1, 1), opt("sst", A, 1)
        ldo = ld if device else N
        rc = lib.pls_hip_x_diagnostics(h.h, X, ldx, N, N, K, A, R, P, None, dtype, mem, Qr, ldo, T2, ldo, S, ldo, ssx, sst)
    elif entry in ("cv_folds", "cv_folds_sharded"):
        (X, ldx), (Y, ldy) = s.inm(d["X"], ld), s.inm(d["Y"], ld)
        rc = lib.pls_hip_cv_folds(h.h, X, ldx, Y, ldy, N, K, M, A, ip, TS, FOLDS, dtype, mem, s.outm(nobs, M * A)[0])
    elif entry == "fit_batch":
        (X, ldx), (Y, ldy) = s.inm(d["X"], ld), s.inm(d["Ys"], ld)
        R, Q, tt = opt("R", K * A, NPROB), opt("Q", M * A, NPROB), opt("tt", A, NPROB)
        B, ssy = opt("B", K * M, NPROB), opt("ssy", M, NPROB)
        rc = lib.pls_hip_fit_batch(h.h, X, ldx, Y, ldy, N, K, M, A, NPROB, dtype, mem, R, Q, tt, B, ssy)
    elif entry == "fit_resampled":
        (X, ldx), (Y, ldy), (Wt, ldw) = s.inm(d["X"], ld), s.inm(d["Y"], ld), s.inm(d["Wt"])
        Q, tt, B = opt("Q", M * A, NREP), opt("tt", A, NREP), opt("B", K * M, NREP)
        B0, Bmean, Bm2 = opt("B0", K, M), opt("Bmean", K, M), opt("Bm2", K, M)
        rc = lib.pls_hip_fit_resampled(h.h, X, ldx, Y, ldy, N, K, M, A, Wt, ldw, NREP, dtype, mem, Q, tt, B, B0, Bmean, Bm2)
    elif entry == "cv_press_batch":
        (X, ldx), (Y, ldy) = s.inm(d["X"], ld), s.inm(d["Ys"], ld)
        PR, ssy, E = s.outm(M * A, NPROB)[0], s.outm(M, NPROB)[0], s.outm(nobs, NPROB * M * A)[0]
        rc = lib.pls_hip_cv_press_batch(h.h, X, ldx, Y, ldy, N, K, M, A, NPROB, ip, TS, FOLDS, dtype, mem, PR, ssy, E)
    elif entry == "validation":
        E = s.inm(d["E"].reshape(M * A, nobs).T)[0]
        PR, D, pw = opt("PRESS", M, A), opt("D", M, A), opt("probw", M, A)
        ref = opt("ref", M, 1, np.int64)
        rc = lib.pls_hip_validation(h.h, E, nobs, A, M, mem, PR, D, pw, ref)
    elif entry == "fit_missing":
        (X, ldx), (Y, ldy) = s.inm(d["Xm"], ld), s.inm(d["Y"], ld)
        W, P, Q, R = s.outm(K, A)[0], s.outm(K, A)[0], s.outm(M, A)[0], s.outm(K, A)[0]
        T, ldt = s.outm(N, A, npdt, ld)
        B, it = s.outm(K, M)[0], s.outm(A, 1, np.int64)[0]
        rc = lib.pls_hip_fit_missing(h.h, X, ldx, Y, ldy, N, K, M, A, dtype, mem, W, P, Q, R, T, ldt, B, it)
    elif entry == "cv_folds_missing":
        (X, ldx), (Y, ldy) = s.inm(d["Xm"], ld), s.inm(d["Y"], ld)
        E, it = s.outm(nobs, M * A)[0], s.outm(A, FOLDS, np.int64)[0]
        rc = lib.pls_hip_cv_folds_missing(h.h, X, ldx, Y, ldy, N, K, M, A, ip, TS, FOLDS, dtype, mem, E, it)
    elif entry == "scores_missing":
        X, ldx = s.inm(d["Xm"], ld)
        S, lds = s.outm(N, A, npdt, ld)
        rc = lib.pls_hip_scores_missing(h.h, X, ldx, N, K, A, s.inm(d["W"])[0], s.inm(d["P"])[0], dtype, mem, S, lds)
    elif entry == "z_scores_missing":
        X, ldx = s.inm(d["Xm"], ld)
        Z, ldz = s.outm(N, K, npdt, ld, alias=s.keep[-1] if device else None)  # (the host path scales its staged copy in place)
        rc = lib.pls_hip_colwise_z_scores_missing(h.h, X, ldx, N, K, dtype, mem, Z, ldz, s.outm(K, 1)[0], s.outm(K, 1)[0],
                                                  s.outm(K, 1, np.int64)[0])
    else:
        raise KeyError(entry)
    L.check(rc, h.h)
    h.synchronize()
    return s.results()


@pytest.fixture(scope="module")
def handles():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pls_amd
    from pls_amd import _lib as L
    torch.cuda.set_device(0)
    plain, sharded = pls_amd.Handle(), pls_amd.Handle()
    cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
    L.check(L.lib().pls_hip_set_reducer(sharded.h, cb, None, 0, 1), sharded.h)
    yield {"plain": plain, "sharded": sharded}
    plain.close()
    sharded.close()


def _handle_of(handles, entry):
    return handles["sharded" if entry == "cv_folds_sharded" else "plain"]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_host_call_is_the_device_call_of_the_staged_layout(handles, entry, dt, po):
    """bit for bit (ACCUMULATING: to the fit_host tolerance), default ALGO_KERNEL, every N and response count of the entry"""
    h = _handle_of(handles, entry)
    tol = 1e-10 if dt == "f64" else 2e-5
    bad = []
    for e, d, N, M in CASES:
        if e != entry or d != dt:
            continue
        host = run_case(h, entry, dt, N, M, device=False)
        dev = run_case(h, entry, dt, N, M, device=True)
        assert len(host) == len(dev) and len(host) > 0 and any(np.isfinite(a).any() for a in host)
        for i, (a, b) in enumerate(zip(host, dev)):
            assert a.shape == b.shape and a.dtype == b.dtype
            if entry in ACCUMULATING:
                err = po.rel_fro(a, b)
                print(f"{entry} {dt} N={N} M={M} output {i}: rel_fro(host, device) = {err:.3e}")
                assert err < tol
            elif a.tobytes() != b.tobytes():
                with np.errstate(invalid="ignore"):
                    diff = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))
                print(f"{entry} {dt} N={N} M={M} output {i}: max |host - device| = {diff:.3e}")
                bad.append((N, M, i, diff))
    assert not bad, bad


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_gram_host_fit(handles, dt, po):
    """ALGO_GRAM: the host path may accumulate X^T X and X^T Y block by block during the upload, which is another order of
    summation than the device-memory fit's; held to the tolerance of test_gpu_parity.py's fit_host test."""
    import pls_amd
    h = handles["plain"]
    tol = 1e-10 if dt == "f64" else 2e-5
    h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_GRAM)
    try:
        for N in NS:
            host = run_case(h, "fit", dt, N, 2, device=False)
            dev = run_case(h, "fit", dt, N, 2, device=True)
            err = po.rel_fro(host[-1], dev[-1])
            print(f"gram fit {dt} N={N}: rel_fro(B host, B device) = {err:.3e}")
            assert err < tol
    finally:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
