"""pls_hip_fit_missing, pls_hip_scores_missing, pls_hip_colwise_z_scores_missing on the device (include/pls_hip.h, "X with
missing values").  Cases, yardstick and bars come from tests/test_missing_ref.py: the numpy restatement
of the algorithm, the project's accuracy bars (1e-10 in fp64, 2e-5 with fp32 storage), and for M > 1 the bar widened to
max(1e-10, 10 x the case's measured sensitivity to where the iteration stops)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_bounds import Guarded
from test_missing_ref import (CASES, MULTI, TOL_F32, TOL_F64, case_data, case_sensitivity, case_yardstick, empty_row_column_checks,
                              fit_missing_ref, gpu_bar, measure, rel, scores_missing_ref, z_scores_missing_ref)

pytestmark = pytest.mark.gpu

NAMES = ("W", "P", "Q", "R", "T", "B", "iters")
BIG = 1e300  # what the guard cells and padding rows of a placed INPUT hold: finite, so a read past row N shows in the result


def _torch():
    import torch
    return torch


def _tdt(st):
    torch = _torch()
    return torch.float32 if st == "f32" else torch.float64


def _dev(a, dt):
    """column-major device copy of a numpy matrix (16-byte columns)"""
    import pls_amd
    torch = _torch()
    t = pls_amd.colmajor_empty(a.shape[0], a.shape[1], dt, "cuda")
    t.copy_(torch.from_numpy(np.array(a, order="C")).to(dt))   # (a copy: the cases' arrays are read-only)
    return t


def _np(out):
    return {k: (v.detach().cpu().numpy() if v is not None and not isinstance(v, np.ndarray) else v) for k, v in out.items()}


def _bits(out):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in _np(out).items()}


@pytest.fixture(scope="module")
def gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def fits(gpu, handle):
    """device fits of the cases, each computed once and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            N, K, M, A, frac, st = CASES[name]
            X, Y, _ = case_data(name)
            cache[name] = _np(handle.fit_missing(_dev(X, _tdt(st)), _dev(Y, _tdt(st)), A))
        return cache[name]
    return get


def _check(got, ref, bar, align, what):
    w = measure(got, ref, align)
    print(f"[missing] {what}: bar {bar:.1e}  " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= bar, (what, k, v, bar)
    return w


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_yardstick(name, fits):
    N, K, M, A, frac, st = CASES[name]
    got, y = fits(name), case_yardstick(name)
    for k in ("W", "P", "Q", "R", "T", "B"):
        assert np.isfinite(got[k]).all(), k
    print(f"[missing] {name}: iters {got['iters']} / yardstick {y['iters']}  sensitivity {case_sensitivity(name):.2e}")
    _check(got, y, gpu_bar(name), M > 1, name)
    assert (np.abs(got["iters"] - y["iters"]) <= 1).all(), (got["iters"], y["iters"])
    if M == 1:
        assert (got["iters"] == 1).all()


# ---- 2. no NaN in X: the NIPALS plan of pls_hip_fit -----------------------------------------------------------------------------
def _separated(name):
    """(X complete, Y with M = 2) for the comparison with pls_hip_fit at 1e-10.  pls_hip_fit takes the direction of a component
    from an eigenvector, pls_hip_fit_missing stops its iteration where |t - t_prev| <= 1e-10 |t|; the iteration is a power
    iteration on Y_a^T X_a X_a^T Y_a, so at an eigenvalue ratio rho it stops within rho / (1 - rho) x 1e-10 of the fixed point.
    The cases' own Y (random mixtures of latent columns of similar scale) has rho up to 0.9 (tests/test_missing_ref.py prints
    the sensitivity); here the two responses follow two latent columns at scales 1 and 0.1, which puts rho near 1e-2 for both
    components and the stop within 1e-12 of the fixed point."""
    N, K, M, A, frac, st = CASES[name]
    _, _, Xc = case_data(name)
    rng = np.random.default_rng([2] + [int(b) for b in name.encode()])
    U = np.linalg.svd(Xc, full_matrices=False)[0]
    Y = np.stack([U[:, 0] + 0.02 * rng.standard_normal(N), 0.1 * U[:, 1] + 0.002 * rng.standard_normal(N)], axis=1)
    return Xc, np.asfortranarray(Y - Y.mean(axis=0))


@pytest.mark.parametrize("name", ["67x19", "130x70", "5000x40", "257x33-m3:separated", "40x300-m2:separated"])
def test_complete_data_equals_the_nipals_plan(name, gpu, handle):
    import pls_amd
    name, _, kind = name.partition(":")
    N, K, M, A, frac, st = CASES[name]
    _, Y, Xc = case_data(name)
    if kind:
        Xc, Y = _separated(name)
        M, A = 2, 2
        s = measure(fit_missing_ref(Xc, Y, A), fit_missing_ref(Xc, Y, A, tol=1e-14, max_iters=2000), True)
        print(f"[missing] {name} separated responses: sensitivity to the stop " + "  ".join(f"{k} {v:.2e}" for k, v in s.items()))
    Xd, Yd = _dev(Xc, _tdt(st)), _dev(Y, _tdt(st))
    got = _np(handle.fit_missing(Xd, Yd, A))
    h = pls_amd.Handle()
    try:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        ref = _np(h.fit_device(Xd, Yd, A))
        h.synchronize()
    finally:
        h.close()
    _check(got, ref, TOL_F64, M > 1, f"{name} complete data vs ALGO_NIPALS")
    assert M > 1 or (got["iters"] == 1).all()


# ---- 3. bounds and inputs -------------------------------------------------------------------------------------------------------
class PlacedInput:
    """a numpy matrix inside a flat device buffer whose every other cell -- guard cells before and after, the padding rows of
    each column (ld > rows) -- holds 1e300: "aligned" 16-byte columns, "eigen" an odd element offset and ld = rows + 1"""

    def __init__(self, a, dt, layout):
        torch = _torch()
        rows, cols = a.shape
        es = torch.empty((), dtype=dt).element_size()
        V = 16 // es
        self.ld = rows + 1 if layout == "eigen" else -(-rows // V) * V + V
        off = 64 + (1 if layout == "eigen" else 0)
        self.flat = torch.full((off + self.ld * cols + 4 * self.ld + 512,), BIG if es == 8 else 3e38, dtype=dt, device="cuda")
        self.view = self.flat[off:off + self.ld * cols].view(cols, self.ld)[:, :rows].t()
        self.view.copy_(torch.from_numpy(np.array(a, order="C")).to(dt))
        self.snap = self.flat.view(torch.int64 if es == 8 else torch.int32).clone()
        self.idt = self.snap.dtype

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def check(self):
        assert bool((self.flat.view(self.idt) == self.snap).all()), "an input (or its surroundings) was modified"


def _raw_fit(handle, Xin, Yin, N, K, M, A, st, layout):
    """pls_hip_fit_missing with every output between guard cells; returns (dict of numpy outputs, the Guarded buffers)"""
    from pls_amd import _lib as L
    torch = _torch()
    g64 = Guarded([(K, A, K), (K, A, K), (M, A, M), (K, A, K), (K, M, K), (A, 1, A)], torch.float64, layout)
    gT = Guarded([(N, A)], _tdt(st), layout)
    rc = L.lib().pls_hip_fit_missing(handle.h, Xin.ptr(), Xin.ld, Yin.ptr(), Yin.ld, N, K, M, A, L.F32 if st == "f32" else L.F64,
                                     L.MEM_DEVICE, g64.ptr(0), g64.ptr(1), g64.ptr(2), g64.ptr(3), gT.ptr(0), gT.ld(0), g64.ptr(4),
                                     g64.ptr(5))
    L.check(rc, handle.h)
    handle.synchronize()
    out = dict(W=g64[0], P=g64[1], Q=g64[2], R=g64[3], B=g64[4], T=gT[0])
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out["iters"] = g64.bits(5).cpu().numpy()[:, 0].copy()
    return out, (g64, gT)


@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("name", ["67x19", "40x300-m2", "1031x130-f32", "513x24"])
def test_bounds_and_inputs(name, layout, gpu, handle):
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    Xin, Yin = PlacedInput(X, _tdt(st), layout), PlacedInput(Y, _tdt(st), layout)
    got, guards = _raw_fit(handle, Xin, Yin, N, K, M, A, st, layout)
    for g in guards:
        g.check()   # every guard cell bit for bit, no prefill left
    Xin.check(); Yin.check()
    y = case_yardstick(name)
    _check(got, y, gpu_bar(name), M > 1, f"{name} {layout}")
    assert (np.abs(got["iters"] - y["iters"]) <= 1).all()


# ---- 4. bits --------------------------------------------------------------------------------------------------------------------
BIT_CASES = ("130x70", "1031x130-f32", "257x33-m3")


def test_same_bits_whatever_the_handle_ran_before(gpu):
    """host against device memory, two calls in a row, after pls_hip_test_poison_workspace, after an unrelated pls_hip_fit
    and pls_hip_fit_batch: tools/missing_probe.py in a child process on the testing build, as tests/test_gpu_history.py"""
    env = dict(os.environ, PLS_AMD_LIBRARY=os.path.join(ROOT, "pls_amd", "csrc", "testing", "libpls_hip.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "missing_probe.py"), *BIT_CASES], env=env, capture_output=True,
                       text=True, timeout=120)
    print(r.stdout)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode in (0, 1), f"the probe ended abnormally ({r.returncode}):\n{tail}"
    m = re.search(r"^done: (\d+) cases, (\d+) differ$", r.stdout, re.M)
    assert m, f"the probe did not finish:\n{tail}"
    assert int(m.group(1)) == len(BIT_CASES)
    assert len(re.findall(r"^(?:same|DIFFERS): ", r.stdout, re.M)) == 6 * len(BIT_CASES)
    assert len(re.findall(r"^same: .*: poison 0x", r.stdout, re.M)) == 2 * len(BIT_CASES), tail
    assert int(m.group(2)) == 0 and r.returncode == 0, "\n".join(re.findall(r"^DIFFERS.*$", r.stdout, re.M))


# ---- 5. NaN payloads ------------------------------------------------------------------------------------------------------------
PAYLOADS = {8: (0xFFF8000000000000, 0x7FF800000BADC0DE, 0x7FF0000000000001, 0xFFF4000000000123),
            4: (0xFFC00000, 0x7FC0BEEF, 0x7F800001, 0xFFA00123)}


@pytest.mark.parametrize("name", ["130x70", "1031x130-f32", "257x33-m3"])
def test_nan_payloads_do_not_matter(name, gpu, handle, fits):
    torch = _torch()
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    dt = _tdt(st)
    es = 4 if st == "f32" else 8
    base = _bits(fits(name))
    Yd = _dev(Y, dt)
    for pat in PAYLOADS[es]:
        Xd = _dev(X, dt)
        nan = torch.isnan(Xd)
        iv = Xd.view(torch.int32 if es == 4 else torch.int64)
        signed = pat - (1 << (8 * es)) if pat >> (8 * es - 1) else pat
        iv[nan] = signed
        assert bool((torch.isnan(Xd) == nan).all())
        got = _bits(handle.fit_missing(Xd, Yd, A))
        for k in NAMES:
            assert got[k] == base[k], (name, hex(pat), k)


# ---- 6. empty row and column ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["67x19", "257x33-m3"])
def test_empty_row_and_column_on_the_device(name, gpu, handle):
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    fit = lambda Xe, Ye, Ae: _np(handle.fit_missing(_dev(Xe, _tdt(st)), _dev(Ye, _tdt(st)), Ae))
    empty_row_column_checks(fit, X, Y, A, 5, 7)


# ---- 7. PLS_HIP_OPT_MISSING_ITERS -----------------------------------------------------------------------------------------------
def test_missing_iters_option(gpu):
    import pls_amd
    from pls_amd import _lib as L
    name = "257x33-m3"
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
    h = pls_amd.Handle()
    try:
        assert h.get_option(pls_amd.OPT_MISSING_ITERS) == 500
        base = _bits(h.fit_missing(Xd, Yd, A))
        for bad in (0, (1 << 20) + 1, -1):
            with pytest.raises(pls_amd.PlsHipError) as e:
                h.set_option(pls_amd.OPT_MISSING_ITERS, bad)
            assert e.value.code == L.ERR_INVALID
        assert h.get_option(pls_amd.OPT_MISSING_ITERS) == 500
        h.set_option(pls_amd.OPT_MISSING_ITERS, 1 << 20)
        h.set_option(pls_amd.OPT_MISSING_ITERS, 1)
        assert h.get_option(pls_amd.OPT_MISSING_ITERS) == 1
        got = _np(h.fit_missing(Xd, Yd, A))
        assert (got["iters"] == 1).all()
        _check(got, fit_missing_ref(X, Y, A, max_iters=1), TOL_F64, True, f"{name} max_iters = 1")
        h.set_option(pls_amd.OPT_MISSING_ITERS, 500)
        again = _bits(h.fit_missing(Xd, Yd, A))
        for k in NAMES:
            assert again[k] == base[k], k
    finally:
        h.close()


# ---- 8. scores_missing ----------------------------------------------------------------------------------------------------------
def _heldout(name, frac=0.2):
    """rows the model has not seen, from the case's own generator continued, with `frac` of their cells missing"""
    N, K, M, A, _, st = CASES[name]
    _, _, Xc = case_data(name)
    rng = np.random.default_rng([7] + [int(b) for b in name.encode()])
    n = 37
    mix = rng.standard_normal((n, min(N, 12)))
    Xn = mix @ Xc[:min(N, 12)] / np.sqrt(min(N, 12)) + 0.05 * rng.standard_normal((n, K))
    if st == "f32":
        Xn = Xn.astype(np.float32).astype(np.float64)
    Xm = Xn.copy()
    Xm[rng.random((n, K)) < frac] = np.nan
    return np.asfortranarray(Xn), np.asfortranarray(Xm)


@pytest.mark.parametrize("name", ["130x70", "257x33-m3", "1031x130-f32", "33x20011"])
def test_scores_missing(name, gpu, handle, fits):
    torch = _torch()
    N, K, M, A, frac, st = CASES[name]
    X, Y, Xc = case_data(name)
    dt = _tdt(st)
    bar = TOL_F32 if st == "f32" else TOL_F64
    m = fits(name)
    W, P, R = (torch.from_numpy(m[k]).cuda() for k in "WPR")
    # the training X reproduces T
    S = handle.scores_missing(_dev(X, dt), W, P).cpu().numpy()
    e = rel(S, m["T"])
    print(f"[missing] {name}: scores of the training X vs T {e:.2e}")
    assert e <= bar
    # complete rows: X R
    Xn, Xm = _heldout(name)
    Xnd = _dev(Xn, dt)
    S = handle.scores_missing(Xnd, W, P).cpu().numpy()
    XR = handle.xb(Xnd, R).cpu().numpy()
    e = rel(S, XR)
    print(f"[missing] {name}: scores of complete rows vs xb(X, R) {e:.2e}")
    assert e <= (TOL_F32 if st == "f32" else 1e-12)
    # held-out rows with 20 % of their cells missing
    S = handle.scores_missing(_dev(Xm, dt), W, P).cpu().numpy()
    ref = scores_missing_ref(Xm, m["W"], m["P"])
    e = max(rel(S[:, a], ref[:, a]) for a in range(A))
    print(f"[missing] {name}: scores of held-out rows with missing cells vs the yardstick {e:.2e}")
    assert e <= bar


def test_scores_missing_eigen_layout_and_host(gpu, handle, fits):
    from pls_amd import _lib as L
    torch = _torch()
    name = "130x70"
    N, K, M, A, frac, st = CASES[name]
    m = fits(name)
    _, Xm = _heldout(name)
    n = Xm.shape[0]
    ref = scores_missing_ref(Xm, m["W"], m["P"])
    Xin = PlacedInput(Xm, torch.float64, "eigen")
    g = Guarded([(n, A)], torch.float64, "eigen")
    gm = Guarded([(K, A, K), (K, A, K)], torch.float64, "eigen")
    gm[0].copy_(torch.from_numpy(m["W"])); gm[1].copy_(torch.from_numpy(m["P"]))
    rc = L.lib().pls_hip_scores_missing(handle.h, Xin.ptr(), Xin.ld, n, K, A, gm.ptr(0), gm.ptr(1), L.F64, L.MEM_DEVICE, g.ptr(0), g.ld(0))
    L.check(rc, handle.h)
    handle.synchronize()
    g.check(); gm.assert_untouched(); Xin.check()
    S = g[0].cpu().numpy()
    assert max(rel(S[:, a], ref[:, a]) for a in range(A)) <= TOL_F64
    Sh = handle.scores_missing(Xm, m["W"], m["P"])   # numpy: host memory
    assert max(rel(Sh[:, a], ref[:, a]) for a in range(A)) <= TOL_F64


# ---- 9. z_scores_missing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["67x19", "1031x130-f32", "5000x40"])
def test_z_scores_missing(name, gpu, handle):
    N, K, M, A, frac, st = CASES[name]
    X, _, Xc = case_data(name)
    dt = _tdt(st)
    shift = np.linspace(-2.0, 3.0, K)
    Xs = np.array(X + shift, order="F")
    if st == "f32":
        Xs = Xs.astype(np.float32).astype(np.float64)
    Xs[:, 2] = np.nan; Xs[4, 2] = 1.5    # one observed cell
    Xs[:, 3] = 2.0                       # constant
    Zr, mr, sr, nr = z_scores_missing_ref(Xs)
    Xd = _dev(Xs, dt)
    Z, mean, sd, nobs = (v.cpu().numpy() for v in handle.z_scores_missing(Xd))
    assert np.array_equal(nobs, nr)
    ok = np.ones(K, dtype=bool); ok[[2, 3]] = False
    assert np.isnan(Z[:, 2]).all() and np.isnan(Z[:, 3]).all() and np.isnan(sd[2]) and sd[3] == 0 and mean[2] == 1.5 and mean[3] == 2.0
    assert np.array_equal(np.isnan(Z), np.isnan(Zr))
    bar = 1e-12 if st == "f64" else 1e-6   # (fp32: Z is rounded to the storage type, 6e-8 per cell)
    e = dict(mean=rel(mean[ok], mr[ok]), sd=rel(sd[ok], sr[ok]), Z=rel(np.nan_to_num(Z[:, ok]), np.nan_to_num(Zr[:, ok])))
    print(f"[missing] {name}: z-scores vs numpy " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["mean"] <= 1e-12 and e["sd"] <= 1e-12 and e["Z"] <= bar
    # in place: the same bits
    Z2, mean2, sd2, nobs2 = handle.z_scores_missing(Xd, inplace=True)
    assert Z2.data_ptr() == Xd.data_ptr()
    for a, b in ((Z, Z2), (mean, mean2), (sd, sd2), (nobs, nobs2)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b.cpu().numpy()).tobytes()
    # the fit drops the two columns
    _, Y, _ = case_data(name)
    fit = _np(handle.fit_missing(Xd, _dev(Y, dt), 2))
    for k in ("W", "P", "R", "B"):
        assert not fit[k][[2, 3], :].any() and np.isfinite(fit[k]).all(), k
    # complete data: pls_hip_colwise_z_scores
    Xcd = _dev(np.asfortranarray(Xc + shift), dt)
    Zc, mc, sc = (v.cpu().numpy() for v in handle.colwise_z_scores(Xcd))
    Zm, mm, sm, nm = (v.cpu().numpy() for v in handle.z_scores_missing(Xcd))
    assert (nm == N).all()
    e = dict(mean=rel(mm, mc), sd=rel(sm, sc), Z=rel(Zm, Zc))
    print(f"[missing] {name}: complete data vs colwise_z_scores " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["mean"] <= 1e-14 and e["sd"] <= 1e-14 and e["Z"] <= (1e-14 if st == "f64" else 1e-6)


def test_z_scores_missing_host(gpu, handle):
    X, _, _ = case_data("67x19")
    Xs = np.array(X + 1.0, order="F")
    Zr, mr, sr, nr = z_scores_missing_ref(Xs)
    Z, mean, sd, nobs = handle.z_scores_missing(Xs)
    assert np.array_equal(nobs, nr) and rel(mean, mr) <= 1e-12 and rel(sd, sr) <= 1e-12
    assert np.array_equal(np.isnan(Z), np.isnan(Zr)) and rel(np.nan_to_num(Z), np.nan_to_num(Zr)) <= 1e-12


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(gpu):
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    N, K, A = 50, 20, 3
    h = pls_amd.Handle()
    try:
        X = h.synth_x(0, N, K, 3)
        Y33, Y = h.synth_y(0, N, 33, 3), h.synth_y(0, N, 2, 3)
        ld = int(X.stride(1))

        def call(Xp, ldx, Yt, K_, M, A_):
            g = Guarded([(K, A, K), (K, A, K), (M, A, M), (K, A, K), (K, M, K), (A, 1, A), (N, A)], torch.float64, "aligned")
            rc = L.lib().pls_hip_fit_missing(h.h, Xp, ldx, Yt.data_ptr(), int(Yt.stride(1)), N, K_, M, A_, L.F64, L.MEM_DEVICE, g.ptr(0),
                                             g.ptr(1), g.ptr(2), g.ptr(3), g.ptr(6), g.ld(6), g.ptr(4), g.ptr(5))
            h.synchronize()
            g.assert_untouched()
            for i in range(len(g)):
                g.assert_prefilled(i)
            return rc
        assert call(X.data_ptr(), ld, Y33, K, 33, A) == L.ERR_UNSUPPORTED
        assert call(X.data_ptr(), ld, Y, K, 2, K + 1) == L.ERR_INVALID
        assert call(X.data_ptr(), N - 1, Y, K, 2, A) == L.ERR_INVALID
        assert call(None, ld, Y, K, 2, A) == L.ERR_INVALID
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        try:
            assert call(X.data_ptr(), ld, Y, K, 2, A) == L.ERR_UNSUPPORTED
            with pytest.raises(pls_amd.PlsHipError) as e:
                h.scores_missing(X, torch.zeros(K, A, dtype=torch.float64, device="cuda"), torch.zeros(K, A, dtype=torch.float64, device="cuda"))
            assert e.value.code == L.ERR_UNSUPPORTED
            with pytest.raises(pls_amd.PlsHipError) as e:
                h.z_scores_missing(X)
            assert e.value.code == L.ERR_UNSUPPORTED
        finally:
            h.clear_reducer()
        out = h.fit_missing(X, Y, A)   # the handle is healthy
        h.synchronize()
        assert np.isfinite(out["B"].cpu().numpy()).all()
    finally:
        h.close()


# ---- 11. the Python surface -----------------------------------------------------------------------------------------------------
def test_model_surface(gpu, handle):
    import pls_amd
    name = "130x70"
    N, K, M, A, frac, st = CASES[name]
    X, Y, Xc = case_data(name)
    y = case_yardstick(name)
    Xd, Yd, Xcd = _dev(X, _tdt(st)), _dev(Y, _tdt(st)), _dev(Xc, _tdt(st))
    m = pls_amd.Model(Xd, Yd, max_components=A, handle=handle, missing=True)
    assert rel(m.coefficients().cpu().numpy(), y["B"]) <= TOL_F64
    assert rel(m.coefficients(2).cpu().numpy(), y["R"][:, :2] @ y["Q"][:, :2].T) <= TOL_F64
    assert rel(m.scores(Xcd).cpu().numpy(), Xc @ y["R"]) <= TOL_F64
    assert rel(m.fitted_values(Xcd).cpu().numpy(), Xc @ y["B"]) <= TOL_F64
    assert rel(m.loadingsX(3).cpu().numpy(), y["P"][:, :3]) <= TOL_F64 and rel(m.loadingsY().cpu().numpy(), y["Q"]) <= TOL_F64
    assert rel(m.scores_missing(Xd).cpu().numpy(), y["T"]) <= TOL_F64
    assert rel(m.fitted_values_missing(Xd).cpu().numpy(), y["T"] @ y["Q"].T) <= TOL_F64
    assert rel(m.fitted_values_missing(Xd, 2).cpu().numpy(), y["T"][:, :2] @ y["Q"][:, :2].T) <= TOL_F64
    m2 = pls_amd.Model(Xd, Yd, max_components=A, handle=handle)   # without the switch a NaN reaches every output
    assert np.isnan(m2.coefficients().cpu().numpy()).any()
    m2.plsr_missing(Xd, Yd)
    assert rel(m2.coefficients().cpu().numpy(), y["B"]) <= TOL_F64
    # numpy inputs: host memory
    mh = pls_amd.Model(X, Y, max_components=A, handle=handle, missing=True)
    assert rel(mh.coefficients(), y["B"]) <= TOL_F64 and rel(mh.T, y["T"]) <= TOL_F64
    assert rel(mh.fitted_values_missing(X), y["T"] @ y["Q"].T) <= TOL_F64
