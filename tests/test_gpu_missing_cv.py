"""pls_hip_cv_folds_missing on the device (include/pls_hip.h, "Cross-validation folds of X with missing values"; INTEGRATION.md
section L).  Cases, folds, yardstick and bars come from tests/test_missing_cv_ref.py: the yardstick is the definition (one
fit_missing_ref + scores_missing_ref per fold), the measure the relative Frobenius error per component column of E, the bars
1e-10 in fp64 with M = 1, 2e-5 with fp32 storage, max(1e-10, 10 x the case's sensitivity to the stop) for M > 1.

Run as a program (`python tests/test_gpu_missing_cv.py <case> <file>`) it is the child of the round-cap test: it makes the
six-fold call of the case on a fresh handle -- under whatever PLS_HIP_MISSCV_ROUND the parent set -- and compares the bytes of
E and iters with the bytes in <file>."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_missing_ref import CASES, case_data, rel
from test_missing_cv_ref import CV_CASES, case_folds, column_err, cv_gpu_bar, cv_missing_ref, cv_sensitivity, cv_yardstick

pytestmark = pytest.mark.gpu

BIT_CASES = ("130x70", "1031x130-f32", "257x33-m3")


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
    t.copy_(torch.from_numpy(np.array(a, order="C")).to(dt))
    return t


def _call(handle, name, idx=None, X=None, Y=None):
    """(E, iters) as numpy arrays from the device-memory call of a case (its own data and folds unless given)"""
    N, K, M, A, frac, st = CASES[name]
    Xc, Yc, _ = case_data(name)
    X = Xc if X is None else X
    Y = Yc if Y is None else Y
    idx = case_folds(name) if idx is None else idx
    E, iters = handle.cv_folds_missing(_dev(X, _tdt(st)), _dev(Y, _tdt(st)), A, idx, want_iters=True)
    return np.ascontiguousarray(E.cpu().numpy()), iters.cpu().numpy()


@pytest.fixture(scope="module")
def gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def runs(gpu, handle):
    """the device calls of the cases, each made once and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _call(handle, name)
        return cache[name]
    return get


def _check(E, iters, Eref, iref, bar, M, what):
    assert np.isfinite(E).all(), what
    errs = [rel(E[:, :, a], Eref[:, :, a]) for a in range(Eref.shape[2])]
    print(f"[missing-cv] {what}: bar {bar:.1e}  per component " + " ".join(f"{e:.2e}" for e in errs) +
          f"  iters up to {iters.max()} / {iref.max()}")
    assert max(errs) <= bar, (what, errs, bar)
    assert (np.abs(iters - iref) <= 1).all(), (what, iters, iref)
    if M == 1:
        assert (iters == 1).all()


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CV_CASES)
def test_parity_with_the_yardstick(name, runs):
    E, iters = runs(name)
    Eref, iref = cv_yardstick(name)
    print(f"[missing-cv] {name}: sensitivity {cv_sensitivity(name):.2e}")
    _check(E, iters, Eref, iref, cv_gpu_bar(name), CASES[name][2], name)


# ---- 2. bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BIT_CASES)
def test_same_bits_twice_alone_and_from_host_memory(name, gpu, handle, runs):
    N, K, M, A, frac, st = CASES[name]
    E, iters = runs(name)
    idx = case_folds(name)
    ts = idx.shape[1]
    E2, it2 = _call(handle, name)
    assert E2.tobytes() == E.tobytes() and it2.tobytes() == iters.tobytes(), "two calls with the same arguments differ"
    E3, it3 = _call(handle, name, idx=idx[3:4])
    assert E3.tobytes() == np.ascontiguousarray(E[:, 3 * ts:4 * ts, :]).tobytes(), "fold 3 alone differs from its slice"
    assert it3.tobytes() == iters[3:4].tobytes()
    X, Y, _ = case_data(name)
    ndt = np.float32 if st == "f32" else np.float64
    Eh, ith = handle.cv_folds_missing(np.asfortranarray(X.astype(ndt)), np.asfortranarray(Y.astype(ndt)), A, idx, want_iters=True)
    assert np.ascontiguousarray(Eh).tobytes() == E.tobytes() and ith.tobytes() == iters.tobytes(), "host memory differs from device memory"


def _child(name, path):
    import pls_amd
    import torch
    torch.cuda.set_device(0)
    h = pls_amd.Handle()
    try:
        E, iters = _call(h, name)
    finally:
        h.close()
    want = open(path, "rb").read()
    got = E.tobytes() + iters.tobytes()
    print(f"round cap {os.environ.get('PLS_HIP_MISSCV_ROUND')}: {len(got)} bytes, {'same' if got == want else 'DIFFERENT'}")
    return 0 if got == want else 1


@pytest.mark.parametrize("name", ["130x70", "257x33-m3"])
def test_same_bits_under_a_round_cap(name, runs, tmp_path):
    """six folds in rounds of two (PLS_HIP_MISSCV_ROUND=2, read when the handle is created: a fresh child process) against the
    default, one round"""
    E, iters = runs(name)
    path = tmp_path / "E.bin"
    path.write_bytes(E.tobytes() + iters.tobytes())
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(path)], env=dict(os.environ, PLS_HIP_MISSCV_ROUND="2"),
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "round cap 2:" in r.stdout and "same" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 3. unaligned input ---------------------------------------------------------------------------------------------------------
class Packed:
    """a numpy matrix inside a flat device buffer at an odd element offset with ld = rows: element-aligned, not 16-byte-aligned
    (rows must be odd, so that no column is); every other cell holds a huge finite value"""

    def __init__(self, a, dt):
        torch = _torch()
        rows, cols = a.shape
        assert rows % 2 == 1
        self.ld = rows
        big = 3e38 if dt == torch.float32 else 1e300
        self.flat = torch.full((64 + 1 + rows * cols + 512,), big, dtype=dt, device="cuda")
        self.view = self.flat[65:65 + rows * cols].view(cols, rows).t()
        self.view.copy_(torch.from_numpy(np.array(a, order="C")).to(dt))
        assert self.view.data_ptr() % 16 != 0
        self.snap = self.flat.clone()

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def check(self):
        torch = _torch()
        it = torch.int32 if self.flat.element_size() == 4 else torch.int64
        assert bool((self.flat.view(it) == self.snap.view(it)).all()), "an input (or its surroundings) was modified"


def _raw(handle, name, Xp, ldx, Yp, ldy, idx, gE, gI, N=None, K=None, M=None, A=None):
    from pls_amd import _lib as L
    n, k, m, a, frac, st = CASES[name]
    N, K, M, A = (n if N is None else N), (k if K is None else K), (m if M is None else M), (a if A is None else A)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    rc = L.lib().pls_hip_cv_folds_missing(handle.h, Xp, ldx, Yp, ldy, N, K, M, A, idx.ctypes.data_as(ctypes.c_void_p), idx.shape[1],
                                          idx.shape[0], L.F32 if st == "f32" else L.F64, L.MEM_DEVICE, gE.ptr(0), gI.ptr(0))
    handle.synchronize()
    return rc


def _guards(M, nobs, A, nf, layout="aligned"):
    from test_gpu_bounds import Guarded
    torch = _torch()
    return Guarded([(nobs * A * M, 1)], torch.float64, layout), Guarded([(nf * A, 1)], torch.float64, layout)


def _unpack(gE, gI, M, nobs, A, nf):
    E = gE[0].cpu().numpy()[:, 0].reshape(M, A, nobs).transpose(0, 2, 1)
    return np.ascontiguousarray(E), gI.bits(0).cpu().numpy()[:, 0].reshape(nf, A)


@pytest.mark.parametrize("name", ["67x19", "257x33-m3", "1031x130-f32"])
def test_unaligned_input(name, gpu, handle):
    from pls_amd import _lib as L
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    idx = case_folds(name)
    nf, ts = idx.shape
    Xin, Yin = Packed(X, _tdt(st)), Packed(Y, _tdt(st))
    gE, gI = _guards(M, nf * ts, A, nf, "eigen")
    L.check(_raw(handle, name, Xin.ptr(), Xin.ld, Yin.ptr(), Yin.ld, idx, gE, gI), handle.h)
    gE.check(); gI.check(); Xin.check(); Yin.check()
    E, iters = _unpack(gE, gI, M, nf * ts, A, nf)
    Eref, iref = cv_yardstick(name)
    _check(E, iters, Eref, iref, cv_gpu_bar(name), M, f"{name} ld = N, odd element offset")


# ---- 4. edge cases --------------------------------------------------------------------------------------------------------------
def test_held_out_row_without_an_observed_cell(gpu, handle):
    name = "67x19"
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    idx = case_folds(name)
    Xe = np.array(X, order="F")
    Xe[idx[0, 0], :] = np.nan
    E, iters = _call(handle, name, X=Xe)
    Eref, iref = cv_missing_ref(Xe, Y, A, idx)
    _check(E, iters, Eref, iref, cv_gpu_bar(name), M, f"{name}, a held-out row all NaN")
    assert np.array_equal(E[:, 0, :], np.repeat(Y[idx[0, 0]][:, None], A, axis=1))  # t = 0: the residual is y itself


def test_column_observed_in_the_held_out_rows_only(gpu, handle):
    name = "67x19"
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    idx = case_folds(name)
    k = 7
    Xe = np.array(X, order="F")
    keep = np.where(np.isnan(Xe[idx[0], k]), 0.25, Xe[idx[0], k])
    Xe[:, k] = np.nan
    Xe[idx[0], k] = keep   # fold 0: no observed training cell in column k, its held-out rows all observed there
    E, iters = _call(handle, name, X=Xe)
    Eref, iref = cv_missing_ref(Xe, Y, A, idx)
    _check(E, iters, Eref, iref, cv_gpu_bar(name), M, f"{name}, a column observed in fold 0's held-out rows only")


# ---- 5. bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["67x19", "40x300-m2", "33x20011", "5x12"])
def test_writes_stay_inside_E_and_iters(name, gpu, handle, runs):
    from pls_amd import _lib as L
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    idx = case_folds(name)
    nf, ts = idx.shape
    Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
    gE, gI = _guards(M, nf * ts, A, nf)
    L.check(_raw(handle, name, Xd.data_ptr(), int(Xd.stride(1)), Yd.data_ptr(), int(Yd.stride(1)), idx, gE, gI), handle.h)
    gE.check(); gI.check()   # every guard cell bit for bit, no prefill left
    E, iters = _unpack(gE, gI, M, nf * ts, A, nf)
    Eb, ib = runs(name)
    assert E.tobytes() == Eb.tobytes() and iters.tobytes() == ib.tobytes()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_E_and_iters_untouched(gpu):
    import pls_amd
    from pls_amd import _lib as L
    name = "67x19"
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    good = case_folds(name)
    nf, ts = good.shape
    h = pls_amd.Handle()
    try:
        Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
        Y33 = h.synth_y(0, N, 33, 3)
        ldx, ldy = int(Xd.stride(1)), int(Yd.stride(1))

        def call(idx, Yt=Yd, M_=M, **kw):
            gE, gI = _guards(M_, idx.shape[0] * idx.shape[1], A, idx.shape[0])
            rc = _raw(h, name, Xd.data_ptr(), ldx, Yt.data_ptr(), int(Yt.stride(1)), idx, gE, gI, M=M_, **kw)
            for g in (gE, gI):
                g.assert_untouched()
                g.assert_prefilled(0)
            return rc
        bad = good.copy(); bad[4, 2] = N
        assert call(bad) == L.ERR_INVALID
        bad = good.copy(); bad[0, 0] = -1
        assert call(bad) == L.ERR_INVALID
        bad = good.copy(); bad[2, 5] = bad[2, 1]
        assert call(bad) == L.ERR_INVALID
        assert call(np.arange(N, dtype=np.int64)[None, :]) == L.ERR_INVALID          # test_size = N
        assert call(np.arange(N + 1, dtype=np.int64)[None, :] % N) == L.ERR_INVALID  # test_size > N
        assert call(good, Yt=Y33, M_=33) == L.ERR_UNSUPPORTED
        assert call(good, A=K + 1) == L.ERR_INVALID
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        try:
            assert call(good) == L.ERR_UNSUPPORTED
        finally:
            h.clear_reducer()
        # a row held out by two DIFFERENT folds is fine, and the handle is healthy
        twice = np.concatenate([good, good[:1]])
        E, iters = _call(h, name, idx=twice)
        Eref, _ = cv_yardstick(name)
        assert column_err(E[:, :nf * ts, :], Eref) <= cv_gpu_bar(name)
        assert E[:, nf * ts:, :].tobytes() == E[:, :ts, :].tobytes()
    finally:
        h.close()


# ---- 7. the Model ---------------------------------------------------------------------------------------------------------------
def test_model_cross_validates_with_missing_cells(gpu, handle):
    import pls_amd
    from pls_amd.model import pick_components
    name = "67x19"
    N, K, M, A, frac, st = CASES[name]
    X, Y, _ = case_data(name)
    Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
    m = pls_amd.Model(Xd, Yd, max_components=A, handle=handle, missing=True)
    E = m.cv_LOO()
    Eref, _ = cv_missing_ref(X, Y, A, np.arange(N, dtype=np.int64)[:, None])
    assert tuple(E.shape) == (M, N, A)
    e = column_err(E.cpu().numpy(), Eref)
    print(f"[missing-cv] {name}: Model.cv_LOO vs the yardstick {e:.2e}")
    assert e <= cv_gpu_bar(name)
    _, _, probw, ref = handle.validation(np.ascontiguousarray(Eref))
    want = pick_components(probw, ref, 0.1)
    got = m.optimal_num_components(E)
    print(f"[missing-cv] {name}: optimal number of components {got} / from the yardstick {want}")
    assert np.array_equal(np.asarray(got), np.asarray(want))
    assert np.isfinite(m.validation(E, pls_amd.MSE).cpu().numpy()).all()
    # leave-some-out: the same splits from the same generator
    E = m.cv_LSO(0.1, 4, rng=np.random.default_rng(3))
    rng = np.random.default_rng(3)
    idx = np.stack([rng.permutation(N)[:int(0.1 * N + 0.5)] for _ in range(4)])
    assert column_err(E.cpu().numpy(), cv_missing_ref(X, Y, A, idx)[0]) <= cv_gpu_bar(name)
    # new data with missing cells: the last column is Y - fitted_values_missing
    E = m.cv_NEW_DATA(Xd, Yd).cpu().numpy()
    F = m.fitted_values_missing(Xd).cpu().numpy()
    assert rel(E[:, :, A - 1], (Y - F).T) <= 1e-12
    # a model fitted without the switch cross-validates as before: the NaN reaches E
    m2 = pls_amd.Model(Xd, Yd, max_components=A, handle=handle)
    assert np.isnan(m2.cv_LSO(0.1, 2, rng=np.random.default_rng(3)).cpu().numpy()).any()
    # numpy inputs: host memory
    mh = pls_amd.Model(X, Y, max_components=A, handle=handle, missing=True)
    assert column_err(mh.cv_LOO(), Eref) <= cv_gpu_bar(name)


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1], sys.argv[2]))
