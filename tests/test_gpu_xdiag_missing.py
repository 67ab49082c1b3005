"""pls_hip_x_diagnostics_missing on the device (include/pls_hip.h): scores, Q residuals, T^2, ssx, sst and
the observed cells per row of X with NaN cells.  Cases, yardstick and bars come from tests/test_xdiag_missing_ref.py: the numpy
restatement of the definition and the project's accuracy bars -- TOL_F64 = 1e-10 relative Frobenius per output for everything
fp64 (for Q also on the worst row), TOL_F32 = 2e-5 for S in fp32 storage.

Run as a program (`python tests/test_gpu_xdiag_missing.py NAME ...`) it is the child process of the streaming cross-check: the
parent sets PLS_HIP_XDIAGMISS_ROUTE=stream, the child prints the errors of every named case against the yardstick, one line each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # the child process: the tests' directory and the repository root, as conftest.py gives the suite
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

from test_missing_ref import CASES as FIT_CASES
from test_missing_ref import TOL_F32, TOL_F64, case_data, rel
from test_xdiag_missing_ref import CASES, RESIDENT, case_ref, worst_row, xd_case, xdiag_missing_ref

pytestmark = pytest.mark.gpu

OUT = ("Q", "T2", "S", "ssx", "sst", "nobs")
RESIDENT_CASES = [n for n, c in CASES.items() if c[5] == RESIDENT]


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


def _np(out):
    return {k: (v.detach().cpu().numpy() if not isinstance(v, np.ndarray) else v) for k, v in out.items()}


def _bits(out):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in _np(out).items()}


def run(handle, X, m, st, tvar=None, want=OUT):
    """the device-memory call on the 16-byte aligned layout; numpy outputs"""
    torch = _torch()
    W, P = torch.from_numpy(np.array(m["W"])).cuda(), torch.from_numpy(np.array(m["P"])).cuda()
    out = handle.x_diagnostics_missing(X if not isinstance(X, np.ndarray) else _dev(X, _tdt(st)), W, P, tvar=tvar, want=want)
    handle.synchronize()
    return _np(out)


def errors(got, ref, st):
    """error per output that `got` holds against the yardstick `ref` (nobs: the largest difference), and of the worst row of Q"""
    e = {}
    for k in got:
        if k == "nobs":
            e[k] = float(np.abs(got[k] - ref[k]).max())
        else:
            e[k] = rel(got[k], ref[k])
    if "Q" in got:
        e["Qrow"] = worst_row(got["Q"], ref["Q"])
    return e


def bar_of(k, st):
    return 0.0 if k == "nobs" else (TOL_F32 if (k == "S" and st == "f32") else TOL_F64)


def check(got, ref, st, what):
    e = errors(got, ref, st)
    print(f"[xdiag-missing] {what}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= bar_of(k, st), (what, k, v, bar_of(k, st))
    for k in got:
        if k != "nobs":
            assert np.isfinite(got[k]).all(), (what, k)
    return e


def xb_launches(handle, fn):
    """fn() and the number of launches it made in the family of the sweeps over X"""
    import pls_amd
    handle.set_option(pls_amd.OPT_PROFILE, 1)
    handle.timing()
    out = fn()
    handle.synchronize()
    n = handle.timing()["launches"]["xb"]
    handle.set_option(pls_amd.OPT_PROFILE, 0)
    return out, n


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a device left in error by an earlier case ends the session here, before anything more is launched on it"""
    torch = _torch()
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:   # (the sticky error of a fault)
            pytest.exit(f"the device is in error, nothing more is run on it: {e}", returncode=3)
    yield


@pytest.fixture(scope="module")
def gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def results(gpu, handle):
    """every output of a case on the default route, computed once and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            X, _, m = xd_case(name)
            cache[name] = run(handle, X, m, CASES[name][4])
        return cache[name]
    return get


# ---- 1. parity with the yardstick -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_yardstick(name, gpu, handle):
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    got, n = xb_launches(handle, lambda: run(handle, X, m, st))
    check(got, case_ref(name), st, f"{name} ({route})")
    assert got["nobs"].dtype == np.int64 and got["S"].dtype == (np.float32 if st == "f32" else np.float64)
    # the route the case claims: one read of X against A + 1 sweeps
    assert n == (1 if route == RESIDENT else A + 1), (name, route, n)


def test_resident_cases_on_the_streaming_route(gpu):
    """every case whose default route is the resident one, again in a fresh child process under PLS_HIP_XDIAGMISS_ROUTE=stream"""
    env = dict(os.environ, PLS_HIP_XDIAGMISS_ROUTE="stream")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *RESIDENT_CASES], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [l["name"] for l in lines] == RESIDENT_CASES
    for l in lines:
        st, A = CASES[l["name"]][4], CASES[l["name"]][2]
        assert l["xb"] == A + 1, l     # it did stream
        for k, v in l["err"].items():
            assert v <= bar_of(k, st), (l["name"], k, v)


# ---- 2. scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "33x20011", "1031x130-f32", "5000x40", "2048x24-f32", "4096x513"])
def test_scores_are_those_of_scores_missing(name, gpu, handle, results):
    torch = _torch()
    st = CASES[name][4]
    X, _, m = xd_case(name)
    S = handle.scores_missing(_dev(X, _tdt(st)), torch.from_numpy(np.array(m["W"])).cuda(), torch.from_numpy(np.array(m["P"])).cuda())
    e = rel(results(name)["S"], S.cpu().numpy())
    print(f"[xdiag-missing] {name}: S vs scores_missing {e:.2e}")
    assert e <= (TOL_F32 if st == "f32" else TOL_F64)


# ---- 3. complete data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "257x33-m3", "5000x40"])
def test_complete_data_equals_x_diagnostics(name, gpu, handle):
    N, K, M, A, frac, st = FIT_CASES[name]
    _, Y, Xc = case_data(name)
    Xd = _dev(Xc, _tdt(st))
    m = handle.fit_missing(Xd, _dev(Y, _tdt(st)), A, want=("W", "P", "R"))
    got = _np(handle.x_diagnostics_missing(Xd, m["W"], m["P"], want=OUT))
    ref = _np(handle.x_diagnostics(Xd, m["R"], m["P"], want=("Q", "T2", "S", "ssx", "sst")))
    e = {k: rel(got[k], ref[k]) for k in ref}
    e["Qrow"] = worst_row(got["Q"], ref["Q"])
    print(f"[xdiag-missing] {name} complete data vs x_diagnostics: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL_F64, e
    assert (got["nobs"] == K).all()


# ---- 4. tvar --------------------------------------------------------------------------------------------------------------------
def _heldout(name, n=37, frac=0.2):
    """rows the model has not seen, mixtures of the case's complete rows, with their own NaN pattern"""
    N, K, A, _, st, _, _ = CASES[name]
    _, Xc, _ = xd_case(name)
    rng = np.random.default_rng([7] + [int(b) for b in name.encode()])
    r = min(N, 12)
    Xn = rng.standard_normal((n, r)) @ Xc[:r] / np.sqrt(r) + 0.05 * rng.standard_normal((n, K))
    if st == "f32":
        Xn = Xn.astype(np.float32).astype(np.float64)
    Xn[rng.random((n, K)) < frac] = np.nan
    return np.asfortranarray(Xn)


@pytest.mark.parametrize("name", ["130x70", "1031x130-f32", "5000x40"])
def test_tvar(name, gpu, handle, results):
    torch = _torch()
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    base = results(name)
    # given tvar = sst / (N - 1): the bits of T2 with tvar = None
    tv = torch.from_numpy(base["sst"] / float(N - 1)).cuda()   # (divided on the host: torch multiplies by the reciprocal)
    again = run(handle, X, m, st, tvar=tv, want=("T2",))
    assert again["T2"].tobytes() == base["T2"].tobytes()
    # new rows, another N, their own NaN pattern, under the training tvar.  2100 rows put 5000x40's on the resident route too.
    Xn = _heldout(name, 2100 if route == RESIDENT else 37)
    got = run(handle, Xn, m, st, tvar=tv)
    check(got, xdiag_missing_ref(Xn, m["W"], m["P"], tvar=tv.cpu().numpy()), st, f"{name}: {Xn.shape[0]} new rows under the training tvar")


# ---- 5. subsets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "1031x130-f32", "5000x40", "2048x24-f32"])
def test_each_output_alone_has_the_bits_it_has_among_all(name, gpu, handle, results):
    X, _, m = xd_case(name)
    st = CASES[name][4]
    Xd = _dev(X, _tdt(st))
    base = _bits(results(name))
    for k in OUT:
        got = _bits(run(handle, Xd, m, st, want=(k,)))
        assert list(got) == [k] and got[k] == base[k], (name, k)
    got = _bits(run(handle, Xd, m, st, want=("ssx", "S")))
    assert got["ssx"] == base["ssx"] and got["S"] == base["S"]


# ---- 6. bounds and inputs -------------------------------------------------------------------------------------------------------
PAYLOADS = {8: (0xFFF8000000000000, 0x7FF800000BADC0DE, 0x7FF0000000000001, 0xFFF4000000000123),
            4: (0xFFC00000, 0x7FC0BEEF, 0x7F800001, 0xFFA00123)}


def _raw(handle, Xin, n, K, A, m, tv, st, layout):
    """the C entry with X placed among 1e300 cells and every output, W, P and tvar between guard cells"""
    from pls_amd import _lib as L
    from test_gpu_bounds import Guarded
    torch = _torch()
    gin = Guarded([(K, A, K), (K, A, K), (A, 1, A)], torch.float64, layout)
    gin[0].copy_(torch.from_numpy(np.array(m["W"]))); gin[1].copy_(torch.from_numpy(np.array(m["P"])))
    gin[2].copy_(torch.from_numpy(np.array(tv)).reshape(A, 1))
    snap = gin.raw.clone()
    g64 = Guarded([(n, A), (n, A), (A + 1, 1, A + 1), (A, 1, A), (n, 1, n)], torch.float64, layout)
    gS = Guarded([(n, A)], _tdt(st), layout)
    rc = L.lib().pls_hip_x_diagnostics_missing(handle.h, Xin.ptr(), Xin.ld, n, K, A, gin.ptr(0), gin.ptr(1), gin.ptr(2),
                                               L.F32 if st == "f32" else L.F64, L.MEM_DEVICE, g64.ptr(0), g64.ld(0), g64.ptr(1), g64.ld(1),
                                               gS.ptr(0), gS.ld(0), g64.ptr(2), g64.ptr(3), g64.ptr(4))
    L.check(rc, handle.h)
    handle.synchronize()
    g64.check(); gS.check()
    assert bool((gin.raw == snap).all()), "W, P, tvar or their surroundings were modified"
    Xin.check()
    out = dict(Q=g64[0], T2=g64[1], ssx=g64[2][:, 0], sst=g64[3][:, 0], S=gS[0])
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out["nobs"] = g64.bits(4).cpu().numpy()[:, 0].copy()
    return out


@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("name", ["67x19", "130x70", "1031x130-f32", "5000x40", "2048x24-f32", "4096x513"])
def test_bounds_and_inputs(name, layout, gpu, handle, results):
    from test_gpu_missing import BIG, PlacedInput
    torch = _torch()
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    ref = case_ref(name)
    tv = ref["sst"] / (N - 1)
    Xin = PlacedInput(X, _tdt(st), layout)
    got = _raw(handle, Xin, N, K, A, m, tv, st, layout)
    check(got, xdiag_missing_ref(X, m["W"], m["P"], tvar=tv), st, f"{name} {layout}")
    base = {k: np.ascontiguousarray(v).tobytes() for k, v in got.items()}
    if layout == "aligned":   # the layout of the shared results: the same bits but for T2, whose tvar came from the host here
        shared = _bits(results(name))
        for k in ("Q", "S", "ssx", "sst", "nobs"):
            assert base[k] == shared[k], (name, k)
    # the result does not depend on what the padding rows and the cells around X hold
    keep = Xin.view.clone()
    Xin.flat.fill_(-7.25)
    Xin.view.copy_(keep)
    Xin.snap = Xin.flat.view(Xin.idt).clone()
    again = _raw(handle, Xin, N, K, A, m, tv, st, layout)
    for k in OUT:
        assert np.ascontiguousarray(again[k]).tobytes() == base[k], (name, layout, k, "padding")
    # ... nor on the payload or the sign of the NaN: quiet, signalling, negative
    es = 4 if st == "f32" else 8
    nan = torch.isnan(Xin.view)
    for pat in PAYLOADS[es]:
        signed = pat - (1 << (8 * es)) if pat >> (8 * es - 1) else pat
        cells = torch.full((int(nan.sum()),), signed, dtype=torch.int32 if es == 4 else torch.int64, device="cuda").view(_tdt(st))
        Xin.view[nan] = cells
        assert bool((torch.isnan(Xin.view) == nan).all())
        Xin.snap = Xin.flat.view(Xin.idt).clone()
        again = _raw(handle, Xin, N, K, A, m, tv, st, layout)
        for k in OUT:
            assert np.ascontiguousarray(again[k]).tobytes() == base[k], (name, layout, k, hex(pat))


# ---- 7. host = device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["67x19", "130x70", "1031x130-f32", "5000x40", "2048x24-f32"])
def test_host_memory_returns_the_bits_of_device_memory(name, gpu, handle, results):
    """the host-memory call stages X with 16-byte columns and W, P packed: the layout of the shared device results"""
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    Xh = np.asfortranarray(X.astype(np.float32) if st == "f32" else X)
    got = handle.x_diagnostics_missing(Xh, np.array(m["W"]), np.array(m["P"]), want=OUT)
    base = _bits(results(name))
    for k in OUT:
        assert isinstance(got[k], np.ndarray) and np.ascontiguousarray(got[k]).tobytes() == base[k], (name, k)
    tv = results(name)["sst"] / (N - 1)
    one = handle.x_diagnostics_missing(Xh, np.array(m["W"]), np.array(m["P"]), tvar=tv, want=("T2",))
    assert one["T2"].tobytes() == base["T2"]


# ---- 8. determinism and history -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "5000x40", "1031x130-f32"])
def test_same_bits_whatever_the_handle_ran_before(name, gpu, results):
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    _, Y, _ = case_data(name)
    Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
    base = _bits(results(name))   # (the session's handle, with whatever the tests before left in it)
    h = pls_amd.Handle()          # a fresh handle
    try:
        first = _bits(run(h, Xd, m, st))
        assert first == base
        assert _bits(run(h, Xd, m, st)) == base   # the same call twice
        h.fit_missing(Xd, Yd, A)
        h.cv_folds_missing(Xd, Yd, 2, np.arange(10).reshape(5, 2))
        with pytest.raises(pls_amd.PlsHipError) as e:   # a refused call
            h.x_diagnostics_missing(Xd, torch.zeros(K, K + 1, dtype=torch.float64, device="cuda"),
                                    torch.zeros(K, K + 1, dtype=torch.float64, device="cuda"))
        assert e.value.code == L.ERR_INVALID
        # another shape in between: the workspace is sized and left behind by it
        big = np.asfortranarray(np.random.default_rng(5).standard_normal((3000, K)))
        run(h, big, m, "f64")
        assert _bits(run(h, Xd, m, st)) == base
    finally:
        h.close()


# ---- 9. edges -------------------------------------------------------------------------------------------------------------------
def _random_model(K, A, seed):
    rng = np.random.default_rng(seed)
    return dict(W=np.asfortranarray(rng.standard_normal((K, A))), P=np.asfortranarray(rng.standard_normal((K, A))))


@pytest.mark.parametrize("name", ["67x19", "5000x40"])
def test_empty_row_and_column(name, gpu, handle):
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    Xe = np.array(X, order="F")
    Xe[5, :] = np.nan
    Xe[:, 7] = np.nan
    got = run(handle, Xe, m, st)
    for k in ("S", "Q", "T2"):
        assert not got[k][5].any(), k
    assert got["nobs"][5] == 0
    check(got, xdiag_missing_ref(Xe, m["W"], m["P"]), st, f"{name} with an empty row and an empty column")


@pytest.mark.parametrize("N,K,A", [(40, 6, 6), (3000, 6, 6), (50, 1, 1), (2500, 1, 1), (1, 9, 3)])
def test_small_shapes(N, K, A, gpu, handle):
    """A = K, K = 1 (both routes), N = 1 with tvar given: any W and P are a model"""
    rng = np.random.default_rng([N, K, A])
    X = np.asfortranarray(rng.standard_normal((N, K)))
    X[rng.random((N, K)) < 0.15] = np.nan
    m = _random_model(K, A, 3)
    tv = np.linspace(1.0, 2.0, A) if N == 1 else None
    got = run(handle, X, m, "f64", tvar=tv)
    check(got, xdiag_missing_ref(X, m["W"], m["P"], tvar=tv), "f64", f"{N}x{K}, A = {A}")


def test_one_row_without_tvar_is_refused_only_for_t2(gpu, handle):
    import pls_amd
    from pls_amd import _lib as L
    X = np.asfortranarray(np.array([[1.0, np.nan, -2.0, 0.5]]))
    m = _random_model(4, 2, 1)
    with pytest.raises(pls_amd.PlsHipError) as e:
        run(handle, X, m, "f64", want=("T2",))
    assert e.value.code == L.ERR_INVALID
    got = run(handle, X, m, "f64", want=("Q", "S", "ssx", "sst", "nobs"))
    check(got, xdiag_missing_ref(X, m["W"], m["P"], tvar=np.ones(2)), "f64", "1x4 without T2")


@pytest.mark.parametrize("name", ["130x70", "5000x40"])
def test_a_zero_in_tvar(name, gpu, handle, results):
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    base = results(name)
    tv = base["sst"] / (N - 1)
    tv[1] = 0.0
    got = run(handle, X, m, st, tvar=tv)
    assert got["T2"][:, 0].tobytes() == base["T2"][:, 0].tobytes()
    assert not np.isfinite(got["T2"][:, 1:]).any()
    for k in ("Q", "S", "ssx", "sst", "nobs"):
        assert got[k].tobytes() == base[k].tobytes(), k


# ---- 10. statuses ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_untouched(gpu):
    import pls_amd
    from pls_amd import _lib as L
    from test_gpu_bounds import Guarded
    torch = _torch()
    N, K, A = 50, 20, 3
    h = pls_amd.Handle()
    try:
        X = h.synth_x(0, N, K, 3)
        ld = int(X.stride(1))
        WP = torch.ones(2, K * A, dtype=torch.float64, device="cuda")
        W, P = WP[0].data_ptr(), WP[1].data_ptr()
        tv = torch.ones(A, dtype=torch.float64, device="cuda").data_ptr()

        def call(Xp=X.data_ptr(), ldx=ld, N_=N, K_=K, A_=A, Wp=W, Pp=P, tvp=tv, short=None, only=None):
            g = Guarded([(N, A), (N, A), (N, A), (A + 1, 1, A + 1), (A, 1, A), (N, 1, N)], torch.float64, "aligned")
            lds = [N - 1 if short == i else g.ld(i) for i in range(3)]
            ptr = lambda i: g.ptr(i) if only is None or i in only else None
            rc = L.lib().pls_hip_x_diagnostics_missing(h.h, Xp, ldx, N_, K_, A_, Wp, Pp, tvp, L.F64, L.MEM_DEVICE, ptr(0), lds[0], ptr(1), lds[1],
                                                       ptr(2), lds[2], ptr(3), ptr(4), ptr(5))
            h.synchronize()
            g.assert_untouched()
            for i in range(len(g)):
                g.assert_prefilled(i)
            return rc
        assert call(N_=0) == L.ERR_INVALID
        assert call(A_=0) == L.ERR_INVALID
        assert call(A_=K + 1) == L.ERR_INVALID
        assert call(ldx=N - 1) == L.ERR_INVALID
        for i in range(3):   # the ld of Qres, T2, S, each asked for
            assert call(short=i) == L.ERR_INVALID
        assert call(Xp=None) == L.ERR_INVALID
        assert call(Wp=None) == L.ERR_INVALID
        assert call(Pp=None) == L.ERR_INVALID
        assert call(N_=1, tvp=None) == L.ERR_INVALID          # T2 from the call's own scores needs two rows
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        try:
            assert call() == L.ERR_UNSUPPORTED
        finally:
            h.clear_reducer()
        # a short ld of an output that is NOT asked for is no error, and the handle is healthy
        g = Guarded([(N, A)], torch.float64, "aligned")
        rc = L.lib().pls_hip_x_diagnostics_missing(h.h, X.data_ptr(), ld, N, K, A, W, P, tv, L.F64, L.MEM_DEVICE, g.ptr(0), g.ld(0), None, 0,
                                                   None, 0, None, None, None)
        L.check(rc, h.h)
        h.synchronize()
        g.check()
        assert np.isfinite(g[0].cpu().numpy()).all()
    finally:
        h.close()


# ---- 11. long leading dimensions --------------------------------------------------------------------------------------------------
if __name__ != "__main__":
    from test_gpu_long_ld import arena  # noqa: E402,F401  (the module-scoped fixture: one flat allocation for all cases)

LONG_CASES = [("130x70", 160, "XQTS"), ("5000x40", 320, "XQS"), ("1031x130-f32", "total", "XS")]


@pytest.mark.parametrize("name,pitch,long", LONG_CASES)
def test_long_leading_dimensions(arena, handle, name, pitch, long):   # noqa: F811
    from pls_amd import _lib as L
    from test_gpu_long_ld import _both, _code, _ldv, _ptr, case_ld
    import pls_amd
    torch = _torch()
    N, K, A, frac, st, route, rt = CASES[name]
    X, _, m = xd_case(name)
    ld = case_ld(pitch, st, K)
    W = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K); W.copy_(torch.from_numpy(np.array(m["W"])))
    P = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K); P.copy_(torch.from_numpy(np.array(m["P"])))

    def call(lay):
        Xd = lay.inp("X", X)
        Q, T2 = lay.out("Q", N, A, torch.float64), lay.out("T", N, A, torch.float64)
        S = lay.out("S", N, A)
        ssx, sst = torch.empty(A + 1, dtype=torch.float64, device="cuda"), torch.empty(A, dtype=torch.float64, device="cuda")
        nobs = torch.empty(N, dtype=torch.int64, device="cuda")
        L.check(L.lib().pls_hip_x_diagnostics_missing(handle.h, _ptr(Xd), _ldv(Xd), N, K, A, _ptr(W), _ptr(P), None, _code(st), L.MEM_DEVICE,
                                                      _ptr(Q), _ldv(Q), _ptr(T2), _ldv(T2), _ptr(S), _ldv(S), _ptr(ssx), _ptr(sst), _ptr(nobs)),
                handle.h)
        handle.synchronize()
        return _np(dict(Q=Q, T2=T2, S=S, ssx=ssx, sst=sst, nobs=nobs))

    got, twin = _both(arena, st, ld, long, call, fill="huge")
    check(got, case_ref(name), st, f"{name} long ld {pitch} {long}")
    for k in OUT:   # the compact twin is 16-byte aligned as well: the same geometry, the same bits
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(twin[k]).tobytes(), (name, k)


# ---- 12. the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["130x70", "1031x130-f32"])
def test_model_x_diagnostics_with_missing_cells(name, gpu, handle):
    import pls_amd
    N, K, M, A, frac, st = FIT_CASES[name]
    X, Y, _ = case_data(name)
    Xd, Yd = _dev(X, _tdt(st)), _dev(Y, _tdt(st))
    model = pls_amd.Model(Xd, Yd, max_components=A, handle=handle, missing=True)
    d = _np(model.x_diagnostics())
    # the yardstick at the model's own W, P and tvar = t_a^T t_a / (N - 1) of its T: with fp32 storage the device fit keeps its work
    # copy in fp32, so its W and P are 1e-7 from the fp64 fit of the same data and so is everything derived from them
    Wm, Pm, Tm = (np.asarray(v.cpu().numpy(), dtype=np.float64) for v in (model.W, model.P, model.T))
    tvm = (Tm * Tm).sum(axis=0) / (N - 1)

    def held(got, ref, what):
        e = dict(Q=rel(got["Q"], ref["Q"]), Qrow=worst_row(got["Q"], ref["Q"]), T2=rel(got["T2"], ref["T2"]),
                 R2X=rel(got["R2X"], 1.0 - ref["ssx"][1:] / ref["ssx"][0]))
        print(f"[xdiag-missing] {name} {what}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert all(np.isfinite(got[k]).all() for k in ("Q", "T2", "R2X"))
        assert max(e.values()) <= TOL_F64, e
        assert np.array_equal(got["nobs"], ref["nobs"])
    ref = xdiag_missing_ref(X, Wm, Pm, tvar=tvm)
    held(d, ref, "Model.x_diagnostics()")
    if st == "f64":   # ... which for fp64 storage is the case's yardstick
        assert rel(d["Q"], case_ref(name)["Q"]) <= TOL_F64 and rel(d["T2"], case_ref(name)["T2"]) <= TOL_F64
    Xn = _heldout(name)
    held(_np(model.x_diagnostics(_dev(Xn, _tdt(st)))), xdiag_missing_ref(Xn, Wm, Pm, tvar=tvm), "Model.x_diagnostics(new rows)")
    # numpy inputs: host memory
    mh = pls_amd.Model(np.asfortranarray(X.astype(np.float32)) if st == "f32" else X, np.asfortranarray(Y.astype(np.float32)) if st == "f32" else Y,
                       max_components=A, handle=handle, missing=True)
    dh = mh.x_diagnostics()
    Th = np.asarray(mh.T, dtype=np.float64)
    held(dh, xdiag_missing_ref(X, np.asarray(mh.W), np.asarray(mh.P), tvar=(Th * Th).sum(axis=0) / (N - 1)), "Model.x_diagnostics(), host memory")


def test_a_plsr_model_keeps_its_route(gpu, handle):
    import pls_amd
    name = "130x70"
    N, K, M, A, frac, st = FIT_CASES[name]
    _, Y, Xc = case_data(name)
    Xd, Yd = _dev(Xc, _tdt(st)), _dev(Y, _tdt(st))
    model = pls_amd.Model(Xd, Yd, max_components=A, handle=handle)
    d = model.x_diagnostics()
    assert sorted(d) == ["Q", "R2X", "T2"]
    out = handle.x_diagnostics(Xd, model.R, model.P, tvar=model._tvar(), want=("Q", "T2", "ssx"))
    ssx = out["ssx"]
    ref = dict(Q=out["Q"], T2=out["T2"], R2X=1.0 - ssx[1:] / ssx[0])
    assert _bits(d) == _bits(ref)


# ---- the child process of test_resident_cases_on_the_streaming_route ----------------------------------------------------------
if __name__ == "__main__":
    import pls_amd
    _torch().cuda.set_device(0)
    assert os.environ.get("PLS_HIP_XDIAGMISS_ROUTE") == "stream"
    h = pls_amd.Handle()
    for name in sys.argv[1:]:
        st = CASES[name][4]
        X, _, m = xd_case(name)
        got, n = xb_launches(h, lambda: run(h, X, m, st))
        print(json.dumps(dict(name=name, xb=n, err=errors(got, case_ref(name), st))), flush=True)
    h.close()
