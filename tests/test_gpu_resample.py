"""pls_hip_fit_resampled on the GPU (pls_amd/csrc/plan_resample.hpp): the same (X, Y) under many sets of row weights -- under
PLS_HIP_ALGO_DUAL every replicate from one G = X X^T, otherwise one refit of row-scaled copies per replicate.  Cases, yardstick
(the oracle on physically repeated or scaled rows) and bars are those of tests/test_resample_ref.py."""
import contextlib

import numpy as np
import pytest

from conftest import handle_with_env
from test_dual_cv_ref import BAR
from test_dual_ref import TOL_B
from test_gpu_bounds import Guarded, Inputs, _place
from test_resample_ref import CASES, GENERAL_ONLY, case_data, case_yardstick, check

pytestmark = pytest.mark.gpu

NAMES = ("Q", "tt", "B", "B0", "Bmean", "Bm2")
DUAL_CASES = [n for n in CASES if n not in GENERAL_ONLY]


def _torch():
    import torch
    return torch


@pytest.fixture
def dual(handle):
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    yield handle
    handle.set_option(pls_amd.OPT_ALGO, 0)


@contextlib.contextmanager
def dual_handle(**env):
    """a fresh handle under the environment switches given, with the option set"""
    import pls_amd
    with handle_with_env(**env) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        yield h


def _dev(a, dt="f64"):
    import pls_amd
    torch = _torch()
    t = torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)
    return pls_amd.as_colmajor(t.to(torch.float32) if dt == "f32" else t)


def _as_np(out):
    torch = _torch()
    return {k: np.ascontiguousarray((v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64))
            for k, v in out.items()}


def run(h, name, mem="device", want=NAMES, weights=None):
    N, K, M, A, nrep, dt, _ = CASES[name]
    X, Y, Wt = case_data(name)
    Wt = Wt if weights is None else weights
    if mem == "device":
        out = h.fit_resampled(_dev(X, dt), _dev(Y, dt), A, _dev(Wt), want=want)
        h.synchronize()
    else:
        ndt = np.float32 if dt == "f32" else np.float64
        out = h.fit_resampled(np.asfortranarray(X.astype(ndt)), np.asfortranarray(Y.astype(ndt)), A, Wt, want=want)
    return _as_np(out)


def _same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


def _shapes_ok(got, name):
    N, K, M, A, nrep, _, _ = CASES[name]
    assert got["Q"].shape == (nrep, M, A) and got["tt"].shape == (nrep, A) and got["B"].shape == (nrep, K, M)
    assert got["B0"].shape == got["Bmean"].shape == got["Bm2"].shape == (K, M)


# ---- 1. the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DUAL_CASES)
def test_resample_parity(dual, name):
    """the sample-space route against the oracle on repeated (or scaled) rows"""
    got = run(dual, name)
    _shapes_ok(got, name)
    check(got, case_yardstick(name), name + " device")


@pytest.mark.parametrize("name", ["17x1003", "97x1500", "1031x3000-f32"])
def test_resample_host_and_device_memory_return_the_same_bits(dual, name):
    got = run(dual, name)
    host = run(dual, name, "host")
    check(host, case_yardstick(name), name + " host")
    assert _same_bits(got, host)


# ---- 2. rounds ----------------------------------------------------------------------------------------------------------------
def test_resample_ragged_rounds(dual):
    """141 items in rounds of 37 (a ragged last one): at the bars of the yardstick, and the summaries within the same bars of
    the uncapped run (not bitwise: the product kernel is chosen by round size)"""
    from oracle import pls_oracle as po
    name = "130x600"
    y = case_yardstick(name)
    full = run(dual, name)
    with dual_handle(PLS_HIP_RESAMPLE_ROUND=37) as h:
        capped = run(h, name)
    check(capped, y, name + " rounds of 37")
    for k in ("B0", "Bmean"):
        assert po.rel_fro(capped[k], full[k]) < TOL_B, k
    se = lambda o: np.sqrt(np.maximum(o["Bm2"], 0.0))
    assert po.rel_fro(se(full), se(capped)) < 2.0 * TOL_B / y["rho"]
    with dual_handle(PLS_HIP_RESAMPLE_ROUND=1) as h:  # one replicate per round, the unit-weight fit alone in the first
        check(run(h, "17x1003"), case_yardstick("17x1003"), "17x1003 rounds of 1")


# ---- 3. the general route -----------------------------------------------------------------------------------------------------
def test_resample_general_route_default_plan(handle):
    """5000 x 64 on a default-plan handle: row-scaled refits, same yardstick, same bars; host memory too"""
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, 0)
    name = "5000x64"
    got = run(handle, name)
    _shapes_ok(got, name)
    check(got, case_yardstick(name), name + " general route")
    host = run(handle, name, "host", want=("B0", "Bmean", "Bm2", "tt"))
    check(host, case_yardstick(name), name + " general route, host")


def test_resample_refit_switch_is_the_cross_check(dual):
    """PLS_HIP_RESAMPLE_REFIT=1 under the option keeps the general route; the two agree within the bars"""
    name = "97x1500"
    got = run(dual, name)
    with dual_handle(PLS_HIP_RESAMPLE_REFIT=1) as h:
        refit = run(h, name)
    check(refit, case_yardstick(name), name + " refit under ALGO_DUAL")
    assert not _same_bits(refit, got)  # (two routes)


# ---- 4. the jack-knife against the cross-validation folds ---------------------------------------------------------------------
def test_resample_leave_one_out_agrees_with_cv_folds(dual):
    """replicate f of jackknife_weights leaves row f out: Y[f] - X[f] B_f is the last column of pls_hip_cv_folds' residuals"""
    name = "nir-loo"
    N, K, M, A, nrep, dt, _ = CASES[name]
    X, Y, Wt = case_data(name)
    B = run(dual, name, want=("B",))["B"]
    E = dual.cv_folds(_dev(X), _dev(Y), A, np.arange(N)[:, None]).cpu().numpy()  # (M, nobs, A)
    res = np.stack([Y[f] - X[f] @ B[f] for f in range(N)])  # (N, M)
    ref = E[:, :, A - 1].T
    err = np.abs(res - ref).max() / max(np.abs(ref).max(), 1.0)
    print(f"[resample] {name}: max|Y[f] - X[f] B_f - E[f, A-1]| / max(max|E|, 1) = {err:.2e}")
    assert err < BAR


def test_model_bootstrap_and_jackknife(dual):
    import pls_amd
    name = "nir-loo"
    N, K, M, A, nrep, dt, _ = CASES[name]
    X, Y, Wt = case_data(name)
    y = case_yardstick(name)
    from oracle import pls_oracle as po
    for where in ("device", "host"):
        Xi, Yi = (_dev(X), _dev(Y)) if where == "device" else (np.array(X), np.array(Y))
        m = pls_amd.Model(Xi, Yi, pls_amd.KERNEL_TYPE1, A, handle=dual)
        jk = _as_np(m.jackknife())
        assert po.rel_fro(jk["B0"], y["B0"]) < TOL_B and po.rel_fro(jk["Bmean"], y["Bmean"]) < TOL_B
        assert po.rel_fro(y["se"] * np.sqrt((N - 1.0) / N), jk["se"]) < 2.0 * TOL_B / y["rho"]
        bs = _as_np(m.bootstrap(20, seed=3))
        ref = run(dual, name, want=("Bm2",), weights=pls_amd.bootstrap_weights(N, 20, 3))
        assert np.array_equal(bs["se"], pls_amd.resample_se(ref["Bm2"], 20, "bootstrap")), where
        assert np.isfinite(bs["se"]).all() and (bs["se"] > 0).any()


# ---- 5. unit weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [("17x1003", 0), ("97x1500", 0), ("130x600", 0), ("130x600", 37)])
def test_resample_unit_weights_are_exact(name, cap):
    """every replicate of unit weights: B_b == B0 bit for bit whatever round it falls into, so Bm2 == 0 and Bmean == B0
    exactly; B0 within TOL_B of fit_batch's B under the option"""
    from oracle import pls_oracle as po
    N, K, M, A, nrep, dt, _ = CASES[name]
    X, Y, _ = case_data(name)
    env = dict(PLS_HIP_RESAMPLE_ROUND=cap) if cap else {}
    with dual_handle(**env) as h:
        got = run(h, name, weights=np.ones((N, nrep)))
        fb = _as_np(h.fit_batch(_dev(X, dt), _dev(Y, dt), M, A, want=("B",)))["B"][0]
    assert not got["Bm2"].any()
    assert np.array_equal(got["Bmean"], got["B0"])
    for b in range(nrep):
        assert np.array_equal(got["B"][b], got["B0"]), b
    assert po.rel_fro(got["B0"], fb) < TOL_B


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------
def test_resample_is_deterministic(dual):
    """the same bits twice on one handle and once on a fresh one"""
    name = "130x600"
    first = run(dual, name)
    assert _same_bits(first, run(dual, name))
    with dual_handle() as h:
        assert _same_bits(first, run(h, name))


def test_resample_every_output_alone(dual):
    """an output asked for alone carries the bits it has among all of them"""
    name = "17x1003"
    full = run(dual, name)
    for k in NAMES:
        got = run(dual, name, want=(k,))
        assert set(got) == {k} and np.array_equal(got[k].view(np.int64), full[k].view(np.int64)), k


# ---- 7. one sweep over X ------------------------------------------------------------------------------------------------------
def test_resample_q_alone_sweeps_x_once():
    """every output NULL except Q: G is the only launch over X (no back-projection), for 3 replicates as for 40"""
    import pls_amd
    N, K, A = 60, 20000, 4
    with dual_handle() as h:
        X = h.synth_x(0, N, K, 5)
        Y = h.synth_y(0, N, 1, 5)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        for nrep in (3, 40):
            Wt = _dev(pls_amd.bootstrap_weights(N, nrep, 1))
            h.timing()
            h.fit_resampled(X, Y, A, Wt, want=("Q",))
            h.synchronize()
            t = h.timing()
            assert t["launches"]["xty"] == 1 and t["bytes"]["xty"] == N * K * 8 + N * N * 8, t
            assert t["launches"]["xb"] == 0 and t["launches"]["deflate"] == 0 and t["launches"]["fused"] == 0, t
            h.fit_resampled(X, Y, A, Wt, want=("Q", "Bm2"))
            h.synchronize()
            assert h.timing()["launches"]["xty"] == 3  # G, B0, the round's B
        h.set_option(pls_amd.OPT_PROFILE, 0)


# ---- 8. guarded buffers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [NAMES, ("B",), ("Q", "Bm2"), ("B0",), ()], ids=["all", "B", "Q-Bm2", "B0", "none"])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("route", ["dual", "refit"])
def test_resample_writes_exactly_its_outputs(route, layout, want):
    """each requested output fully written, the others, the guards and the inputs untouched, on both routes ("eigen": odd
    leading dimension, pointers aligned to 8 bytes only)"""
    from pls_amd import _lib as L
    torch = _torch()
    name = "17x1003"
    N, K, M, A, nrep, dt, _ = CASES[name]
    Xh, Yh, Wh = case_data(name)
    gx, X = _place(Xh, torch.float64, layout)
    gy, Y = _place(Yh, torch.float64, layout)
    gw, W = _place(Wh, torch.float64, layout)
    snap = Inputs(X=X, Y=Y, W=W)
    go = Guarded([(M * A, nrep, M * A), (A, nrep, A), (K * M, nrep, K * M), (K, M, K), (K, M, K), (K, M, K)], torch.float64, layout)
    with dual_handle(**(dict(PLS_HIP_RESAMPLE_REFIT=1) if route == "refit" else {})) as h:
        rc = L.lib().pls_hip_fit_resampled(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A, gw.ptr(0), gw.ld(0), nrep,
                                           L.F64, L.MEM_DEVICE, *[go.ptr(i) if k in want else None for i, k in enumerate(NAMES)])
        L.check(rc, h.h)
        h.synchronize()
    go.assert_untouched()
    gx.assert_untouched(); gy.assert_untouched(); gw.assert_untouched()
    snap.check()
    for i, k in enumerate(NAMES):
        if k in want:
            go.assert_written(i)
        else:
            go.assert_prefilled(i)
    arr = lambda i: go[i].cpu().numpy().astype(np.float64)
    got = dict(Q=arr(0).T.reshape(nrep, A, M).transpose(0, 2, 1), tt=arr(1).T, B=arr(2).T.reshape(nrep, M, K).transpose(0, 2, 1),
               B0=arr(3), Bmean=arr(4), Bm2=arr(5))
    check({k: got[k] for k in want}, case_yardstick(name), f"guarded {route} {layout} {want}")


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_resample_refusals_leave_the_outputs_alone(dual):
    """a reducer: PLS_HIP_ERR_UNSUPPORTED; A > K, ldw < N, nrep = 0: PLS_HIP_ERR_INVALID; the outputs keep their fill pattern"""
    from pls_amd import _lib as L
    torch = _torch()
    name = "17x1003"
    N, K, M, A, nrep, dt, _ = CASES[name]
    Xh, Yh, Wh = case_data(name)
    gx, X = _place(Xh, torch.float64, "aligned")
    gy, Y = _place(Yh, torch.float64, "aligned")
    gw, W = _place(Wh, torch.float64, "aligned")
    go = Guarded([(M * A, nrep, M * A), (A, nrep, A), (K * M, nrep, K * M), (K, M, K), (K, M, K), (K, M, K)], torch.float64)

    def call(h, A_=A, ldw=None, nrep_=nrep):
        return L.lib().pls_hip_fit_resampled(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A_, gw.ptr(0),
                                             gw.ld(0) if ldw is None else ldw, nrep_, L.F64, L.MEM_DEVICE,
                                             *[go.ptr(i) for i in range(len(NAMES))])

    def untouched():
        dual.synchronize()
        go.assert_untouched()
        for i in range(len(NAMES)):
            go.assert_prefilled(i)

    assert call(dual, A_=K + 1) == L.ERR_INVALID
    assert call(dual, ldw=N - 1) == L.ERR_INVALID
    assert call(dual, nrep_=0) == L.ERR_INVALID
    untouched()
    with dual_handle() as h:
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        assert call(h) == L.ERR_UNSUPPORTED
        h.synchronize()
        h.clear_reducer()
    untouched()
    assert call(dual) == L.OK  # (... and the same call without any of that is taken)
    dual.synchronize()
    go.check()
