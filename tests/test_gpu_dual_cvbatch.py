"""Cross-validated fits of many response sets (pls_hip_cv_press_batch, pls_amd/csrc/plan_dual_cvbatch.hpp) on the GPU: under
PLS_HIP_ALGO_DUAL every (problem, fold) pair from one G = X X^T, PRESS and ssy reduced on the device; every other handle one
cross-validation per problem.  Cases, reference (one oracle refit per fold and problem) and bars are those of
tests/test_dual_cvbatch_ref.py."""
import ctypes

import numpy as np
import pytest

from conftest import handle_with_env
from test_dual_cv_ref import BAR, CASES, case_data, rel_err
from test_dual_cvbatch_ref import CASES_B, PRESS_TOL, case_data_b, case_reference_b, press_err, ssy_of
from test_gpu_bounds import Guarded, Inputs, _place

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture
def dual(handle):
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    yield handle
    handle.set_option(pls_amd.OPT_ALGO, 0)


def _dev(a, dt="f64"):
    import pls_amd
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return pls_amd.as_colmajor(t.to(torch.float32) if dt == "f32" else t)


def _case(name):
    """(X, Ys) on the device in the case's storage type, their host images in that type, M, A, idx, nprob"""
    X, Ys, M, A, idx, nprob = case_data_b(name)
    dt = CASES[CASES_B[name][0]][6]
    npdt = np.float32 if dt == "f32" else np.float64
    return _dev(X, dt), _dev(Ys, dt), np.asfortranarray(X.astype(npdt)), np.asfortranarray(Ys.astype(npdt)), M, A, idx, nprob


def _np(o):
    torch = _torch()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).copy() for k, v in o.items()}


ALL = ("PRESS", "ssy", "E")


def _check(E, ref, what):
    err = rel_err(E, ref)
    print(f"{what}: max|E - ref| / max(max|ref|, 1) = {err:.2e}")
    assert err < BAR, what


def _rel_entries(got, want):
    """max over the entries of |got - want| / |want| (0 where both are 0)"""
    d = np.abs(got - want)
    with np.errstate(all="ignore"):
        return float(np.max(np.where(np.abs(want) > 0, d / np.abs(want), np.where(d == 0, 0.0, np.inf))))


def _rel_max(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _check_sums(o, Ysh, M, idx, what):
    perr = press_err(o["PRESS"], o["E"])
    serr = _rel_entries(o["ssy"], ssy_of(np.asarray(Ysh, dtype=np.float64), M, idx))
    print(f"{what}: max rel |PRESS - sum E^2| = {perr:.2e}   max rel |ssy - sum Y^2| = {serr:.2e}")
    assert perr <= PRESS_TOL and serr <= PRESS_TOL, what


@pytest.mark.parametrize("name", list(CASES_B))
def test_cvbatch_parity(dual, name):
    """1: device call and host-memory call against one oracle refit per fold and problem; PRESS and ssy against numpy sums over
    the E of the same call; the host call within 1e-12 max(max|ref|, 1) of the device call"""
    X, Ys, Xh, Ysh, M, A, idx, nprob = _case(name)
    ref = case_reference_b(name)
    d = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    h = _np(dual.cv_press_batch(Xh, Ysh, M, A, idx, want=ALL))
    assert d["PRESS"].shape == (nprob, M, A) and d["ssy"].shape == (nprob, M) and d["E"].shape == ref.shape
    _check(d["E"], ref, name + " device")
    _check(h["E"], ref, name + " host")
    _check_sums(d, Ysh, M, idx, name + " device")
    _check_sums(h, Ysh, M, idx, name + " host")
    delta = 1e-12 * max(np.abs(ref).max(), 1.0)
    assert np.abs(h["E"] - d["E"]).max() < delta
    # residuals within delta of each other: |sum e'^2 - sum e^2| <= 2 delta sum |e| + nobs delta^2 <= 2 delta sqrt(nobs PRESS) + ...
    nobs = idx.size
    assert np.all(np.abs(h["PRESS"] - d["PRESS"]) <= 2 * delta * np.sqrt(nobs * d["PRESS"]) + nobs * delta * delta + PRESS_TOL * d["PRESS"])
    assert np.array_equal(h["ssy"], d["ssy"])


@pytest.mark.parametrize("name", ["97x1500", "130-columns"])
def test_cvbatch_asks_only_for_what_is_needed(dual, name):
    """2: PRESS and ssy with E = NULL are bit-equal to PRESS and ssy with E asked for; two identical calls are bit-equal"""
    X, Ys, _, _, M, A, idx, nprob = _case(name)
    full = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    lean = _np(dual.cv_press_batch(X, Ys, M, A, idx))
    again = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    only = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=("PRESS",)))
    assert set(lean) == {"PRESS", "ssy"} and set(only) == {"PRESS"}
    for k in ("PRESS", "ssy"):
        assert np.array_equal(lean[k], full[k]), k
    assert np.array_equal(only["PRESS"], full["PRESS"])
    for k in ALL:
        assert np.array_equal(again[k], full[k]), k


@pytest.mark.parametrize("name", ["97x1500", "17x1003"])
def test_cvbatch_against_cv_folds_and_validation(dual, name):
    """3: PRESS and E of every problem within 1e-12 relative of cv_folds(X, Y_b) plus validation on the same DUAL handle"""
    X, Ys, _, _, M, A, idx, nprob = _case(name)
    o = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    for b in range(nprob):
        Eb = dual.cv_folds(X, Ys[:, b * M:(b + 1) * M], A, idx)
        press = dual.validation(Eb)[0].cpu().numpy()
        Eb = Eb.cpu().numpy()
        ee, pe = _rel_max(o["E"][b], Eb), _rel_entries(o["PRESS"][b], press)
        print(f"{name} problem {b}: max|E - E_cv| / max|E_cv| = {ee:.2e}   max rel |PRESS - PRESS_val| = {pe:.2e}")
        assert ee <= 1e-12 and pe <= 1e-12, (name, b)


@pytest.mark.parametrize("cap", [1, 5, 7])
def test_cvbatch_rounds(dual, cap):
    """4: with 12 folds per problem, rounds of 5 and 7 make a problem straddle rounds and leave a ragged last round; rounds of 1"""
    import pls_amd
    name = "97x1500"
    X, Ys, _, _, M, A, idx, nprob = _case(name)
    ref = case_reference_b(name)
    one = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    with handle_with_env(PLS_HIP_DUALCVB_ROUND=cap) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        o = _np(h.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    _check(o["E"], ref, f"{name} rounds of {cap}")
    ee, pe, se = _rel_max(o["E"], one["E"]), _rel_entries(o["PRESS"], one["PRESS"]), _rel_entries(o["ssy"], one["ssy"])
    print(f"{name} rounds of {cap} against one round: E {ee:.2e}  PRESS {pe:.2e}  ssy {se:.2e}")
    assert ee <= 1e-12 and pe <= 1e-12 and se <= 1e-12


def test_cvbatch_one_sweep_over_x():
    """5: the route is taken and books one sweep over X and G, for 2 problems as for 9"""
    import pls_amd
    N, K, A, nf = 60, 20000, 4, 6
    rng = np.random.default_rng(nf)
    idx = np.stack([rng.permutation(N)[:5] for _ in range(nf)])
    with handle_with_env() as h:
        X = h.synth_x(0, N, K, 5); Ys = h.synth_y(0, N, 9, 5)
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        for nprob in (2, 9):
            h.timing()
            h.cv_press_batch(X, Ys[:, :nprob], 1, A, idx)
            t = h.timing()
            assert t["bytes"]["xty"] == N * K * 8 + N * N * 8, (nprob, t)
            assert t["launches"]["xty"] == 1, (nprob, t)
            assert t["launches"]["xb"] == 0 and t["launches"]["deflate"] == 0 and t["launches"]["fused"] == 0, (nprob, t)
        h.set_option(pls_amd.OPT_PROFILE, 0)


def test_cvbatch_masking(dual):
    """6: the held-out rows of a problem never reach the model of the fold that holds them out.  As test_dual_cv_masking reads
    it: E = Y_te - pred is formed with ONE rounding, so pred is read off exactly where Y_te = 0, and with the held-out rows of
    fold f0 of problem b0 replaced by zeros, and by other finite values, E of that item must be fl(Y_te - pred) bit for bit.
    The other folds of problem b0 train on those rows and move, as they must; every item of every OTHER problem -- E, PRESS,
    ssy -- must not move by a bit."""
    torch = _torch()
    name = "97x1500"
    X, Ys, _, _, M, A, idx, nprob = _case(name)
    nf, ts = idx.shape
    b0, f0 = 2, 5
    te = torch.from_numpy(idx[f0].copy()).cuda()
    cols = slice(b0 * M, (b0 + 1) * M)
    rng = np.random.default_rng(3)
    Y0 = Ys.clone(); Y0[te, cols] = 0.0
    Y2 = Ys.clone(); Y2[te, cols] = torch.from_numpy(1.0e3 * rng.standard_normal((ts, M))).cuda()
    o1, o0, o2 = (_np(dual.cv_press_batch(X, Yv, M, A, idx, want=ALL)) for Yv in (Ys, Y0, Y2))
    item = lambda o: o["E"][b0][:, f0 * ts:(f0 + 1) * ts]  # (M, ts, A)
    pred = -item(o0)  # exact
    assert np.isfinite(pred).all() and np.abs(pred).max() > 0
    for Yv, o in ((Ys, o1), (Y2, o2)):
        yte = Yv[te, cols].cpu().numpy().T[:, :, None]  # (M, ts, 1)
        assert np.array_equal(item(o), yte - pred)
    others = [b for b in range(nprob) if b != b0]
    for o in (o0, o2):
        for k in ALL:
            assert np.array_equal(o[k][others], o1[k][others]), k
    _check(o1["E"], case_reference_b(name), name)


@pytest.mark.parametrize("name", ["97x1500", "17x1003"])
def test_cvbatch_general_route(dual, name):
    """7: PLS_HIP_CVBATCH_REFIT=1 on a DUAL handle, and the plain call on a handle without the option: both within the bar of the
    reference and within 1e-10 relative on PRESS of the sample-space route"""
    import pls_amd
    X, Ys, _, Ysh, M, A, idx, nprob = _case(name)
    ref = case_reference_b(name)
    s = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    with handle_with_env(PLS_HIP_CVBATCH_REFIT=1) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        r = _np(h.cv_press_batch(X, Ys, M, A, idx, want=ALL))
        lean = _np(h.cv_press_batch(X, Ys, M, A, idx))
    dual.set_option(pls_amd.OPT_ALGO, 0)
    p = _np(dual.cv_press_batch(X, Ys, M, A, idx, want=ALL))
    for what, o in (("refit switch", r), ("plain handle", p)):
        _check(o["E"], ref, f"{name} {what}")
        _check_sums(o, Ysh, M, idx, f"{name} {what}")
        pe = _rel_entries(o["PRESS"], s["PRESS"])
        print(f"{name} {what}: max rel |PRESS - PRESS_sample_space| = {pe:.2e}")
        assert pe <= 1e-10, (name, what)
        assert np.array_equal(o["ssy"], s["ssy"]) or _rel_entries(o["ssy"], s["ssy"]) <= PRESS_TOL
    assert _rel_entries(lean["PRESS"], r["PRESS"]) <= PRESS_TOL and np.array_equal(lean["ssy"], r["ssy"])


def _raw_call(h, gx, gy, N, K, M, A, nprob, idx, ts, nf, out, ys_null=False):
    from pls_amd import _lib as L
    return L.lib().pls_hip_cv_press_batch(h.h, gx.ptr(0), gx.ld(0), None if ys_null else gy.ptr(0), gy.ld(0), N, K, M, A, nprob,
                                          idx.ctypes.data_as(ctypes.c_void_p), ts, nf, L.F64, L.MEM_DEVICE, out.ptr(0), out.ptr(1),
                                          out.ptr(2))


def _outputs(M, A, nobs, nprob, layout):
    torch = _torch()
    return Guarded([(M * A, nprob, M * A), (M, nprob, M), (nobs, nprob * M * A, nobs)], torch.float64, layout)


def test_cvbatch_refusals(dual):
    """8a: nprob = 0, a NULL Ys, an index out of range, test_size >= N: PLS_HIP_ERR_INVALID; a handle with a reducer:
    PLS_HIP_ERR_UNSUPPORTED; the outputs untouched every time"""
    from pls_amd import _lib as L
    torch = _torch()
    name = "17x1003"
    Xh, Ysh, M, A, idx, nprob = case_data_b(name)
    N, K = Xh.shape
    nf, ts = idx.shape
    gx, _ = _place(Xh, torch.float64, "aligned")
    gy, _ = _place(Ysh, torch.float64, "aligned")
    out = _outputs(M, A, nf * ts, nprob, "aligned")
    bad_idx = idx.copy(); bad_idx[3, 0] = N
    neg_idx = idx.copy(); neg_idx[0, 0] = -1
    wide = np.ascontiguousarray(np.tile(np.arange(N, dtype=np.int64), (2, 1)))  # test_size = N
    calls = {
        "nprob = 0": lambda: _raw_call(dual, gx, gy, N, K, M, A, 0, idx, ts, nf, out),
        "NULL Ys": lambda: _raw_call(dual, gx, gy, N, K, M, A, nprob, idx, ts, nf, out, ys_null=True),
        "index = N": lambda: _raw_call(dual, gx, gy, N, K, M, A, nprob, bad_idx, ts, nf, out),
        "index < 0": lambda: _raw_call(dual, gx, gy, N, K, M, A, nprob, neg_idx, ts, nf, out),
        "test_size = N": lambda: _raw_call(dual, gx, gy, N, K, M, A, nprob, wide, N, 2, out),
    }
    for what, call in calls.items():
        assert call() == L.ERR_INVALID, what
        dual.synchronize()
        out.assert_untouched()
        for i in range(3):
            out.assert_prefilled(i)
    cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)
    L.check(L.lib().pls_hip_set_reducer(dual.h, cb, None, 0, 1), dual.h)
    try:
        rc = _raw_call(dual, gx, gy, N, K, M, A, nprob, idx, ts, nf, out)
    finally:
        dual.clear_reducer()
    assert rc == L.ERR_UNSUPPORTED
    dual.synchronize()
    out.assert_untouched()
    for i in range(3):
        out.assert_prefilled(i)


@pytest.mark.parametrize("route", ["sample-space", "per-problem"])
@pytest.mark.parametrize("name,layout", [("17x1003", "eigen"), ("97x1500", "aligned")])
def test_cvbatch_writes_exactly_its_outputs(name, layout, route):
    """8b: the call writes all of PRESS, ssy and E and nothing around them; X, Ys and the padding of ldy are untouched"""
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    Xh, Ysh, M, A, idx, nprob = case_data_b(name)
    N, K = Xh.shape
    nf, ts = idx.shape
    nobs = nf * ts
    gx, X = _place(Xh, torch.float64, layout)
    gy, Ys = _place(Ysh, torch.float64, layout)
    ins = Inputs(X=X, Ys=Ys, test_idx=idx)
    out = _outputs(M, A, nobs, nprob, layout)
    env = {"PLS_HIP_CVBATCH_REFIT": 1} if route == "per-problem" else {}
    with handle_with_env(**env) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        L.check(_raw_call(h, gx, gy, N, K, M, A, nprob, idx, ts, nf, out), h.h)
        h.synchronize()
    out.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    ref = case_reference_b(name)
    E = out[2].cpu().numpy().T.reshape(nprob, M, A, nobs).transpose(0, 1, 3, 2)
    _check(E, ref, f"{name} {layout} {route}")
    PRESS = out[0].cpu().numpy().T.reshape(nprob, A, M).transpose(0, 2, 1)
    assert press_err(PRESS, E) <= PRESS_TOL
    assert _rel_entries(out[1].cpu().numpy().T, ssy_of(Ysh, M, idx)) <= PRESS_TOL


def test_cvbatch_permutation_test_q2(dual):
    """9: Handle.permutation_test(cv=idx) on the nir example (60 x 401, z-scored, A = 3, 20 permutations, 6 folds)"""
    import pls_amd
    X, Y, _, _ = case_data("nir-loo")
    N, A, nperm = X.shape[0], 3, 20
    cv = np.random.default_rng(11).permutation(N).reshape(6, 10)
    Ys = np.asfortranarray(np.concatenate([Y[r] for r in np.vstack([np.arange(N)[None], _perms(N, nperm)])], axis=1))
    for where in ("device", "host"):
        Xi, Yi, Ysi = (_dev(X), _dev(Y), _dev(Ys)) if where == "device" else (X, Y, Ys)
        plain = dual.permutation_test(Xi, Yi, A, nperm, seed=5)
        t = dual.permutation_test(Xi, Yi, A, nperm, seed=5, cv=cv)
        assert not {"q2y", "q2y_perm", "p_q2"} & set(plain)
        assert np.array_equal(t["perms"], _perms(N, nperm))
        assert np.array_equal(t["r2y"], plain["r2y"]) and np.array_equal(t["r2y_perm"], plain["r2y_perm"])
        assert np.array_equal(t["p"], plain["p"])
        assert t["q2y"].shape == (1, A) and t["q2y_perm"].shape == (nperm, 1, A) and t["p_q2"].shape == (1, A)
        o = _np(dual.cv_press_batch(Xi, Ysi, 1, A, cv))
        q2 = 1.0 - o["PRESS"] / o["ssy"][:, :, None]
        assert np.array_equal(t["q2y"], q2[0]) and np.array_equal(t["q2y_perm"], q2[1:])
        assert np.array_equal(t["p_q2"], pls_amd.permutation_pvalues(q2[0], q2[1:]))
        print(f"nir {where}: q2y = {t['q2y'][0]}, largest permuted at A = {t['q2y_perm'][:, 0, A - 1].max():.3f}, p_q2 = {t['p_q2'][0]}")
        assert t["q2y"][0, A - 1] > t["q2y_perm"][:, 0, A - 1].max()
        assert t["p_q2"][0, A - 1] == 1.0 / (nperm + 1)
        small = dual.permutation_test(Xi, Yi, A, nperm, seed=5, cv=cv, max_bytes=7 * N * 8)  # chunks of 7 problems
        assert np.abs(small["q2y_perm"] - t["q2y_perm"]).max() <= 1e-12 and np.abs(small["q2y"] - t["q2y"]).max() <= 1e-12
    m = pls_amd.Model(_dev(X), _dev(Y), pls_amd.KERNEL_TYPE2, A, handle=dual)
    tm = m.permutation_test(nperm, seed=5, cv=cv)
    assert np.array_equal(tm["q2y"], t["q2y"]) or np.abs(tm["q2y"] - t["q2y"]).max() <= 1e-12
    assert np.array_equal(tm["p_q2"], t["p_q2"]) and "q2y" not in m.permutation_test(nperm, seed=5)


def _perms(N, nperm, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N) for _ in range(nperm)])
