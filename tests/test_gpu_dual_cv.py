"""Cross-validation folds under the sample-space plan (pls_hip_cv_folds with PLS_HIP_ALGO_DUAL, pls_amd/csrc/plan_dual_cv.hpp)
on the GPU: every fold from one G = X X^T, one sweep over X whatever A and the number of folds are.  Cases, reference (one
oracle refit per fold) and bar are those of tests/test_dual_cv_ref.py."""
import ctypes

import numpy as np
import pytest

from conftest import handle_with_env
from test_dual_cv_ref import BAR, CASES, case_data, case_reference, fold_indices, rel_err
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
    """(X, Y) on the device in the case's storage type, their host images in that type, A, idx"""
    X, Y, A, idx = case_data(name)
    dt = CASES[name][6]
    npdt = np.float32 if dt == "f32" else np.float64
    return _dev(X, dt), _dev(Y, dt), np.asfortranarray(X.astype(npdt)), np.asfortranarray(Y.astype(npdt)), A, idx


def _check(E, ref, what):
    err = rel_err(E, ref)
    print(f"{what}: max|E - ref| / max(max|ref|, 1) = {err:.2e}")
    assert err < BAR, what


@pytest.mark.parametrize("name", list(CASES))
def test_dual_cv_parity(dual, name):
    """1: device call and host-memory call against one oracle refit per fold; the host call within 1e-12 of the device call"""
    X, Y, Xh, Yh, A, idx = _case(name)
    ref = case_reference(name)
    E = dual.cv_folds(X, Y, A, idx).cpu().numpy()
    Eh = dual.cv_folds(Xh, Yh, A, idx)
    _check(E, ref, name + " device")
    _check(Eh, ref, name + " host")
    assert np.abs(Eh - E).max() < 1e-12 * max(np.abs(ref).max(), 1.0)


@pytest.mark.parametrize("name", ["97x1500", "130-columns"])
@pytest.mark.parametrize("cap", [5, 1])
def test_dual_cv_rounds(name, cap):
    """2: several rounds (a ragged last one; one fold per round) against the same reference"""
    import pls_amd
    X, Y, _, _, A, idx = _case(name)
    with handle_with_env(PLS_HIP_DUALCV_ROUND=cap) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        E = h.cv_folds(X, Y, A, idx).cpu().numpy()
    _check(E, case_reference(name), f"{name} rounds of {cap}")


def _profiled_folds(h, X, Y, A, N, nf):
    rng = np.random.default_rng(nf)
    idx = np.stack([rng.permutation(N)[:5] for _ in range(nf)])
    h.timing()
    h.cv_folds(X, Y, A, idx)
    return h.timing()


def test_dual_cv_one_sweep_over_x():
    """3: the route is taken and books one sweep over X and G, for 4 folds as for 12 (the refit route books a fit per fold)"""
    import pls_amd
    N, K, A = 60, 20000, 4
    with handle_with_env() as h:
        X = h.synth_x(0, N, K, 5); Y = h.synth_y(0, N, 1, 5)
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        for nf in (4, 12):
            t = _profiled_folds(h, X, Y, A, N, nf)
            assert t["bytes"]["xty"] == N * K * 8 + N * N * 8, (nf, t)
            assert t["launches"]["xty"] == 1, (nf, t)
            assert t["launches"]["xb"] == 0 and t["launches"]["deflate"] == 0 and t["launches"]["fused"] == 0, (nf, t)
        h.set_option(pls_amd.OPT_PROFILE, 0)


def test_dual_cv_masking():
    """4: the held-out rows of Y never reach a fold's model.  The route forms E = Y_te - pred with ONE rounding, pred being the
    running prediction of the held-out rows, so pred is read off exactly where Y_te = 0 (E = -pred).  With the held-out rows
    replaced by zeros, and by other finite values, E must be fl(Y_te - pred) bit for bit: the predictions are bit-equal between
    the calls.  (fl(Y_te - E) itself is no such observable: it rounds twice, differently for different Y_te.)"""
    import pls_amd
    torch = _torch()
    name = "97x1500"
    N, K, M, A, ts, nf, _ = CASES[name]
    X, Y, _, _, A, idx = _case(name)
    idx = idx[:1]
    te = torch.from_numpy(idx[0]).cuda()
    rng = np.random.default_rng(3)
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        Y0 = Y.clone(); Y0[te] = 0.0
        Y2 = Y.clone(); Y2[te] = torch.from_numpy(1.0e3 * rng.standard_normal((ts, M))).cuda()
        E1 = h.cv_folds(X, Y, A, idx).cpu().numpy()
        pred = -h.cv_folds(X, Y0, A, idx).cpu().numpy()  # (M, ts, A), exact
        E2 = h.cv_folds(X, Y2, A, idx).cpu().numpy()
    assert np.isfinite(pred).all() and np.abs(pred).max() > 0
    for Yv, E in ((Y, E1), (Y2, E2)):
        yte = Yv[te].cpu().numpy().T[:, :, None]  # (M, ts, 1)
        assert np.array_equal(E, yte - pred)
    _check(E1, case_reference(name)[:, :ts], name + " one fold")


@pytest.mark.parametrize("name", ["17x1003", "513x4100"])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
def test_dual_cv_writes_exactly_e(name, layout):
    """5: E is written and nothing around it; X and Y are untouched"""
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    N, K, M, A, ts, nf, _ = CASES[name]
    Xh, Yh, A, idx = case_data(name)
    nobs = nf * ts
    gx, X = _place(Xh, torch.float64, layout)
    gy, Y = _place(Yh, torch.float64, layout)
    ins = Inputs(X=X, Y=Y, test_idx=idx)
    ge = Guarded([(nobs, M * A, nobs)], torch.float64, layout)
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        rc = L.lib().pls_hip_cv_folds(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A,
                                      idx.ctypes.data_as(ctypes.c_void_p), ts, nf, L.F64, L.MEM_DEVICE, ge.ptr(0))
        L.check(rc, h.h)
        h.synchronize()
    ge.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    ref = case_reference(name)
    want = ref.transpose(1, 0, 2).reshape(nobs, M * A)  # E[m (nobs A) + i + c nobs] = column m A + c, row i
    assert np.abs(ge[0].cpu().numpy() - want).max() < BAR * max(np.abs(ref).max(), 1.0)


def test_dual_cv_is_deterministic(dual):
    """6: the same bits twice on one handle and once on a fresh one"""
    import pls_amd
    torch = _torch()
    X, Y, _, _, A, idx = _case("513x4100")
    first = dual.cv_folds(X, Y, A, idx).clone()
    again = dual.cv_folds(X, Y, A, idx)
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        fresh = h.cv_folds(X, Y, A, idx)
    assert torch.equal(first, again)
    assert torch.equal(first, fresh)


def test_dual_cv_refit_switch_is_the_cross_check(dual):
    """7a: PLS_HIP_CV_REFIT=1 under ALGO_DUAL takes the refit route; the two agree within the bar"""
    import pls_amd
    name = "97x1500"
    X, Y, _, _, A, idx = _case(name)
    E = dual.cv_folds(X, Y, A, idx).cpu().numpy()
    with handle_with_env(PLS_HIP_CV_REFIT=1) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        Er = h.cv_folds(X, Y, A, idx).cpu().numpy()
    _check(Er, case_reference(name), name + " refit under ALGO_DUAL")
    assert np.abs(Er - E).max() < BAR * max(np.abs(E).max(), 1.0)


def test_dual_cv_declined_calls_route_as_before(oracle):
    """7b: M = 33, and a handle with a one-rank reducer, under ALGO_DUAL: PLS_HIP_OK from the existing routes, at the bar"""
    import pls_amd
    from pls_amd import _lib as L
    from test_dual_cv_ref import fold_reference
    N, K, A, ts, nf = 50, 60, 2, 5, 4
    idx = fold_indices(N, ts, nf)
    X = oracle.synth_x(0, N, K)
    Y33, Y2 = oracle.synth_y(0, N, 33), oracle.synth_y(0, N, 2)
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        E = h.cv_folds(_dev(X), _dev(Y33), A, idx).cpu().numpy()
        _check(E, fold_reference(X, Y33, A, idx), "M = 33")
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        E = h.cv_folds(_dev(X), _dev(Y2), A, idx).cpu().numpy()
        h.clear_reducer()
        _check(E, fold_reference(X, Y2, A, idx), "one-rank reducer")


def test_dual_cv_other_plans_route_as_before():
    """7c: under ALGO_KERNEL the profile of test 3 does not show the one-sweep figure"""
    import pls_amd
    N, K, A = 60, 20000, 4
    with handle_with_env() as h:
        X = h.synth_x(0, N, K, 5); Y = h.synth_y(0, N, 1, 5)
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        t = _profiled_folds(h, X, Y, A, N, 4)
        h.set_option(pls_amd.OPT_PROFILE, 0)
    assert not (t["bytes"]["xty"] == N * K * 8 + N * N * 8 and t["launches"]["xty"] == 1), t


def test_dual_cv_one_member_group():
    """8: pls_hip_group_cv_folds on a one-member group reaches the route through the member's handle"""
    import pls_amd
    name = "nir-loo"
    Xh, Yh, A, idx = case_data(name)
    g = pls_amd.Group([0])
    try:
        g.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        E = g.cv_folds(g.upload(Xh), g.upload(Yh), A, idx)
        g.set_option(pls_amd.OPT_ALGO, 0)
    finally:
        g.close()
    _check(np.asarray(E), case_reference(name), "one-member group")


def test_dual_cv_end_to_end_validation(handle):
    """9: nir leave-one-out: the PRESS minimum and the component choice at alpha = 0.1 from the new route's E are those from
    the E of the default plan"""
    import pls_amd
    from pls_amd.model import pick_components
    X, Y, _, _, A, idx = _case("nir-loo")
    handle.set_option(pls_amd.OPT_ALGO, 0)
    base = handle.validation(handle.cv_folds(X, Y, A, idx))
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    try:
        got = handle.validation(handle.cv_folds(X, Y, A, idx))
    finally:
        handle.set_option(pls_amd.OPT_ALGO, 0)
    ref0, ref1 = base[3].cpu().numpy(), got[3].cpu().numpy()
    assert np.array_equal(ref0, ref1)
    assert np.array_equal(pick_components(base[2].cpu().numpy(), ref0, 0.1), pick_components(got[2].cpu().numpy(), ref1, 0.1))
