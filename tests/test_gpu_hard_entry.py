"""The resampling, PRESS and missing-value entry points on hard data, against an 80-digit reference (tests/hard_data.py,
tests/golden/hard/e_*.npz), and every remaining entry point under exact power-of-two scaling.

tests/test_gpu_hard_data.py holds pls_hip_fit, pls_hip_fit_batch and pls_hip_cv_folds to max(FLOOR, 10 x err_form[form]) on six
hard input families; the entry points added since -- pls_hip_fit_resampled, pls_hip_cv_press_batch, pls_hip_fit_missing and its
companions -- had only met centred, unit-scale data and missing cells scattered uniformly.  Here they meet the same families,
the same rule, the same constants:

    err_hip <= max(FLOOR, 10 x err_form[form of the route])

err_form: what the plain-fp64 CPU restatement of the route's algebra achieves on the same inputs against the same reference,
measured when the fixture was made and pinned by tests/test_hard_data_ref.py (which also asserts the conditions that keep these
bounds meaningful).  The factor 10 is that file's one decimal digit for another summation order of the same algebra.

  route                        handle                                           form
  resample-dual                ALGO_DUAL                                        dual    (dual_resample)
  resample-refit               PLS_HIP_TINY=0, KERNEL plan                      kernel  (the oracle on the scaled rows)
  resample-refit-under-dual    ALGO_DUAL, created under PLS_HIP_RESAMPLE_REFIT  kernel
  press-dual                   ALGO_DUAL                                        dual    (dual_fit per fold)
  press-general                PLS_HIP_TINY=0, default plan                     type2   (the K-space fold route, as `cv`)
  missing                      the session's handle                             fit_missing_ref

Resampling: seven weight columns (six bootstrap draws with rows dropping out, one of fractional weights); B per replicate, B0,
Bmean, the Q columns, t^T t, and se = sqrt(max(Bm2, 0)) at max(2 FLOOR_B / rho, 10 x err_form_se).  PRESS: Y and Y with its rows
reversed at once; entrywise relative error with the floor the E floor implies for a sum of squares, 2 FLOOR_E |Y_held| /
sqrt(PRESS_ref); ssy to 1e-12; the same bits with and without E.  Missing values: cells missing at random, and a layout with a
whole tile missing, one column and one row with a single observed cell (hard_data.missing_mask), device and host memory; B per
component count and T per column at max(FLOOR, 10 err_form, 10 sens) -- sens: how far the fit moves with the stopping rule.

The second half: X 2^e, Y 2^f (and the weights 4^g) change nothing but exponents, so every output of every entry point must
come back bit-identical or scaled by an exact power of two (the table in test_power_of_two_scaling_is_exact_everywhere).

Every figure is printed before it is asserted; test_zz_write_entry_table prints the table of the run and, when
PLS_HARD_ENTRY_ACCURACY_FILE names a file, writes it there (the source of the second table in INTEGRATION.md section I).
"""
import functools
import os

import numpy as np
import pytest

import hard_data as hd
from conftest import handle_with_env
from test_dual_batch_ref import TOL_TT
from test_dual_ref import TOL_COL
from test_gpu_hard_data import FLOOR_B, FLOOR_B32, FLOOR_E, MARGIN, SCALE_CASES, SCALINGS, _dev, _np, handles  # noqa: F401

pytestmark = pytest.mark.gpu

A = hd.A
RATIOS = []      # (case, route, form, output, err_hip, err_form, err_hip / err_form, err_hip / bound)
SSY_TOL = 1e-12  # a plain sum of at most 60 squares: 60 eps in any order (PRESS_TOL of tests/test_dual_cvbatch_ref.py)
Z_TOL = 1e-12    # mean and sd of a column of 1e4 +- 1: a shifted one-sweep variance keeps twelve digits, an unshifted one two

RESAMPLE_ROUTES = {   # name -> (form, handle)
    "resample-dual": ("dual", "dual"),
    "resample-refit": ("kernel", "general"),
    "resample-refit-under-dual": ("kernel", "refit_dual"),
}
PRESS_ROUTES = {"press-dual": ("dual", "dual"), "press-general": ("type2", "general")}
RES_NAMES = ("Q", "tt", "B", "B0", "Bmean", "Bm2")
MEMORIES = ("device", "host")


@pytest.fixture(scope="module")
def H(handles):
    """the handles of tests/test_gpu_hard_data.py and refit_dual: ALGO_DUAL on a handle that keeps the general resampling route"""
    import pls_amd
    with handle_with_env(PLS_HIP_RESAMPLE_REFIT=1) as refit:
        refit.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        refit.set_option(pls_amd.OPT_PROFILE, 2)
        yield dict(handles, refit_dual=refit)


@functools.lru_cache(maxsize=None)
def _entry(case):
    from oracle import pls_oracle as po
    return hd.load_entry(po, *case)


def _es(f32):
    return 4 if f32 else 8


def _passes(lau):
    return lau["fused"] + lau["xb"] + lau["deflate"]


def _sample_space_only(t, N, K, f32, what):
    """one sweep over X and G is all the call booked: the sample-space route ran, not a fall-back"""
    lau = t["launches"]
    assert lau["xty"] == 1 and t["bytes"]["xty"] == N * K * _es(f32) + 8 * N * N and _passes(lau) == 0, (what, t)


def _record(case, route, form, output, err, ef, floor):
    """prints the figures, books the worst of them, returns the bound"""
    err, ef = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(ef, dtype=np.float64))
    bound = np.maximum(floor, MARGIN * ef) * np.ones_like(err)
    ef = ef * np.ones_like(err)
    c = int(np.argmax(err / bound))
    ratio = float(np.max(err / np.maximum(ef, 1e-16)))
    RATIOS.append((hd.case_name(*case), route, form, output, float(err.flat[c]), float(ef.flat[c]), ratio, float(err.flat[c] / bound.flat[c])))
    print(f"{hd.case_name(*case)} {route} [{form}] {output}: err_hip {err.reshape(-1)}  err_form {np.unique(ef)}  "
          f"err_hip/err_form {ratio:.3g}  err_hip/bound {err.flat[c] / bound.flat[c]:.3g}")
    return bound


# ---- resampling ------------------------------------------------------------------------------------------------------------------
def run_resample(H, route, X, Y, Wt, f32=False, want=RES_NAMES):
    import pls_amd
    h = H[RESAMPLE_ROUTES[route][1]]
    N, K = X.shape
    Xd, Yd, Wd = _dev(X, f32), _dev(Y, f32), _dev(Wt)
    if route == "resample-refit":
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
    if route == "resample-dual":
        h.timing()
        h.fit_resampled(Xd, Yd, A, Wd, want=("Q", "tt")); h.synchronize()
        _sample_space_only(h.timing(), N, K, f32, route)
    h.timing()
    out = h.fit_resampled(Xd, Yd, A, Wd, want=want); h.synchronize()
    lau = h.timing()["launches"]
    if route == "resample-dual":
        assert _passes(lau) == 0 and lau["xty"] >= 1, (route, lau)
    else:   # row-scaled refits under KERNEL, on either handle: per replicate passes over the scaled copy or a single-launch fit
        assert _passes(lau) + lau["small"] >= Wt.shape[1], (route, lau)
        if route == "resample-refit":
            assert _passes(lau) >= Wt.shape[1], (route, lau)
    return {k: _np(v) for k, v in out.items()}


def check_resample(H, case, route):
    family, N, K, M, f32 = case
    X, Y, Wt, fx, ex = _entry(case)
    form = RESAMPLE_ROUTES[route][0]
    got = run_resample(H, route, X, Y, Wt, f32)
    assert all(np.isfinite(v).all() for v in got.values()), route
    err = dict(zip(hd.RESAMPLE_FIGURES, hd.resample_errors(got, ex)))
    rho = float(ex["rho"])
    fb = FLOOR_B32 if f32 else FLOOR_B
    floors = dict(r=fb, se=2.0 * fb / rho, Bmean=fb, Q=FLOOR_B32 if f32 else TOL_COL, tt=FLOOR_B32 if f32 else TOL_TT)
    ok = {}
    for k in hd.RESAMPLE_FIGURES:
        bound = _record(case, route, form, "B_b" if k == "r" else k, err[k], float(ex[f"err_form_{k}_{form}"]), floors[k])
        ok[k] = bool((err[k] <= bound).all())
    e0 = hd.rel_fro(got["B0"], fx["B_ref"][A - 1])
    ok["B0"] = bool(e0 <= _record(case, route, form, "B0", e0, fx["err_form_" + form][A - 1], fb)[0])
    assert all(ok.values()), (route, ok, err)
    # a replicate of unit weights is the fit of (X, Y) itself, bit for bit
    one = run_resample(H, route, X, Y, np.concatenate([Wt, np.ones((N, 1))], axis=1), f32, want=("B", "B0"))
    assert np.array_equal(one["B"][hd.NREP], one["B0"]), route
    assert np.array_equal(one["B0"], got["B0"]) and np.array_equal(one["B"][:hd.NREP], got["B"]), route


# ---- PRESS -----------------------------------------------------------------------------------------------------------------------
def run_press(H, route, X, Y, f32=False):
    """cv_press_batch on [Y | Y with its rows reversed] over the three contiguous folds: dict(PRESS, ssy, E), and the same
    call without E"""
    import pls_amd
    h = H[PRESS_ROUTES[route][1]]
    N, K = X.shape
    M = Y.shape[1]
    if route == "press-general":
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
    Xd, Yd = _dev(X, f32), _dev(np.concatenate([Y, hd.second_responses(Y)], axis=1), f32)
    idx = hd.fold_indices(N)
    h.timing()
    lean = h.cv_press_batch(Xd, Yd, M, A, idx, want=("PRESS", "ssy")); h.synchronize()
    t = h.timing()
    if route == "press-dual":
        _sample_space_only(t, N, K, f32, route)
    else:
        assert _passes(t["launches"]) == 0 and t["launches"]["xty"] >= 1 and t["launches"]["small"] >= 1, (route, t)
    full = h.cv_press_batch(Xd, Yd, M, A, idx, want=("PRESS", "ssy", "E")); h.synchronize()
    return {k: _np(v) for k, v in full.items()}, {k: _np(v) for k, v in lean.items()}


def check_press(H, case, route):
    family, N, K, M, f32 = case
    X, Y, Wt, fx, ex = _entry(case)
    form = PRESS_ROUTES[route][0]
    full, lean = run_press(H, route, X, Y, f32)
    assert full["PRESS"].shape == (2, M, A) and full["ssy"].shape == (2, M) and full["E"].shape == (2, M, 3 * hd.TS[N], A)
    assert all(np.isfinite(v).all() for v in full.values()), route
    held = hd.fold_indices(N).reshape(-1)
    ynorm = np.stack([np.linalg.norm(Yp[held], axis=0) for Yp in (Y, hd.second_responses(Y))])          # (2, M)
    fe = FLOOR_B32 if f32 else FLOOR_E
    floor = 2.0 * fe * ynorm[:, :, None] / np.sqrt(ex["PRESS_ref"])
    err = np.abs(full["PRESS"] - ex["PRESS_ref"]) / ex["PRESS_ref"]
    bound = _record(case, route, form, "PRESS", err, float(ex["err_form_P_" + form]), floor)
    ee = np.linalg.norm(full["E"][0] - fx["E_ref"]) / np.linalg.norm(Y[held])
    be = _record(case, route, form, "E", ee, float(fx["err_form_E_" + form]), fe)
    es = np.abs(full["ssy"] - ex["ssy_ref"]) / ex["ssy_ref"]
    print(f"{hd.case_name(*case)} {route}: ssy relative error {es.max():.2e}")
    assert (err <= bound).all() and ee <= be[0], (route, err, bound, ee, be)
    assert (es <= SSY_TOL).all(), (route, es)
    assert np.array_equal(full["PRESS"], lean["PRESS"]) and np.array_equal(full["ssy"], lean["ssy"]), route


# ---- missing values --------------------------------------------------------------------------------------------------------------
def _same_bits(t, a):
    """a device (or host) matrix still holds the bits of the numpy image it was made from, NaN included"""
    return np.array_equal(np.ascontiguousarray(_np_raw(t)).view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


def _np_raw(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _place(a, f32, mem):
    if mem == "device":
        return _dev(a, f32)
    return np.asfortranarray(a.astype(np.float32 if f32 else np.float64))


def run_missing(H, Xn, Y, f32=False, mem="device"):
    """dict(W, P, Q, R, T, B, iters) of fit_missing, the scores of the training rows from scores_missing, and whether X kept its bits"""
    h = H["default"]
    Xi, Yi = _place(Xn, f32, mem), _place(Y, f32, mem)
    image = _np_raw(Xi).copy()
    out = h.fit_missing(Xi, Yi, A)
    S = h.scores_missing(Xi, out["W"], out["P"])
    h.synchronize()
    got = {k: (_np_raw(v) if k == "iters" else _np(v)) for k, v in out.items()}
    return got, _np(S), _same_bits(Xi, image)


def _align(T, Tref):
    s = np.sign(np.einsum("na,na->a", T, Tref)); s[s == 0] = 1.0
    return T * s[None, :]


def check_missing(H, case, pat, mem):
    family, N, K, M, f32 = case
    X, Y, Wt, fx, ex = _entry(case)
    mask = hd.missing_mask(N, K, pat)
    got, S, kept = run_missing(H, hd.with_missing(X, mask), Y, f32, mem)
    route = f"missing-{pat}-{mem}"
    print(f"{hd.case_name(*case)} {route}: iters {got['iters']} / reference {ex['iters_ref_' + pat]}")
    for k in ("W", "P", "Q", "R", "T", "B"):   # the missing tile, the single-cell row and column: no 0 / 0 anywhere
        assert np.isfinite(got[k]).all(), (route, k)
    assert np.isfinite(S).all() and kept, route
    Tref = ex["Tm_ref_" + pat]
    got["T"] = _align(got["T"], Tref)
    eb, et = hd.missing_errors(got, ex, pat)
    eb[A - 1] = max(eb[A - 1], hd.rel_fro(got["B"], ex["Bm_ref_" + pat][A - 1]))
    es = np.array([hd.rel_fro(_align(S, Tref)[:, c], Tref[:, c]) for c in range(A)])
    sens = float(ex["sens_m_" + pat])
    fb, fc = (FLOOR_B32, FLOOR_B32) if f32 else (FLOOR_B, TOL_COL)
    bb = _record(case, route, "nipals-missing", "B", eb, ex["err_form_m_" + pat], max(fb, MARGIN * sens))
    bt = _record(case, route, "nipals-missing", "T", et, ex["err_form_mT_" + pat], max(fc, MARGIN * sens))
    bs = _record(case, route, "nipals-missing", "scores", es, ex["err_form_mT_" + pat], max(fc, MARGIN * sens))
    assert (eb <= bb).all() and (et <= bt).all() and (es <= bs).all(), (route, eb, bb, et, bt, es, bs)
    if M == 1:
        assert (got["iters"] == 1).all(), got["iters"]
    else:
        assert (np.abs(got["iters"] - ex["iters_ref_" + pat]) <= 1).all(), (got["iters"], ex["iters_ref_" + pat])


def check_z_scores(H, case, pat, mem):
    family, N, K, M, f32 = case
    X, Y, Wt, fx, ex = _entry(case)
    mask = hd.missing_mask(N, K, pat)
    Xi = _place(hd.with_missing(X, mask), f32, mem)
    image = _np_raw(Xi).copy()
    Z, mean, sd, nobs = (_np_raw(v) for v in H["default"].z_scores_missing(Xi))
    H["default"].synchronize()
    assert _same_bits(Xi, image)
    assert np.array_equal(nobs, ex["znobs_" + pat])
    assert np.array_equal(np.isnan(Z), mask | (nobs < 2)[None, :])      # NaN kept where a cell is missing; a single-cell column NaN throughout
    two = nobs >= 2
    em = np.abs(mean[two] - ex["zmean_ref_" + pat][two]) / np.abs(ex["zmean_ref_" + pat][two])
    esd = np.abs(sd[two] - ex["zsd_ref_" + pat][two]) / ex["zsd_ref_" + pat][two]
    print(f"{hd.case_name(*case)} z-scores-{pat}-{mem}: mean {em.max():.2e}  sd {esd.max():.2e}")
    if family.startswith("offset"):
        assert em.max() <= Z_TOL and esd.max() <= Z_TOL, (em.max(), esd.max())


FP64_CASES = [c for c in hd.all_cases() if not c[4]]
MISSING_CASES = [c for c in FP64_CASES if hd.has_missing_reference(*c[:4])]
F32_CASE = hd.F32_CASE + (True,)
_ids = lambda c: hd.case_name(*c)


@pytest.mark.parametrize("route", list(RESAMPLE_ROUTES))
@pytest.mark.parametrize("case", FP64_CASES, ids=_ids)
def test_resampling_on_hard_data(H, case, route):
    check_resample(H, case, route)


@pytest.mark.parametrize("route", list(PRESS_ROUTES))
@pytest.mark.parametrize("case", FP64_CASES, ids=_ids)
def test_press_on_hard_data(H, case, route):
    check_press(H, case, route)


@pytest.mark.parametrize("mem", MEMORIES)
@pytest.mark.parametrize("pat", hd.MISSING_PATTERNS)
@pytest.mark.parametrize("case", MISSING_CASES, ids=_ids)
def test_missing_values_on_hard_data(H, case, pat, mem):
    check_missing(H, case, pat, mem)


@pytest.mark.parametrize("mem", MEMORIES)
@pytest.mark.parametrize("pat", hd.MISSING_PATTERNS)
@pytest.mark.parametrize("case", [c for c in FP64_CASES if c[3] == 1], ids=_ids)
def test_column_statistics_with_missing_values_on_hard_data(H, case, pat, mem):
    check_z_scores(H, case, pat, mem)


@pytest.mark.parametrize("what", ["resample-dual", "press-dual", "missing-mcar", "missing-blocks", "z-scores"])
def test_entry_points_on_hard_data_fp32_storage(H, what):
    """`offset` with offsets fp32 holds exactly, inputs rounded once to fp32; the reference is that of the rounded inputs"""
    if what == "resample-dual":
        check_resample(H, F32_CASE, what)
    elif what == "press-dual":
        check_press(H, F32_CASE, what)
    elif what == "z-scores":
        for pat in hd.MISSING_PATTERNS:
            check_z_scores(H, F32_CASE, pat, "device")
    else:
        for mem in MEMORIES:
            check_missing(H, F32_CASE, what.split("-")[1], mem)


# ---- power-of-two scaling, bit for bit -------------------------------------------------------------------------------------------
WEIGHT_EXP = 3   # the weights by 4^g: s = sqrt(w) by 2^g


def _fit_model(H, X, Y, f32):
    """R, P, Q (device, fp64) and T of the KERNEL plan: the model the diagnostics and SSE calls are given"""
    import pls_amd
    h = H["general"]
    h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
    out = h.fit_device(_dev(X, f32), _dev(Y, f32), A)
    h.synchronize()
    return out


def _model_sse(h, Xd, Yd, R, Q, f32):
    import pls_amd
    import torch
    from pls_amd import _lib as L
    N, K = Xd.shape
    M = Yd.shape[1]
    Rc = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K).copy_(R)
    Qc = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M).copy_(Q)
    out = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M)
    L.check(L.lib().pls_hip_model_sse(h.h, Xd.data_ptr(), int(Xd.stride(1)), Yd.data_ptr(), int(Yd.stride(1)), N, K, M, A,
                                      Rc.data_ptr(), Qc.data_ptr(), L.F32 if f32 else L.F64, L.MEM_DEVICE, out.data_ptr()), h.h)
    h.synchronize()
    return out


def _all_calls(H, X, Y, Wt, f32, model, E0, e, f, g):
    """(route, output) -> (array, exponent of two it carries under X 2^e, Y 2^f, Wt 4^g) for every call of the table, on the
    scaled inputs.  model: R, P, Q of the UNSCALED fit (R and P are invariant, Q carries f - e: an exact rescaling);
    E0: the unscaled residuals of problem 0."""
    import pls_amd
    import torch
    out = {}
    N, K = X.shape
    M = Y.shape[1]
    Xs, Ys, Ws = np.ldexp(X, e), np.ldexp(Y, f), np.ldexp(Wt, 2 * g)
    sc = dict(Q=f - e, B=f - e, B0=f - e, Bmean=f - e, Bm2=2 * (f - e), tt=2 * (e + g))
    for route in ("resample-dual", "resample-refit"):
        got = run_resample(H, route, Xs, Ys, Ws, f32)
        out.update({(route, k): (got[k], sc[k]) for k in sc})
    for route in PRESS_ROUTES:
        got, _ = run_press(H, route, Xs, Ys, f32)
        out.update({(route, k): (got[k], n) for k, n in (("PRESS", 2 * f), ("ssy", 2 * f), ("E", f))})
    h = H["default"]
    for pat in hd.MISSING_PATTERNS:
        Xn = hd.with_missing(Xs, hd.missing_mask(N, K, pat))
        got, S, _ = run_missing(H, Xn, Ys, f32)
        sm = dict(W=0, P=0, R=0, iters=0, T=e, Q=f - e, B=f - e)
        out.update({("missing-" + pat, k): (got[k], sm[k]) for k in sm})
        out[("scores-missing-" + pat, "S")] = (S, e)
        Z, mean, sd, nobs = (_np_raw(v) for v in h.z_scores_missing(_dev(Xn, f32)))
        out.update({("z-scores-missing-" + pat, k): v for k, v in (("Z", (Z, 0)), ("nobs", (nobs, 0)), ("mean", (mean, e)), ("sd", (sd, e)))})
    Xd, Yd = _dev(Xs, f32), _dev(Ys, f32)
    Z, mean, sd = (_np_raw(v) for v in h.colwise_z_scores(Xd))
    out.update({("z-scores", k): v for k, v in (("Z", (Z, 0)), ("mean", (mean, e)), ("sd", (sd, e)))})
    R, P = model["R"], model["P"]
    Qs = torch.from_numpy(np.ldexp(model["Q"].cpu().numpy(), f - e)).cuda()     # (numpy's ldexp is exact; a pow on the device need not be)
    every = ("Q", "T2", "S", "ssx", "sst")
    d0 = h.x_diagnostics(Xd, R, P, want=every)
    tvar = torch.from_numpy(np.ldexp(model["tvar"].cpu().numpy(), 2 * e)).cuda()
    d1 = h.x_diagnostics(Xd, R, P, tvar=tvar, want=every)
    sx = dict(Q=2 * e, T2=0, S=e, ssx=2 * e, sst=2 * e)
    for route, d in (("x-diagnostics", d0), ("x-diagnostics-tvar", d1)):
        out.update({(route, k): (_np_raw(d[k]), sx[k]) for k in every})
    out[("sse-by-components", "SSE")] = (_np_raw(h.sse_by_components(d0["S"], Yd, Qs)), 2 * f)
    out[("model-sse", "SSE")] = (_np_raw(_model_sse(h, Xd, Yd, R, Qs, f32)), 2 * f)
    Ed = torch.from_numpy(np.ldexp(E0, f)).cuda()
    default = h.get_option(pls_amd.OPT_VALIDATION_LDS_ROWS)
    try:
        for route, rows in (("validation-lds", default), ("validation-stream", 0)):
            h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, rows)
            press, D, probw, ref = (_np_raw(v) for v in h.validation(Ed))
            out.update({(route, k): v for k, v in (("PRESS", (press, 2 * f)), ("D", (D, 0)), ("probw", (probw, 0)), ("ref", (ref, 0)))})
    finally:
        h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, default)
    h.synchronize()
    return out


def _in_range(key, a, N, f32):
    """What of an output the law covers.  One exception, fp32 storage only: W, P, R of the `blocks` column with a single
    observed cell.  Its loading is p = x / t, so the deflated cell x - t p is zero in exact arithmetic and rounding noise at
    1e-16 |x| in fp64, squared again by every later component; the fp32 work copy holds 1e-32 |x| and then 1e-48 |x|, which
    is below the smallest fp32 subnormal at one scale of X and representable at 2^40 times that scale.  From the third
    component on that column's W and P are quotients of this noise: the format's range, not a threshold of the algorithm.
    With fp64 storage the same entries obey the law bit for bit."""
    if f32 and key[0] == "missing-blocks" and key[1] in ("W", "P", "R"):
        return np.delete(a, hd.BLOCKS[N][2][0], axis=0)
    return a


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", SCALE_CASES, ids=lambda c: hd.case_name(*c))
def test_power_of_two_scaling_is_exact_everywhere(H, case, dt):
    """X 2^e, Y 2^f for (e, f) = (+40, -9), (-40, +13), the resampling weights by 4^g, g = 3:

      fit_resampled, both routes      Q 2^(f-e); B, B0, Bmean 2^(f-e); Bm2 2^(2(f-e)); tt 2^(2(e+g));
                                      the weights alone: Q, B, B0, Bmean, Bm2 bit-identical
      cv_press_batch, both routes     PRESS, ssy 2^(2f); E 2^f
      fit_missing, both patterns      W, P, R, iters bit-identical; T 2^e; Q, B 2^(f-e)
      scores_missing                  S 2^e
      z_scores_missing, z_scores      Z, nobs bit-identical; mean, sd 2^e
      x_diagnostics, tvar NULL/given  T2 bit-identical; Qres, ssx, sst 2^(2e); S 2^e          (tvar given: tvar 2^(2e))
      sse_by_components, model_sse    SSE 2^(2f), with the scaled model
      validation, LDS and streaming   ref, D, probw bit-identical; PRESS 2^(2f)              (on E 2^f)

    +-40 keeps every square and every fp32 score normal on these data.  tests/test_hard_data_ref.py shows the CPU restatements
    obey the same table bit for bit: it is a property of the algebra."""
    import torch
    f32 = dt == "f32"
    from oracle import pls_oracle as po
    X, Y = hd.hard_inputs(po, *case)
    if f32:
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    N = X.shape[0]
    Wt = hd.resample_weights(N)
    fit = _fit_model(H, X, Y, f32)
    T = fit["T"].to(torch.float64)
    model = dict(R=fit["R"], P=fit["P"], Q=fit["Q"], tvar=(T * T).sum(0) / (N - 1))
    E0 = run_press(H, "press-dual", X, Y, f32)[0]["E"][0]
    base = _all_calls(H, X, Y, Wt, f32, model, E0, 0, 0, 0)
    broken = []
    for e, f, g in [(0, 0, WEIGHT_EXP)] + [(e, f, WEIGHT_EXP) for e, f in SCALINGS]:
        got = _all_calls(H, X, Y, Wt, f32, model, E0, e, f, g)
        for key, (a0, _) in base.items():
            have, n = got[key]
            want = np.ldexp(a0.astype(np.float64), n) if a0.dtype.kind == "f" else a0
            have = have.astype(np.float64) if have.dtype.kind == "f" else have
            want, have = _in_range(key, want, N, f32), _in_range(key, have, N, f32)
            if not np.array_equal(want, have, equal_nan=(a0.dtype.kind == "f")):
                with np.errstate(all="ignore"):
                    rel = float(np.nanmax(np.abs(want - have)) / max(float(np.nanmax(np.abs(want))), 1e-300))
                where = np.unique(np.argwhere(~((want == have) | (np.isnan(want) & np.isnan(have))))[:, 0])[:6].tolist() if want.ndim else []
                broken.append((key[0], (e, f, g), key[1], f"{rel:.2e}", where))
    print(hd.case_name(*case + (False,)), dt, "broken:", broken)
    assert not broken, broken


def test_zz_write_entry_table():
    """the figures of this run: per (case, route, output) the device's worst error, the CPU figure of its form there, the worst
    ratio of the two, and the share of the bound used"""
    if not RATIOS:   # (run on its own: nothing to tabulate)
        return
    lines = [f"{'case':28s} {'route':26s} {'form':14s} {'output':7s} {'err_hip':>9s} {'err_form':>9s} {'hip/form':>9s} {'hip/bound':>9s}"]
    for name, route, form, output, eh, ef, ratio, used in RATIOS:
        lines.append(f"{name:28s} {route:26s} {form:14s} {output:7s} {eh:9.2e} {ef:9.2e} {ratio:9.3g} {used:9.3g}")
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("PLS_HARD_ENTRY_ACCURACY_FILE")
    if out:
        with open(out, "w") as fh:
            fh.write(text)
