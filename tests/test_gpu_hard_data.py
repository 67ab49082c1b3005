"""Every fit route of the library on hard data, against an 80-digit reference (tests/hard_data.py, tests/golden/hard/h_*.npz).

The rest of the suite draws its inputs from the seeded generator or the z-scored examples: zero-mean, unit-scale data on
which the forms that work from X^T X or X X^T lose nothing.  Here the same routes meet uncentred, graded, nearly
rank-deficient and spectra-like inputs.  For every component count c a route exposes

    rel_fro(B_hip[c], B_ref[c]) <= max(FLOOR, 10 x err_form[form][c])

FLOOR: the bar the suite holds the route to on benign data (1e-10 for B in fp64, 2e-5 with fp32 storage; 1e-8 for the
cross-validation residuals, in units of the norm of the held-out responses).  err_form: what the plain-fp64 CPU restatement
of the algebra the route implements achieves on the same inputs, measured against the same reference when the fixture was
made and pinned by tests/test_hard_data_ref.py.  The factor 10 is one decimal digit for another (blocked) summation order of
the same algebra: a margin over a CPU measurement, not a measured device figure.  A route that needs more loses digits its
algebra does not.

Routes -> forms, as include/pls_hip.h describes them:
  kernel   KERNEL fused / unfused, AUTO where its cost model picks KERNEL, the single-launch fits (one workgroup; resident)
  nipals   NIPALS
  type2    GRAM, KERNEL_TYPE2, the resident X^T X launch AUTO picks for mid-size data, the host-memory entry under GRAM (X^T X
           accumulated during the upload), fit_batch and cv_folds on their K-space routes
  dual     every route under ALGO_DUAL: fit, fit_batch, cv_folds
Which kernels ran is checked through the launch counters, as test_auto_plan_choice and the resident tests do.

The second half: scaling X by 2^e and Y by 2^f is exact in binary floating point, and nothing in the algorithm has an
absolute scale, so W, P, R must come out bit-identical and T, Q, B scaled by exact powers of two -- on every route, in both
storage types.  A route that breaks this hides an absolute threshold or reads something it did not compute.

Every figure is printed before it is asserted; test_zz_write_ratio_table prints the table of the run and, when
PLS_HARD_ACCURACY_FILE names a file, writes it there (the source of the table in INTEGRATION.md section I).
"""
import functools
import os

import numpy as np
import pytest

import hard_data as hd
from conftest import handle_with_env

pytestmark = pytest.mark.gpu

A = hd.A
FLOOR_B, FLOOR_B32, FLOOR_E = 1e-10, 2e-5, 1e-8
MARGIN = 10.0
RATIOS = []      # (case, route, form, worst err_hip, err_form there, worst err_hip / err_form, worst err_hip / bound)

FIT_ROUTES = {   # name -> (form, handle, algo, fuse, method, memory)
    "kernel-fused": ("kernel", "general", "KERNEL", 1, 1, "device"),
    "kernel-unfused": ("kernel", "general", "KERNEL", 0, 1, "device"),
    "nipals": ("nipals", "general", "NIPALS", 1, 1, "device"),
    "gram": ("type2", "general", "GRAM", 1, 1, "device"),
    "auto": ("kernel", "general", "AUTO", 1, 1, "device"),           # below 4096 rows the cost model picks KERNEL
    "type2": ("type2", "general", "KERNEL", 1, 2, "device"),
    "single-launch": ("kernel", "default", "KERNEL", 1, 1, "device"),
    "single-launch-auto": (None, "default", "AUTO", 1, 1, "device"),  # tall: the resident X^T X launch; wide: one workgroup, kernel form
    "dual": ("dual", "dual", "DUAL", 1, 1, "device"),
    "host-gram": ("type2", "default", "GRAM", 1, 1, "host"),
}
OTHER_ROUTES = {"batch": "type2", "batch-dual": "dual", "cv": "type2", "cv-dual": "dual"}
ALL_ROUTES = list(FIT_ROUTES) + list(OTHER_ROUTES)
F32_ROUTES = ("kernel-fused", "gram", "dual")


def _torch():
    import torch
    return torch


def _form(route, N):
    if route == "single-launch-auto":
        return "type2" if N > 1024 else "kernel"
    return FIT_ROUTES[route][0] if route in FIT_ROUTES else OTHER_ROUTES[route]


@pytest.fixture(scope="module")
def handles(handle):
    """default: the session's handle; general: no single-launch fits (PLS_HIP_TINY=0: the general plans on every shape);
    dual: ALGO_DUAL"""
    import pls_amd
    with handle_with_env(PLS_HIP_TINY=0) as general, handle_with_env() as dual:
        dual.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        for h in (handle, general, dual):
            h.set_option(pls_amd.OPT_PROFILE, 2)
        try:
            yield {"default": handle, "general": general, "dual": dual}
        finally:
            handle.set_option(pls_amd.OPT_PROFILE, 0)


@functools.lru_cache(maxsize=None)
def _case(case):
    from oracle import pls_oracle as po
    return hd.load_case(po, *case)


def _dev(a, f32=False):
    """a column-major device copy with 16-byte aligned columns"""
    import pls_amd
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a))
    dt = torch.float32 if f32 else torch.float64
    out = pls_amd.colmajor_empty(a.shape[0], a.shape[1], dt, "cuda")
    out.copy_(t.to(dt))
    return out


def _np(t):
    return t.cpu().numpy().astype(np.float64) if hasattr(t, "cpu") else np.asarray(t, dtype=np.float64)


def _launch_check(route, lau, N, K, by):
    """the intended kernel family ran"""
    total = sum(lau.values())
    passes = lau["fused"] + lau["xb"] + lau["deflate"]
    if route in ("single-launch", "single-launch-auto"):
        assert total == 1 and lau["small"] == 1, (route, lau)
    elif route == "kernel-fused" or route == "auto":
        assert total > 1 and lau["fused"] + lau["xb"] >= A and lau["deflate"] == 0, (route, lau)
    elif route == "kernel-unfused":
        assert lau["fused"] == 0 and lau["xb"] >= A and lau["deflate"] == 0, (route, lau)
    elif route == "nipals":
        assert total > 1 and lau["fused"] + lau["deflate"] >= A - 1, (route, lau)
    elif route in ("gram", "host-gram"):
        assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] <= 1, (route, lau)     # no pass over X per component; T = X R
    elif route == "type2":
        assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] == 0 and lau["xty"] >= 1, (route, lau)
    elif route in ("dual", "batch-dual", "cv-dual"):
        assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] == 0 and lau["xty"] >= 1, (route, lau)
    elif route in ("batch", "cv"):
        assert passes == 0 and lau["xty"] >= 1 and lau["small"] >= 1, (route, lau)


def _algo(name):
    import pls_amd
    return getattr(pls_amd, "ALGO_" + name)


def run_fit(handles, route, X, Y, f32=False):
    """dict(W, P, Q, R, T, B) as fp64 numpy arrays (T in its storage type, None for KERNEL_TYPE2) and the launch counts"""
    import pls_amd
    form, which, algo, fuse, method, mem = FIT_ROUTES[route]
    h = handles[which]
    h.set_option(pls_amd.OPT_ALGO, _algo(algo)); h.set_option(pls_amd.OPT_FUSE, fuse)
    try:
        h.timing()
        meth = pls_amd.KERNEL_TYPE1 if method == 1 else pls_amd.KERNEL_TYPE2
        if mem == "host":
            dt = np.float32 if f32 else np.float64
            out = h.fit_host(X.astype(dt), Y.astype(dt), A, method=meth, dtype=dt)
        else:
            out = h.fit_device(_dev(X, f32), _dev(Y, f32), A, method=meth)
            h.synchronize()
            out = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
        lau = h.timing()["launches"]
    finally:
        if which != "dual":
            h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
        h.set_option(pls_amd.OPT_FUSE, 1)
    return out, lau


def run_batch(handles, route, X, Y, f32=False):
    """fit_batch on [Y | Y with its rows reversed]: dict(R, Q, tt, B), each (2, ...)"""
    h = handles["dual" if route == "batch-dual" else "default"]
    Xd, Yd = _dev(X, f32), _dev(np.concatenate([Y, hd.second_responses(Y)], axis=1), f32)
    M = Y.shape[1]
    if route == "batch-dual":   # the route, not a fall-back: one sweep over X and G is all it books for Q, tt, ssy
        h.timing()
        h.fit_batch(Xd, Yd, M, A, want=("Q", "tt", "ssy")); h.synchronize()
        t = h.timing()
        es = 4 if f32 else 8
        assert t["launches"]["xty"] == 1 and t["bytes"]["xty"] == X.shape[0] * X.shape[1] * es + X.shape[0] ** 2 * 8, t
    h.timing()
    out = h.fit_batch(Xd, Yd, M, A, want=("R", "Q", "tt", "B")); h.synchronize()
    lau = h.timing()["launches"]
    return {k: v.cpu().numpy() for k, v in out.items()}, lau


def run_cv(handles, route, X, Y, f32=False):
    """cv_folds over the three contiguous folds: E (M, 3 ts, A)"""
    h = handles["dual" if route == "cv-dual" else "general"]
    h.timing()
    E = h.cv_folds(_dev(X, f32), _dev(Y, f32), A, hd.fold_indices(X.shape[0])).cpu().numpy()
    t = h.timing()
    if route == "cv-dual":
        es = 4 if f32 else 8
        assert t["launches"]["xty"] == 1 and t["bytes"]["xty"] == X.shape[0] * X.shape[1] * es + X.shape[0] ** 2 * 8, t
    return E, t["launches"]


def _b_errors(R, Q, B, Bref):
    """rel_fro(B_c, Bref[c]) for c = 1..A from the route's R and Q; the route's own B at c = A counts too"""
    Bs = hd.b_by_components(R, Q)
    err = np.array([hd.rel_fro(Bs[c], Bref[c]) for c in range(A)])
    if B is not None:
        err[A - 1] = max(err[A - 1], hd.rel_fro(B, Bref[A - 1]))
    return err


def _record(case, route, form, err, ef, floor):
    err, ef = np.atleast_1d(err), np.atleast_1d(ef)
    bound = np.maximum(floor, MARGIN * ef)
    c = int(np.argmax(err / bound))
    ratio = float(np.max(err / np.maximum(ef, 1e-16)))
    RATIOS.append((hd.case_name(*case), route, form, float(err[c]), float(ef[c]), ratio, float(err[c] / bound[c])))
    print(f"{hd.case_name(*case)} {route} [{form}]: err_hip {err}  err_form {ef}  err_hip/err_form {ratio:.3g}  err_hip/bound {err[c] / bound[c]:.3g}")
    return bound


def check_route(handles, case, route):
    family, N, K, M, f32 = case
    X, Y, fx = _case(case)
    form = _form(route, N)
    form_key = "f32_storage" if (f32 and form == "kernel") else form   # (fp32 storage of the scores: the oracle's emulation)
    floor = FLOOR_B32 if f32 else FLOOR_B
    if route in FIT_ROUTES:
        out, lau = run_fit(handles, route, X, Y, f32)
        print(route, lau)
        err = _b_errors(out["R"], out["Q"], out["B"], fx["B_ref"])
        bound = _record(case, route, form, err, fx["err_form_" + form_key], floor)
        _launch_check(route, lau, N, K, None)
        assert np.isfinite(out["B"]).all() and (err <= bound).all(), (route, err, bound)
        if family in ("plain", "graded"):   # the invariants and t^T t at the tolerances of tests/test_gpu_parity.py
            assert np.allclose((out["W"] ** 2).sum(0), 1.0, atol=1e-12), route
            assert np.allclose(out["P"].T @ out["R"], np.eye(A), atol=1e-8), route
            if out["T"] is not None:
                assert np.allclose((out["T"].astype(np.float64) ** 2).sum(0), fx["tt_ref"], rtol=1e-9), route
    elif route.startswith("batch"):
        out, lau = run_batch(handles, route, X, Y, f32)
        print(route, lau)
        err = _b_errors(out["R"][0], out["Q"][0], out["B"][0], fx["B_ref"])
        bound = _record(case, route, form, err, fx["err_form_" + form_key], floor)
        # the second response set is another problem on the same X: held to what the form achieves on IT
        err2 = _b_errors(out["R"][1], out["Q"][1], out["B"][1], fx["B2_ref"])
        bound2 = _record(case, route + " (2nd set)", form, err2, fx["err_form2_" + form_key], floor)
        _launch_check(route, lau, N, K, None)
        assert (err <= bound).all() and (err2 <= bound2).all(), (route, err, bound, err2, bound2)
        if family in ("plain", "graded"):
            assert np.allclose(out["tt"][0], fx["tt_ref"], rtol=1e-9), route
    else:
        E, lau = run_cv(handles, route, X, Y, f32)
        print(route, lau)
        err = np.linalg.norm(E - fx["E_ref"]) / np.linalg.norm(Y[hd.fold_indices(N).reshape(-1)])
        bound = _record(case, route, form, err, float(fx["err_form_E_" + form_key]), FLOOR_E)
        _launch_check(route, lau, N, K, None)
        assert np.isfinite(E).all() and err <= bound[0], (route, err, bound)


FP64_CASES = [c for c in hd.all_cases() if not c[4]]
F32_CASE = hd.F32_CASE + (True,)


@pytest.mark.parametrize("route", ALL_ROUTES)
@pytest.mark.parametrize("case", FP64_CASES, ids=lambda c: hd.case_name(*c))
def test_route_on_hard_data(handles, case, route):
    check_route(handles, case, route)


@pytest.mark.parametrize("route", F32_ROUTES)
def test_route_on_hard_data_fp32_storage(handles, route):
    """`offset` with offsets fp32 holds exactly, inputs rounded once to fp32; the reference is that of the rounded inputs"""
    check_route(handles, F32_CASE, route)


def test_resident_gram_is_the_tall_auto_route(handles):
    """both single-launch routes book one launch: on the tall shapes AUTO must be the X^T X form, not the per-component
    resident kernel an explicit KERNEL request gets -- other arithmetic, other bits"""
    for N, K, M in hd.SHAPES:
        if N <= 1024:
            continue
        X, Y, _ = _case(("offset_x", N, K, M, False))
        a, _ = run_fit(handles, "single-launch", X, Y)
        b, _ = run_fit(handles, "single-launch-auto", X, Y)
        assert not np.array_equal(a["B"], b["B"]), (N, K, M)


# ---- power-of-two scaling, bit for bit -----------------------------------------------------------------------------------------
SCALINGS = ((40, -9), (-40, 13))
SCALE_CASES = [(fam, N, K, M) for fam in ("plain", "graded") for N, K, M in hd.SHAPES]


def _run_any(handles, route, X, Y, f32):
    """name -> (array, exponent of two it scales with under X 2^e, Y 2^f as a function (e, f) -> int)"""
    if route in FIT_ROUTES:
        out, _ = run_fit(handles, route, X, Y, f32)
        sc = dict(W=lambda e, f: 0, P=lambda e, f: 0, R=lambda e, f: 0, T=lambda e, f: e, Q=lambda e, f: f - e, B=lambda e, f: f - e)
        return {k: (out[k], sc[k]) for k in sc if out.get(k) is not None}
    if route.startswith("batch"):
        out, _ = run_batch(handles, route, X, Y, f32)
        sc = dict(R=lambda e, f: 0, Q=lambda e, f: f - e, tt=lambda e, f: 2 * e, B=lambda e, f: f - e)
        return {k: (out[k], sc[k]) for k in sc}
    E, _ = run_cv(handles, route, X, Y, f32)
    return {"E": (E, lambda e, f: f)}


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("case", SCALE_CASES, ids=lambda c: hd.case_name(*c))
def test_power_of_two_scaling_is_exact(handles, case, dt):
    """X 2^e, Y 2^f for (e, f) = (+40, -9), (-40, +13): W, P, R bit-identical, T = T0 2^e, Q = Q0 2^(f - e), B = B0 2^(f - e)
    (fit_batch: tt = tt0 2^(2e); cv_folds: E = E0 2^f) on every route.  +-40 keeps (X^T Y)^T (X^T Y) and every fp32 score
    normal."""
    f32 = dt == "f32"
    X, Y, _ = _case(case + (False,))
    if f32:
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    broken = []
    for route in ALL_ROUTES:
        base = _run_any(handles, route, X, Y, f32)
        for e, f in SCALINGS:
            got = _run_any(handles, route, np.ldexp(X, e), np.ldexp(Y, f), f32)
            for k, (a0, sc) in base.items():
                want = np.ldexp(a0.astype(np.float64), sc(e, f))
                have = got[k][0].astype(np.float64)
                if not np.array_equal(want, have):
                    rel = float(np.max(np.abs(want - have)) / max(float(np.max(np.abs(want))), 1e-300))
                    broken.append((route, (e, f), k, f"{rel:.2e}"))
    print(hd.case_name(*case + (False,)), dt, "broken:", broken)
    assert not broken, broken


def test_zz_write_ratio_table():
    """the figures of this run: per (case, route) the device's worst error over the component counts, the CPU figure of its
    form at that count, the worst ratio of the two, and the share of the bound used"""
    if not RATIOS:   # (run on its own: nothing to tabulate)
        return
    lines = [f"{'case':28s} {'route':20s} {'form':7s} {'err_hip':>9s} {'err_form':>9s} {'hip/form':>9s} {'hip/bound':>9s}"]
    for name, route, form, eh, ef, ratio, used in RATIOS:
        lines.append(f"{name:28s} {route:20s} {form:7s} {eh:9.2e} {ef:9.2e} {ratio:9.3g} {used:9.3g}")
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("PLS_HARD_ACCURACY_FILE")
    if out:
        with open(out, "w") as fh:
            fh.write(text)
