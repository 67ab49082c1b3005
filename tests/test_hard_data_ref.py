"""The hard-data fixtures (tests/golden/hard/h_*.npz, tests/hard_data.py) against the live CPU restatements: no GPU.

Every case is regenerated bit for bit from (family, N, K, M, seed) and verified by its checksums; err_form -- how far the
oracle's kernel, NIPALS and type-2 forms and dual_fit land from the 80-digit reference -- is measured again and must sit
within a factor 2 of the stored figure, so the fixtures and the yardstick cannot drift apart.  Every figure is the largest
over three row orders of the same data (hard_data.row_orders): the form's own spread over the order of its sums.  A figure at rounding level
(both below 1e-13: a few ulps of a relative Frobenius error, where the order of a BLAS sum moves it by more than a factor)
counts as equal.

Then the conditions that keep the bounds of tests/test_gpu_hard_data.py meaningful:
  * the largest err_form over all cases is <= 1e-5: no bound there exceeds 1e-4, no (case, route) pair is uninformative
    (the second response set of fit_batch, a fit to noise: <= 1e-4);
  * the offset data separates the forms: on `offset_x` (X + 1e4 (1 + k mod 3), Y as generated)
    err_form[type2] >= 100 err_form[kernel] -- measured 1e3 .. 3e5;
  * on `plain` every err_form is < 1e-13.
On `offset` as well (the same X, and Y + 100) the kernel form itself loses digits -- X^T Y is then 1e9 of offset products
over O(N) of signal, and the form deflates it by subtraction: err_form[kernel] 6e-9 .. 3e-8 against err_form[type2]
1e-7 .. 1.4e-6, a factor 17 .. 52, not 100.  What the GPU bounds need of that family is that a type-2 route held to the
kernel form's bound would fail: err_form[type2] > 10 err_form[kernel], asserted below.

The second half does the same for tests/golden/hard/e_*.npz, the fixtures of tests/test_gpu_hard_entry.py (row-weighted
replicates, PRESS, missing values), and shows that the scaling table of that module holds bit for bit in the CPU restatements.
"""
import numpy as np
import pytest

import hard_data as hd
from test_dual_ref import dual_fit

NOISE = 1e-13


def _close(live, stored):
    live, stored = np.asarray(live, dtype=np.float64), np.asarray(stored, dtype=np.float64)
    both_noise = (live < NOISE) & (stored < NOISE)
    return np.all(both_noise | ((live <= 2.0 * stored) & (stored <= 2.0 * live)))


@pytest.fixture(scope="module")
def measured(oracle, po):
    """case -> (err_form, err_form2, err_form_E, fixture): measured once, shared"""
    out = {}
    for case in hd.all_cases():
        X, Y, fx = hd.load_case(po, *case)
        out[case] = hd.measure_err_form(oracle, dual_fit, X, Y, fx, case[4]) + (fx,)
    return out


@pytest.mark.parametrize("case", hd.all_cases(), ids=lambda c: hd.case_name(*c))
def test_fixture_matches_live_restatements(measured, case):
    eb, eb2, ee, fx = measured[case]
    family, N, K, M, f32 = case
    assert (int(fx["N"]), int(fx["K"]), int(fx["M"]), int(fx["A"]), int(fx["f32"])) == (N, K, M, hd.A, int(f32))
    assert fx["B_ref"].shape == (hd.A, K, M) and fx["B2_ref"].shape == (hd.A, K, M) and fx["tt_ref"].shape == (hd.A,)
    assert fx["E_ref"].shape == (M, 3 * hd.TS[N], hd.A) and np.array_equal(fx["fold_idx"], hd.fold_indices(N))
    forms = hd.FORMS + (("f32_storage",) if f32 else ())
    for form in forms:
        print(f"{hd.case_name(*case)} {form}: B live {eb[form].max():.2e} stored {fx['err_form_' + form].max():.2e}   "
              f"E live {ee[form]:.2e} stored {float(fx['err_form_E_' + form]):.2e}")
        assert _close(eb[form], fx["err_form_" + form]), (form, eb[form], fx["err_form_" + form])
        assert _close(eb2[form], fx["err_form2_" + form]), (form, eb2[form], fx["err_form2_" + form])
        assert _close(ee[form], fx["err_form_E_" + form]), (form, ee[form], fx["err_form_E_" + form])


def test_second_response_set_and_scores(oracle, po):
    """B2_ref is the reference of Y with its rows reversed, tt_ref the reference's t^T t: the oracle's kernel form on
    benign data reproduces both to rounding"""
    for N, K, M in hd.SHAPES:
        X, Y, fx = hd.load_case(po, "plain", N, K, M)
        c = oracle.plsr(X, hd.second_responses(Y), hd.A)
        assert hd.rel_fro(hd.b_by_components(c["R"], c["Q"])[-1], fx["B2_ref"][-1]) < 1e-13
        c = oracle.plsr(X, Y, hd.A)
        assert hd.rel_fro((c["T"] ** 2).sum(0), fx["tt_ref"]) < 1e-13


def test_no_bound_is_uninformative(measured):
    worst = max(max(float(np.max(v)) for v in eb.values()) for eb, _, _, _ in measured.values())
    worst2 = max(max(float(np.max(v)) for v in eb2.values()) for _, eb2, _, _ in measured.values())
    worst_e = max(max(ee.values()) for _, _, ee, _ in measured.values())
    print(f"largest err_form: B {worst:.2e}, B of the second response set {worst2:.2e}, E {worst_e:.2e}")
    assert worst <= 1e-5 and worst_e <= 1e-5
    # Y with its rows reversed has lost its relation to X: a fit to noise, worse conditioned than any first set (measured
    # 1.0e-5 on `offset`, and 1e-5 .. 4e-5 for every N between 1200 and 1500).  Its bounds stay below 1e-3, four orders under
    # what one fp32 partial sum costs on the same data (6e-8 times the 1e10 by which these problems amplify 1e-16).
    assert worst2 <= 1e-4


def test_offset_separates_the_forms(measured):
    for case, (eb, _, _, _) in measured.items():
        if case[4] or not case[0].startswith("offset"):
            continue
        ratio = eb["type2"][-1] / eb["kernel"][-1]
        print(f"{hd.case_name(*case)}: err_form[type2] / err_form[kernel] = {ratio:.3g}")
        assert ratio >= (100.0 if case[0] == "offset_x" else 10.0), (case, ratio)


def test_plain_is_benign(measured):
    for case, (eb, eb2, ee, _) in measured.items():
        if case[0] == "plain":
            assert all(np.max(v) < 1e-13 for v in list(eb.values()) + list(eb2.values())), (case, eb, eb2)
            assert all(v < 1e-13 for v in ee.values()), (case, ee)


# ---- the resampling, PRESS and missing-value entry points: tests/golden/hard/e_*.npz ------------------------------------------
# The fixtures hold, per case: the 80-digit fits of the seven row-weighted replicates (hard_data.resample_weights) with their
# mean, standard error and rho; the fold residuals of the second response set with PRESS and ssy of both problems summed in 80
# digits; per missing-cell pattern (hard_data.missing_mask) an 80-digit restatement of fit_missing_ref and the column
# statistics of the masked X; and err_form_* / sens_m_*: where the plain-fp64 restatements land from all that.  Below they are
# pinned to the live restatements by the rule above, and the conditions that keep the bounds of
# tests/test_gpu_hard_entry.py meaningful are asserted.
@pytest.fixture(scope="module")
def entry_measured(oracle, po):
    """case -> (live figures, fixture): measured once, shared"""
    out = {}
    for case in hd.all_cases():
        X, Y, Wt, fx, ex = hd.load_entry(po, *case)
        out[case] = (hd.measure_entry_forms(oracle, dual_fit, X, Y, Wt, fx, ex, case[4]), ex)
    return out


@pytest.mark.parametrize("case", hd.all_cases(), ids=lambda c: hd.entry_name(*c))
def test_entry_fixture_matches_live_restatements(entry_measured, case):
    live, ex = entry_measured[case]
    family, N, K, M, f32 = case
    A, nrep = hd.A, hd.NREP
    assert (str(ex["family"]), int(ex["N"]), int(ex["K"]), int(ex["M"]), int(ex["A"]), int(ex["f32"])) == (family, N, K, M, A, int(f32))
    assert ex["Qr_ref"].shape == (nrep, M, A) and ex["ttr_ref"].shape == (nrep, A) and ex["Br_ref"].shape == (nrep, K, M)
    assert ex["Bmean_ref"].shape == ex["se_ref"].shape == (K, M)
    assert ex["E2_ref"].shape == (M, 3 * hd.TS[N], A) and ex["PRESS_ref"].shape == (2, M, A) and ex["ssy_ref"].shape == (2, M)
    for pat in hd.MISSING_PATTERNS:
        assert ex["zmean_ref_" + pat].shape == ex["zsd_ref_" + pat].shape == ex["znobs_" + pat].shape == (K,)
        assert (("Bm_ref_" + pat) in ex) == hd.has_missing_reference(family, N, K, M)
        if ("Bm_ref_" + pat) in ex:
            assert ex["Bm_ref_" + pat].shape == (A, K, M) and ex["Tm_ref_" + pat].shape == (N, A)
    for k, v in live.items():
        print(f"{hd.entry_name(*case)} {k}: live {np.max(v):.2e} stored {np.max(ex[k]):.2e}")
        if k.startswith("iters"):
            continue
        assert _close(v, ex[k]), (k, v, ex[k])


def test_entry_references_restate_the_benign_case(oracle, po):
    """on `plain` the oracle on the scaled rows reproduces every replicate's Q, t^T t and B, the sums of squares of the
    stored residuals reproduce PRESS, and fit_missing_ref reproduces T and the iteration counts: the 80-digit figures are
    the figures of the operations the entry points document"""
    from test_missing_ref import fit_missing_ref
    from test_resample_ref import q_column_err
    for N, K, M in hd.SHAPES:
        X, Y, Wt, fx, ex = hd.load_entry(po, "plain", N, K, M)
        for b in range(hd.NREP):
            s = np.sqrt(Wt[:, b])[:, None]
            c = oracle.plsr(np.asfortranarray(s * X), np.asfortranarray(s * Y), hd.A)
            assert q_column_err(np.asarray(c["Q"]), ex["Qr_ref"][b]).max() < 1e-12
            assert hd.rel_fro((np.asarray(c["T"]) ** 2).sum(0), ex["ttr_ref"][b]) < 1e-13
        assert hd.press_errors(hd.press_of(fx["E_ref"]), ex["PRESS_ref"][0]) < 1e-13
        assert hd.press_errors(hd.press_of(ex["E2_ref"]), ex["PRESS_ref"][1]) < 1e-13
        held = hd.fold_indices(N).reshape(-1)
        assert np.allclose((Y[held] ** 2).sum(0), ex["ssy_ref"][0], rtol=1e-14) and np.allclose((Y[::-1][held] ** 2).sum(0), ex["ssy_ref"][1], rtol=1e-14)
        for pat in hd.MISSING_PATTERNS if hd.has_missing_reference("plain", N, K, M) else ():
            got = fit_missing_ref(hd.with_missing(X, hd.missing_mask(N, K, pat)), Y, hd.A)
            assert np.array_equal(got["iters"], ex["iters_ref_" + pat]), (N, K, M, pat, got["iters"], ex["iters_ref_" + pat])


def test_entry_conditions(entry_measured):
    """what the GPU bounds rest on: no bound above 1e-4; the replicates spread (rho >= RHO_MIN: the bar on se is 2 FLOOR_B / rho);
    the missing-value form keeps its digits on every family (NIPALS: no squared condition number) and does not hang on where
    its iteration stops; no component runs into max_iters"""
    from test_resample_ref import RHO_MIN
    for case, (live, ex) in entry_measured.items():
        name = hd.entry_name(*case)
        for k, v in live.items():
            if k.startswith("err_form_") and not k.startswith("err_form_m"):
                assert np.max(v) <= 1e-5, (name, k, v)
        print(f"{name}: rho {float(ex['rho']):.3g}")
        assert float(ex["rho"]) >= RHO_MIN, (name, float(ex["rho"]))
        for pat in hd.MISSING_PATTERNS:
            if ("Bm_ref_" + pat) not in ex:
                continue
            print(f"{name} {pat}: err_form_m {np.max(live['err_form_m_' + pat]):.2e}  T {np.max(live['err_form_mT_' + pat]):.2e}  "
                  f"sens_m {live['sens_m_' + pat]:.2e}  iters {ex['iters_ref_' + pat]} / fp64 {live['iters_fp64_' + pat]}")
            assert np.max(live["err_form_m_" + pat]) <= 1e-10 and np.max(live["err_form_mT_" + pat]) <= 1e-10, (name, pat)
            assert live["sens_m_" + pat] <= 1e-7, (name, pat)
            assert ex["iters_ref_" + pat].max() < 500 and live["iters_fp64_" + pat].max() < 500, (name, pat)


def test_offset_separates_the_resampling_forms(entry_measured):
    """on `offset_x` a sample-space route held to the kernel form's bound would fail"""
    for case, (live, ex) in entry_measured.items():
        if case[0] == "offset_x":
            ratio = live["err_form_r_dual"] / live["err_form_r_kernel"]
            print(f"{hd.entry_name(*case)}: err_form_r[dual] / err_form_r[kernel] = {ratio:.3g}")
            assert ratio >= 10.0, (case, ratio)


def test_single_cells_and_the_missing_tile_are_in_the_blocks_mask():
    for N, K, _ in hd.SHAPES:
        (r0, r1), (k0, k1), (kc, rc), (ir, kr) = hd.BLOCKS[N]
        m = hd.missing_mask(N, K, "blocks")
        assert m[r0:r1, k0:k1].all() and (r1 - r0) * (k1 - k0) >= 64 * 16
        assert (~m[:, kc]).sum() == 1 and not m[rc, kc] and (~m[ir]).sum() == 1 and not m[ir, kr]
        assert (~m).sum(axis=0).min() == 1 and (~m).sum(axis=1).min() == 1   # nothing is empty
        mc = hd.missing_mask(N, K, "mcar")
        assert abs(mc.mean() - hd.MCAR_FRACTION) < 0.01 and (~mc).sum(axis=0).min() > 1 and (~mc).sum(axis=1).min() > 1


# ---- the scaling table of tests/test_gpu_hard_entry.py is a property of the algebra ----------------------------------------------
SCALINGS = ((40, -9), (-40, 13))
WEIGHT_EXP = 3


def _scaled(a, n):
    return np.ldexp(np.asarray(a, dtype=np.float64), n)


@pytest.mark.parametrize("family", ["plain", "graded"])
@pytest.mark.parametrize("shape", hd.SHAPES, ids=lambda s: "%dx%d_m%d" % s)
def test_restatements_obey_the_scaling_table(po, oracle, family, shape):
    """X 2^e, Y 2^f, Wt 4^g: dual_resample, fit_missing_ref (both patterns) and xdiag_yardstick scale bit for bit as the table
    of the GPU module says -- powers of two commute with every rounding, and nothing in the algorithms has an absolute scale"""
    from test_missing_ref import fit_missing_ref
    from test_resample_ref import dual_resample
    from test_xdiag_ref import xdiag_yardstick
    N, K, M = shape
    X, Y = hd.hard_inputs(po, family, N, K, M)
    Wt = hd.resample_weights(N)
    A, g = hd.A, WEIGHT_EXP
    with np.errstate(all="ignore"):
        r0 = dual_resample(X, Y, A, Wt)
        rw = dual_resample(X, Y, A, _scaled(Wt, 2 * g))
    for k in ("Q", "B", "B0", "Bmean", "Bm2"):
        assert np.array_equal(r0[k], rw[k]), k
    assert np.array_equal(_scaled(r0["tt"], 2 * g), rw["tt"])
    masks = {pat: hd.missing_mask(N, K, pat) for pat in hd.MISSING_PATTERNS}
    m0 = {pat: fit_missing_ref(hd.with_missing(X, m), Y, A) for pat, m in masks.items()}
    c = oracle.plsr(X, Y, A)
    R, P = np.asarray(c["R"]), np.asarray(c["P"])
    x0 = xdiag_yardstick(X, R, P)
    for e, f in SCALINGS:
        Xs, Ys = _scaled(X, e), _scaled(Y, f)
        with np.errstate(all="ignore"):
            r1 = dual_resample(Xs, Ys, A, _scaled(Wt, 2 * g))
        for k, n in (("Q", f - e), ("B", f - e), ("B0", f - e), ("Bmean", f - e), ("Bm2", 2 * (f - e)), ("tt", 2 * (e + g))):
            assert np.array_equal(_scaled(r0[k], n), r1[k]), ("dual_resample", (e, f), k)
        for pat, m in masks.items():
            m1 = fit_missing_ref(hd.with_missing(Xs, m), Ys, A)
            for k, n in (("W", 0), ("P", 0), ("R", 0), ("T", e), ("Q", f - e), ("B", f - e)):
                assert np.array_equal(_scaled(m0[pat][k], n), m1[k]), ("fit_missing_ref", pat, (e, f), k)
            assert np.array_equal(m0[pat]["iters"], m1["iters"])
        x1 = xdiag_yardstick(Xs, R, P)
        x2 = xdiag_yardstick(Xs, R, P, tvar=_scaled(x0["tvar"], 2 * e))
        for k, n in (("S", e), ("Q", 2 * e), ("ssx", 2 * e), ("sst", 2 * e), ("T2", 0)):
            assert np.array_equal(_scaled(x0[k], n), x1[k]) and np.array_equal(x1[k], x2[k]), ("xdiag_yardstick", (e, f), k)
