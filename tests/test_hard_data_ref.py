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
