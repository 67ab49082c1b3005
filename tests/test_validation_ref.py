"""The yardstick of the validation summary (pls_hip_validation, include/pls_hip.h) and its own checks; no GPU needed.

The yardstick is a plain numpy restatement of the formulas in the header: PRESS as the exact sum of the fp64 squares rounded
once (math.fsum), the reference column by the strict-`<` scan from column 0, the signed-rank sum D from a STABLE argsort of
|del| accumulated in integers, probw from the closed formula.  tests/test_gpu_validation.py compares the device with it;
here it is compared with a brute-force O(n^2) rank count, and the entry point is shown to have no CPU path.
"""
import math

import numpy as np
import pytest

EPS = 2.0 ** -52


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def press_ref(E):
    """E (M, nobs, A) -> PRESS (M, A): fsum of the squares"""
    E = np.asarray(E, dtype=np.float64)
    M, _, A = E.shape
    return np.array([[math.fsum((E[m, :, c] * E[m, :, c]).tolist()) for c in range(A)] for m in range(M)])


def ref_column(press_row):
    """first column with the strictly smallest PRESS, scanning from column 0 with `<`"""
    r = 0
    for c in range(1, len(press_row)):
        if press_row[c] < press_row[r]:
            r = c
    return r


def deltas(e_ref, e_alt):
    d = np.abs(e_ref) - np.abs(e_alt)
    return np.abs(d), (d > 0).astype(np.int64) - (d < 0).astype(np.int64)


def signed_rank_sum(e_ref, e_alt):
    """D = sum rank_i * sign_i, ranks 1-based from a stable ascending sort of |del| (ties in row order); a Python int.
    (The products are summed in int64: |D| <= n (n + 1) / 2 < 2^63 for every n that fits in memory, so the sum is exact.)"""
    mag, s = deltas(e_ref, e_alt)
    order = np.argsort(mag, kind="stable")
    n = len(order)
    assert n * (n + 1) // 2 < 2 ** 62
    return int(np.dot(np.arange(1, n + 1, dtype=np.int64), s[order]))


def normalcdf(z):
    a = abs(z)
    poly = 1 + 0.196854 * a + 0.115194 * a * a + 0.000344 * a * a * a + 0.019527 * a * a * a * a
    p = 0.5 / math.pow(poly, 4)
    return p if z < 0 else 1.0 - p


def probw_from_d(d, n):
    t = float(n * (n + 1)) / 2.0
    v = (t - d) / 2.0
    ev = t / 2.0
    sv = math.sqrt(float(n * (n + 1) * (2 * n + 1)) / 24.0)
    return 1.0 - normalcdf((v - ev) / sv)


def summary_ref(E, alpha=0.1, press=None):
    """(press, ref, D, probw, best): D (M, A) object array of Python ints (0 at alt >= ref), probw NaN at alt >= ref"""
    E = np.asarray(E, dtype=np.float64)
    M, nobs, A = E.shape
    press = press_ref(E) if press is None else press
    ref = np.array([ref_column(press[m]) for m in range(M)], dtype=np.int64)
    D = np.zeros((M, A), dtype=object)
    probw = np.full((M, A), np.nan)
    best = ref + 1
    for m in range(M):
        for alt in range(ref[m]):
            D[m, alt] = signed_rank_sum(E[m, :, ref[m]], E[m, :, alt])
            probw[m, alt] = probw_from_d(float(D[m, alt]), nobs)
        hits = [alt for alt in range(ref[m]) if probw[m, alt] > alpha]
        if hits:
            best[m] = hits[0] + 1
    return press, ref, D, probw, best


# ---- the inputs ---------------------------------------------------------------------------------------------------------
def synth_residuals(M, nobs, A, seed):
    """residuals with a PRESS minimum in the interior and alternatives on both sides of alpha = 0.1: per response a common
    base ~ N(0, 1), column c = (1 + g_c) base + 0.3 N(0, 1) with g_c growing away from c* = 2A/3 - (m mod 3) -- by a few
    1/sqrt(nobs) below c* (so that the nearest alternatives are NOT significantly worse), by 0.05 per column above"""
    rng = np.random.default_rng(seed)
    E = np.empty((M, nobs, A))
    for m in range(M):
        base = rng.standard_normal(nobs)
        cs = max(0, (2 * A) // 3 - (m % 3))
        for c in range(A):
            k = abs(c - cs)
            g = ((0.6 * k if k <= 2 else 4.0 * k) / math.sqrt(nobs)) if c < cs else 0.05 * k
            E[m, :, c] = (1.0 + g) * base + 0.3 * rng.standard_normal(nobs)
    return E


def check_preconditions(E, summary, alpha=0.1, ties_expected=False):
    """what keeps a comparison from being a coin toss; asserted on the yardstick alone"""
    press, ref, _, probw, _ = summary
    M, nobs, A = E.shape
    for m in range(M):
        if A > 1:
            two = np.sort(press[m])[:2]
            assert (two[1] - two[0]) > 100 * nobs * EPS * two[1], f"response {m}: PRESS minimum not separated: {two}"
        for alt in range(ref[m]):
            assert abs(probw[m, alt] - alpha) > 1e-6, f"probw[{m}, {alt}] = {probw[m, alt]} too close to alpha"
            if not ties_expected:
                mag, _ = deltas(E[m, :, ref[m]], E[m, :, alt])
                assert len(np.unique(mag)) == nobs, f"ties in |del| of pair ({m}, {alt})"


# ---- the yardstick against brute force ----------------------------------------------------------------------------------
def _brute_d(e_ref, e_alt):
    mag, s = deltas(e_ref, e_alt)
    n = len(mag)
    d = 0
    for i in range(n):
        rank = 1 + sum(1 for j in range(n) if mag[j] < mag[i] or (mag[j] == mag[i] and j < i))
        d += rank * int(s[i])
    return d


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 257])
@pytest.mark.parametrize("decimals", [None, 1])
def test_signed_rank_sum_against_rank_count(n, decimals):
    rng = np.random.default_rng(100 + n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    if decimals is not None:  # many ties and zeros
        a, b = np.round(a, decimals), np.round(b, decimals)
    assert signed_rank_sum(a, b) == _brute_d(a, b)
    assert signed_rank_sum(a, a) == 0
    assert abs(signed_rank_sum(a, b)) <= n * (n + 1) // 2


def test_probw_formula():
    # D = 0: v = ev, z = 0, normalcdf(0) = 1 - 0.5 = 0.5
    assert probw_from_d(0.0, 10) == 0.5
    # all differences positive: D = t, v = 0, the smallest p-value; all negative: the largest
    n = 20
    t = n * (n + 1) // 2
    assert probw_from_d(float(t), n) > 0.99 and probw_from_d(float(-t), n) < 0.01
    assert probw_from_d(1.0, 1) == pytest.approx(1.0 - normalcdf(-1.0))
    # n(n+1)(2n+1) beyond 2^64 (n = 3e6): Python integers do not wrap
    assert 0.0 <= probw_from_d(1e9, 3_000_000) <= 1.0


def test_reference_column_scan():
    assert ref_column([3.0, 2.0, 2.0, 5.0]) == 1               # first of equal minima
    assert ref_column([float("nan"), 1.0, 0.5]) == 0           # nothing is < NaN
    assert ref_column([2.0, float("nan"), 1.0]) == 2           # a NaN never replaces the minimum
    assert ref_column([1.0]) == 0


def test_generator_meets_the_preconditions_small():
    for (M, nobs, A, seed) in [(1, 60, 10, 1), (3, 1000, 12, 2)]:
        E = synth_residuals(M, nobs, A, seed)
        s = summary_ref(E)
        check_preconditions(E, s)
        assert all(0 < r < A - 1 for r in s[1]), "PRESS minimum not in the interior"


def test_entry_point_has_no_cpu_path():
    """without a device no handle can be made (PLS_HIP_ERR_DEVICE), so Handle.validation cannot be reached; the entry point
    itself rejects the NULL handle instead of dereferencing it"""
    import torch
    import pls_amd
    E = synth_residuals(1, 8, 3, 0)
    if not torch.cuda.is_available():
        with pytest.raises(pls_amd.PlsHipError) as e:
            pls_amd.Handle().validation(E)
        assert e.value.code == 2  # PLS_HIP_ERR_DEVICE
    out = np.zeros(3)
    rc = pls_amd.lib().pls_hip_validation(None, E.ctypes.data, 8, 3, 1, 0, out.ctypes.data, None, None, None)
    assert rc == 1 and not out.any()


def test_python_surface_is_exported():
    import pls_amd
    assert (pls_amd.RESS, pls_amd.MSE) == (0, 1) and pls_amd.OPT_VALIDATION_LDS_ROWS == 9
    for name in ("validation", "optimal_num_components", "print_validation"):
        assert callable(getattr(pls_amd.Model, name))
    assert callable(pls_amd.Handle.validation)
