"""NIPALS fits of X with missing values (pls_hip_fit_missing and its companions): the parts that need no GPU.

fit_missing_ref restates the algorithm of include/pls_hip.h ("X with missing values") in numpy: NaN in X marks a missing cell,
every inner product over a column or a row runs over the observed cells only and is divided by the sum of squares of the other
factor over the same cells; a quotient with denominator exactly 0 is 0; R by the recursion r_a = w_a - sum_j r_j (p_j^T w_a).
scores_missing_ref is the sequential deflation of rows with a model's W and P, z_scores_missing_ref nanmean / nanstd (ddof 1).
tests/test_gpu_missing.py takes its cases, its yardstick and its bars from here.

Data of a case, from its name (numpy.random.default_rng): X = a rank-8 signal with singular scales 3 ... 1 plus 0.05 noise, Y
from the leading latent columns plus 0.1 noise, both column-centred; then a uniformly random fraction of the cells of X is NaN.

Self-checks of the yardstick, bars as the feature's issue sets them:
  * on the complete data of every case it equals the oracle's plsr: B within 1e-10, W, P, Q, T per column up to sign;
  * the float64 restatement is within 1e-13 of the same restatement in longdouble on B and T (the cases are well conditioned);
  * M > 1: tol = 1e-10 against tol = 1e-14, max_iters = 2000 differs by at most 1e-9 on B and on T.  That difference, per case,
    is the SENSITIVITY the GPU bars for M > 1 rest on: max(1e-10, 10 x sensitivity) (case_sensitivity);
  * an all-NaN row and an all-NaN column give zeros in T[i, :] and W/P/R/B[k, :], everything else finite, B equal to the fit
    with that column removed to 1e-12.
"""
import functools

import numpy as np
import pytest

TOL_F64 = 1e-10   # include/pls_hip.h, "Accuracy": the KERNEL and NIPALS forms in fp64
TOL_F32 = 2e-5    # the same paragraph, fp32 storage
TOL_LONGDOUBLE = 1e-13
TOL_SENSITIVITY = 1e-9

# name -> (N, K, M, A, missing fraction, storage)
CASES = {
    "67x19": (67, 19, 1, 4, 0.15, "f64"),            # one K range of the row sweep, ragged everything
    "130x70": (130, 70, 1, 5, 0.15, "f64"),          # several K ranges, two column lanes per row
    "257x33-m3": (257, 33, 3, 4, 0.15, "f64"),
    "40x300": (40, 300, 1, 5, 0.20, "f64"),
    "40x300-m2": (40, 300, 2, 4, 0.20, "f64"),
    "1031x130-f32": (1031, 130, 1, 6, 0.10, "f32"),  # more than one row block of the row sweep
    "97x1003-m3": (97, 1003, 3, 5, 0.10, "f64"),     # slow convergence: many batches of iterations
    "5000x40": (5000, 40, 1, 3, 0.10, "f64"),        # several row groups of the column sweep
    "33x20011": (33, 20011, 1, 3, 0.10, "f64"),      # the K-split row sweep with hundreds of ranges
    # the implementation's own thresholds (plan_missing.hpp, miss_geom), smallest shapes on either side.  Row sweep: one K range
    # (K < 16 column lanes' worth: 67x19, 5x12) against several (130x70); column lanes that meet in LDS (fewer than 129 fp64 row
    # pairs: 130x70) against none (257x33); one row block (N = 512) against two (N = 513; fp32: 1031).  Column sweep: one row
    # group against several (5000x40); 16-byte packs against single elements is the caller's alignment (the "eigen" layout of
    # test_gpu_missing.py).  M > 1: components of at most 8 iterations, one batch (6 and 7 in 40x300-m2 and 97x1003-m3), against
    # several batches (up to 57 in 257x33-m3).
    "5x12": (5, 12, 1, 2, 0.10, "f64"),
    "512x24": (512, 24, 1, 2, 0.10, "f64"),
    "513x24": (513, 24, 1, 2, 0.10, "f64"),
    # the batch tails of the row sweep's lane walk (miss_row_walk: 8 columns in flight per lane, then a column at a time): the
    # columns a lane owns in the LAST K range, by miss_row_split for 256 compute units and 16-byte packs.  Eight column lanes per
    # row (nine ranges of 72 columns): 57 columns left = 7 or 8 per lane, 65 left = 8 or 9; N = 41 is no multiple of the pack.
    # One column lane (ranges of 9, 8 and 9 columns): 7, 8 and 9 left; N = 601 is no multiple of the fp32 pack of 4.
    "40x633": (40, 633, 1, 3, 0.10, "f64"),
    "41x641": (41, 641, 1, 3, 0.10, "f64"),
    "600x313": (600, 313, 1, 3, 0.10, "f64"),
    "601x304-f32": (601, 304, 1, 3, 0.10, "f32"),
    "602x306": (602, 306, 1, 3, 0.10, "f64"),
}
# name -> (fewest, most) columns a lane owns in the LAST K range of the row sweep, 256 compute units: what the comments above claim.
# tests/test_xdiagmiss_layout.py holds miss_row_split (pls_amd/csrc/miss_layout.hpp) to it.
TAILS = {"40x633": (7, 8), "41x641": (8, 9), "600x313": (7, 7), "601x304-f32": (8, 8), "602x306": (9, 9)}
MULTI = tuple(n for n, c in CASES.items() if c[2] > 1)


def _seed(name):
    return [int(b) for b in name.encode()]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X with NaN, Y, X complete): fp64 host images (of the fp32 data where the storage is fp32), read-only"""
    N, K, M, A, frac, dt = CASES[name]
    rng = np.random.default_rng(_seed(name))
    L = rng.standard_normal((N, 8))
    V = rng.standard_normal((K, 8))
    Xc = (L * np.linspace(3.0, 1.0, 8)) @ V.T + 0.05 * rng.standard_normal((N, K))
    C = rng.standard_normal((max(M, 3), M))
    Y = L[:, :max(M, 3)] @ C + 0.1 * rng.standard_normal((N, M))
    Xc = Xc - Xc.mean(axis=0)
    Y = Y - Y.mean(axis=0)
    if dt == "f32":
        Xc, Y = Xc.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    X = Xc.copy()
    X[rng.random((N, K)) < frac] = np.nan
    X, Y, Xc = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Xc)
    for a in (X, Y, Xc):
        a.setflags(write=False)
    return X, Y, Xc


def _quot(num, den):
    with np.errstate(all="ignore"):
        return np.where(den == 0, 0, num / np.where(den == 0, 1, den))


def fit_missing_ref(X, Y, A, tol=1e-10, max_iters=500, dtype=np.float64):
    """dict(W, P, Q, R, T, B, iters) of the algorithm in arithmetic `dtype`; stop: |t - t_prev| <= tol |t| from it = 2 on"""
    X = np.asarray(X, dtype=dtype)
    Y = np.array(Y, dtype=dtype, ndmin=2)
    if Y.shape[0] != X.shape[0]:
        Y = Y.T
    N, K = X.shape
    M = Y.shape[1]
    obs = ~np.isnan(X)
    O = obs.astype(dtype)
    Xa = np.where(obs, X, 0).astype(dtype)
    Ya = Y.copy()
    W = np.zeros((K, A), dtype=dtype); P = np.zeros((K, A), dtype=dtype); R = np.zeros((K, A), dtype=dtype)
    Q = np.zeros((M, A), dtype=dtype); T = np.zeros((N, A), dtype=dtype)
    iters = np.zeros(A, dtype=np.int64)
    tol2 = dtype(tol) * dtype(tol)
    for a in range(A):
        u = Ya[:, int(np.argmax((Ya * Ya).sum(axis=0)))].copy() if M > 1 else Ya[:, 0].copy()
        t_prev = None
        it = 0
        while True:
            it += 1
            w = _quot(Xa.T @ u, O.T @ (u * u))
            nrm = np.sqrt(w @ w)
            w = _quot(w, nrm)
            t = _quot(Xa @ w, O @ (w * w))
            tt = t @ t
            q = _quot(Ya.T @ t, tt)
            if M == 1:
                break
            if it >= 2 and ((t - t_prev) @ (t - t_prev)) <= tol2 * tt:
                break
            if it >= max_iters:
                break
            t_prev = t
            u = _quot(Ya @ q, q @ q)
        p = _quot(Xa.T @ t, O.T @ (t * t))
        Xa = Xa - np.outer(t, p) * O
        Ya = Ya - np.outer(t, q)
        r = w.copy()
        for j in range(a):
            r = r - R[:, j] * (P[:, j] @ w)
        W[:, a], P[:, a], R[:, a], Q[:, a], T[:, a], iters[a] = w, p, r, q, t, it
    return dict(W=W, P=P, Q=Q, R=R, T=T, B=R @ Q.T, iters=iters)


def scores_missing_ref(X, W, P, dtype=np.float64):
    """sequential deflation of rows with missing cells: t_a = sum_obs x w_a / sum_obs w_a^2, x <- x - t_a p_a"""
    X = np.asarray(X, dtype=dtype)
    obs = ~np.isnan(X)
    O = obs.astype(dtype)
    Xa = np.where(obs, X, 0).astype(dtype)
    A = W.shape[1]
    S = np.zeros((X.shape[0], A), dtype=dtype)
    for a in range(A):
        w = np.asarray(W[:, a], dtype=dtype)
        t = _quot(Xa @ w, O @ (w * w))
        Xa = Xa - np.outer(t, np.asarray(P[:, a], dtype=dtype)) * O
        S[:, a] = t
    return S


def z_scores_missing_ref(X):
    """(Z, mean, sd, nobs): nanmean, nanstd with ddof 1; a column with sd 0 or NaN is NaN throughout"""
    X = np.asarray(X, dtype=np.float64)
    nobs = (~np.isnan(X)).sum(axis=0).astype(np.int64)
    with np.errstate(all="ignore"), __import__("warnings").catch_warnings():
        __import__("warnings").simplefilter("ignore")
        mean = np.nanmean(X, axis=0)
        sd = np.nanstd(X, axis=0, ddof=1)
        Z = (X - mean) / sd
    return Z, mean, sd, nobs


def rel(a, b):
    """relative Frobenius error of a against b (absolute where b is zero)"""
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    n = np.linalg.norm(b.astype(np.float64))
    d = float(np.sqrt(((a - b) ** 2).sum()))
    return d / n if n > 0 else d


def column_err(got, ref, align=True):
    """worst per-column relative error of a matrix whose columns are components, sign-aligned on themselves if asked"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    worst = 0.0
    for a in range(ref.shape[1]):
        g = got[:, a]
        if align and g @ ref[:, a] < 0:
            g = -g
        worst = max(worst, rel(g, ref[:, a]))
    return worst


def measure(got, ref, align):
    """{B, W, P, Q, R, T: error} of whatever `got` holds against ref; columns up to sign where `align`"""
    w = {}
    for k in ("B", "W", "P", "Q", "R", "T"):
        if got.get(k) is not None and ref.get(k) is not None:
            w[k] = rel(got[k], ref[k]) if k == "B" else column_err(got[k], ref[k], align)
    return w


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """the float64 restatement on the case's data with NaN (of the fp32-rounded inputs for fp32 storage), computed once"""
    N, K, M, A, frac, dt = CASES[name]
    X, Y, _ = case_data(name)
    y = fit_missing_ref(X, Y, A)
    for v in y.values():
        v.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def case_sensitivity(name):
    """M > 1: the difference between stopping at tol = 1e-10 and at tol = 1e-14 (max_iters 2000), the larger of B and T"""
    N, K, M, A, frac, dt = CASES[name]
    if M == 1:
        return 0.0
    X, Y, _ = case_data(name)
    tight = fit_missing_ref(X, Y, A, tol=1e-14, max_iters=2000)
    w = measure(case_yardstick(name), tight, align=True)
    return max(w["B"], w["T"])


def gpu_bar(name):
    """the bar of a case on the device: the project's accuracy bars, for M > 1 widened by where the iteration stops"""
    N, K, M, A, frac, dt = CASES[name]
    if dt == "f32":
        return TOL_F32
    return TOL_F64 if M == 1 else max(TOL_F64, 10.0 * case_sensitivity(name))


# ---- self-checks of the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_complete_data_equals_the_oracle(name, oracle):
    N, K, M, A, frac, dt = CASES[name]
    _, Y, Xc = case_data(name)
    got = fit_missing_ref(Xc, Y, A)
    ref = oracle.plsr(Xc, Y, A)
    ref["B"] = np.asarray(oracle.coefficients(ref["R"], ref["Q"]))
    w = measure(got, ref, align=True)
    print(f"[missing] {name} complete data vs the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()), "iters", got["iters"])
    assert w["B"] <= TOL_F64, (name, w)
    if M == 1:
        assert (got["iters"] == 1).all()
    else:
        # The oracle takes the direction from an eigenvector, the restatement stops where |t - t_prev| <= 1e-10 |t|: at a
        # convergence rate rho the columns are then still rho / (1 - rho) x 1e-10 from the fixed point (2e-10 measured at 57
        # iterations).  What is held to the oracle per column is the fixed point itself, the iteration run to tol = 1e-14; how
        # far the default stop is from it is test_sensitivity_to_the_stopping_rule's figure.
        w = measure(fit_missing_ref(Xc, Y, A, tol=1e-14, max_iters=2000), ref, align=True)
        print(f"[missing] {name} complete data vs the oracle, tol 1e-14: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    assert max(w.values()) <= TOL_F64, (name, w)


@pytest.mark.parametrize("name", list(CASES))
def test_float64_against_longdouble(name):
    N, K, M, A, frac, dt = CASES[name]
    X, Y, _ = case_data(name)
    y = case_yardstick(name)
    ld = fit_missing_ref(X, Y, A, dtype=np.longdouble)
    w = measure(y, ld, align=False)
    print(f"[missing] {name} float64 vs longdouble: B {w['B']:.2e}  T {w['T']:.2e}  iters {y['iters']} / {ld['iters']}")
    assert w["B"] <= TOL_LONGDOUBLE and w["T"] <= TOL_LONGDOUBLE, (name, w)


@pytest.mark.parametrize("name", MULTI)
def test_sensitivity_to_the_stopping_rule(name):
    s = case_sensitivity(name)
    print(f"[missing] {name} sensitivity (tol 1e-10 vs 1e-14): {s:.2e}  iters {case_yardstick(name)['iters']}  gpu bar {gpu_bar(name):.2e}")
    assert s <= TOL_SENSITIVITY, (name, s)


def empty_row_column_checks(fit, X, Y, A, i, k):
    """the assertions on a fit `fit(X, Y, A) -> dict` of data whose row i and column k are entirely missing"""
    Xe = np.array(X, order="F")
    Xe[i, :] = np.nan
    Xe[:, k] = np.nan
    got = fit(Xe, Y, A)
    for n in ("W", "P", "R", "B"):
        assert not np.asarray(got[n])[k, :].any(), n
    assert not np.asarray(got["T"])[i, :].any()
    for n in ("W", "P", "R", "B", "Q", "T"):
        assert np.isfinite(np.asarray(got[n])).all(), n
    keep = np.arange(X.shape[1]) != k
    sub = fit(np.asfortranarray(Xe[:, keep]), Y, A)
    e = rel(np.asarray(got["B"])[keep, :], sub["B"])
    print(f"[missing] empty row {i} and column {k}: B against the fit without the column {e:.2e}")
    assert e <= 1e-12


@pytest.mark.parametrize("name", ["67x19", "257x33-m3"])
def test_empty_row_and_column(name):
    N, K, M, A, frac, dt = CASES[name]
    X, Y, _ = case_data(name)
    empty_row_column_checks(fit_missing_ref, X, Y, A, 5, 7)


def test_scores_ref_reproduces_the_training_scores():
    X, Y, Xc = case_data("130x70")
    y = case_yardstick("130x70")
    assert rel(scores_missing_ref(X, y["W"], y["P"]), y["T"]) <= 1e-13
    assert rel(scores_missing_ref(Xc, y["W"], y["P"]), Xc @ y["R"]) <= 1e-12  # complete rows: x^T R


def test_z_scores_ref():
    X, _, _ = case_data("67x19")
    Xz = np.array(X)
    Xz[:, 2] = np.nan; Xz[4, 2] = 1.5   # one observed cell
    Xz[:, 3] = 2.0                      # constant
    Z, mean, sd, nobs = z_scores_missing_ref(Xz)
    assert nobs[2] == 1 and np.isnan(Z[:, 2]).all() and np.isnan(Z[:, 3]).all() and sd[3] == 0
    ok = np.ones(19, dtype=bool); ok[[2, 3]] = False
    assert np.allclose(np.nanmean(Z[:, ok], axis=0), 0, atol=1e-14) and np.allclose(np.nanstd(Z[:, ok], axis=0, ddof=1), 1, rtol=1e-13)
    assert (np.isnan(Z) == np.isnan(Xz))[:, ok].all()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_python_surface_is_exported():
    import pls_amd
    from pls_amd import _lib as L
    assert pls_amd.OPT_MISSING_ITERS == L.OPT_MISSING_ITERS == 10 and "OPT_MISSING_ITERS" in pls_amd.__all__
    for n in ("fit_missing", "scores_missing", "z_scores_missing"):
        assert callable(getattr(pls_amd.Handle, n))
    for n in ("plsr_missing", "scores_missing", "fitted_values_missing"):
        assert callable(getattr(pls_amd.Model, n))


def test_entry_points_reject_the_null_handle():
    """a NULL handle is rejected by all three entry points without being dereferenced, and nothing is written"""
    import pls_amd
    from pls_amd import _lib as L
    z = np.zeros(16)
    p = z.ctypes.data
    lib = pls_amd.lib()
    assert lib.pls_hip_fit_missing(None, p, 2, p, 2, 2, 2, 1, 1, L.F64, L.MEM_HOST, p, p, p, p, p, 2, p, p) == L.ERR_INVALID
    assert lib.pls_hip_scores_missing(None, p, 2, 2, 2, 1, p, p, L.F64, L.MEM_HOST, p, 2) == L.ERR_INVALID
    assert lib.pls_hip_colwise_z_scores_missing(None, p, 2, 2, 2, L.F64, L.MEM_HOST, p, 2, p, p, p) == L.ERR_INVALID
    assert not z.any()
