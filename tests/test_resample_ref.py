"""Row-weighted replicate fits (pls_hip_fit_resampled: bootstrap and jack-knife of B): the parts that need no GPU.

dual_resample below restates the sample-space route in numpy, step for step as pls_amd/csrc/plan_resample.hpp enqueues it:
G = X X^T once; per replicate s = sqrt(w), Y~_0 = s o Y, the recursion of the plan (tests/test_dual_ref.py: dual_fit) with the
product read back through s, g~ = s o (G (s o Y~_a)); S from the recurrence of tests/test_dual_batch_ref.py, D = S Q^T, and the
back-projection B = X^T (s o D).  B0 is the same computation with unit weights; s1 and s2 accumulate d_b = B_b - B0 in
replicate order.

Yardstick, independent of any square root where the weights are counts: oracle.plsr on the physically repeated rows
X[idx], Y[idx]; for fractional weights the oracle on the scaled rows.  Bars, the project's own: B, B0, Bmean by po.rel_fro
below TOL_B = 1e-10, Q columns (sign-aligned on themselves: no other per-component output exists here) below TOL_COL, tt
relative 1e-9.  se = sqrt(Bm2): every B_b within TOL_B |B0| moves a deviation by at most 2 TOL_B |B0|, so the bar is
po.rel_fro(se_ref, se) < 2 TOL_B / rho with rho = rms_b |B_b - B0|_F / |B0|_F from the yardstick, and rho >= 1e-2 is asserted
as a condition on the inputs.  tests/test_gpu_resample.py takes its cases, its yardstick and its bars from here.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_dual_batch_ref import TOL_TT
from test_dual_cv_ref import fold_indices
from test_dual_ref import TOL_B, TOL_COL, dominant_eigvec
from test_fit_batch_ref import nir_z

RHO_MIN = 1e-2
WEIGHT_SEED = 11

# name -> (N, K, M, A, nrep, storage, weights): "frac" uniform in [0.25, 4], "boot" bootstrap_weights, "loo" jackknife_weights
CASES = {
    "smallest": (3, 40, 1, 1, 3, "f64", "frac"),             # the smallest call with a zero-free weight column
    "17x1003": (17, 1003, 1, 5, 5, "f64", "boot"),           # ragged K, rows dropping out
    "97x1500": (97, 1500, 3, 8, 6, "f64", "frac"),           # M > 1: the direction from the weighted S
    # more than 32 product columns; a second, ragged, 128-column block of both products
    "130x600": (130, 600, 1, 3, 140, "f64", "boot"),
    "largest-M": (150, 800, 32, 4, 3, "f64", "frac"),
    "1031x3000-f32": (1031, 3000, 8, 8, 3, "f32", "boot"),   # more than one row per thread of the step
    "129x40001": (129, 40001, 1, 6, 3, "f64", "boot"),       # K beyond every K x K route, one row past a block of G
    "nir-loo": (60, 401, 1, 3, 60, "f64", "loo"),
    "5000x64": (5000, 64, 2, 4, 4, "f64", "boot"),           # tall: the GPU runs it on a default-plan handle (the general route)
    "A-10": (64, 300, 1, 10, 4, "f64", "boot"),
}
GENERAL_ONLY = ("5000x64",)  # cases the GPU runs on a default-plan handle


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import pls_oracle as po
    return po.OracleLib()


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, Y, Wt) of a case: fp64 host images (of the fp32 data where the storage is fp32), read-only"""
    import pls_amd
    from oracle import pls_oracle as po
    oracle = _oracle()
    N, K, M, A, nrep, dt, kind = CASES[name]
    if name.startswith("nir"):
        X, Y = nir_z(po)
    else:
        X = oracle.synth_x(0, N, K); X = X - X.mean(axis=0)
        Y = oracle.synth_y(0, N, M); Y = Y - Y.mean(axis=0)
    if dt == "f32":
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    if kind == "frac":
        Wt = np.random.default_rng(WEIGHT_SEED).uniform(0.25, 4.0, size=(N, nrep))
    elif kind == "boot":
        Wt = pls_amd.bootstrap_weights(N, nrep, WEIGHT_SEED)
        assert (Wt == 0).any() and (Wt.sum(axis=0) == N).all()
    else:
        Wt = pls_amd.jackknife_weights(N)
    X, Y, Wt = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Wt, dtype=np.float64)
    assert X.shape == (N, K) and Y.shape == (N, M) and Wt.shape == (N, nrep)
    for a in (X, Y, Wt):
        a.setflags(write=False)
    return X, Y, Wt


def _oracle_fit(X, Y, A, w):
    """(Q, tt, B) of the oracle for one weight column: repeated rows for counts, scaled rows otherwise"""
    oracle = _oracle()
    if w is None:
        Xw, Yw = X, Y
    elif np.array_equal(w, np.round(w)):
        idx = np.repeat(np.arange(X.shape[0]), w.astype(np.int64))
        Xw, Yw = X[idx], Y[idx]
    else:
        s = np.sqrt(w)[:, None]
        Xw, Yw = s * X, s * Y
    Xw, Yw = np.asfortranarray(Xw), np.asfortranarray(Yw)
    ref = oracle.plsr(Xw, Yw, A)
    R, Q = np.asarray(ref["R"]), np.asarray(ref["Q"])
    return Q, ((Xw @ R) ** 2).sum(axis=0), np.asarray(oracle.coefficients(ref["R"], ref["Q"]))


def summaries(B, B0):
    """(Bmean, Bm2) of the replicates' coefficients about B0, as the entry point defines them"""
    nrep = B.shape[0]
    s1 = np.zeros_like(B0); s2 = np.zeros_like(B0)
    for b in range(nrep):
        d = B[b] - B0
        s1 += d
        s2 += d * d
    return B0 + s1 / nrep, s2 - s1 * s1 / nrep


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """dict(Q, tt, B, B0, Bmean, se, rho) of a case from the oracle, computed once per session and left unchanged"""
    N, K, M, A, nrep, _, _ = CASES[name]
    X, Y, Wt = case_data(name)
    with ThreadPoolExecutor(max_workers=8) as pool:  # (the oracle is a C library: no interpreter lock while it runs)
        per = list(pool.map(lambda b: _oracle_fit(X, Y, A, None if b < 0 else Wt[:, b]), range(-1, nrep)))
    B0 = per[0][2]
    Q, tt, B = (np.stack([p[i] for p in per[1:]]) for i in range(3))
    Bmean = B.mean(axis=0)
    se = np.sqrt(((B - Bmean) ** 2).sum(axis=0))
    rho = float(np.sqrt(np.mean([np.linalg.norm(B[b] - B0) ** 2 for b in range(nrep)])) / np.linalg.norm(B0))
    y = dict(Q=Q, tt=tt, B=B, B0=B0, Bmean=Bmean, se=se)
    for v in y.values():
        v.setflags(write=False)
    y["rho"] = rho
    return y


def dual_resample(X, Y, A, Wt, power_iters=48):
    """dict(Q (nrep, M, A), tt (nrep, A), B (nrep, K, M), B0, Bmean, Bm2 (K, M)) of the sample-space route, fp64"""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64); Wt = np.asarray(Wt, dtype=np.float64)
    N, K = X.shape
    M = Y.shape[1]
    G = X @ X.T  # the only product with X besides the back-projections

    def one(w):
        s = np.sqrt(w)[:, None]
        Ya = s * Y
        Yin = s * Ya
        U = np.zeros((N, A)); T = np.zeros((N, A)); Q = np.zeros((M, A)); C = np.zeros((A, A)); tt = np.zeros(A)
        for a in range(A):
            Z = s * (G @ Yin)
            if M == 1:
                u, g = Ya[:, 0].copy(), Z[:, 0].copy()
            else:
                S = Ya.T @ Z
                S = np.triu(S) + np.triu(S, 1).T
                qh = dominant_eigvec(S, power_iters)
                u, g = Ya @ qh, Z @ qh
            nw = np.sqrt(u @ g)
            c = (T[:, :a].T @ g) / tt[:a]
            t = (g - T[:, :a] @ c) / nw
            C[:a, a] = c / nw
            tt[a] = t @ t
            q = (Ya.T @ t) / tt[a]
            Ya = Ya - np.outer(t, q)
            Yin = s * Ya
            U[:, a], T[:, a], Q[:, a] = u / nw, t, q
        S = np.zeros((N, A))
        for a in range(A):
            S[:, a] = U[:, a] - S[:, :a] @ C[:a, a]
        return Q, tt, X.T @ (s * (S @ Q.T))

    B0 = one(np.ones(N))[2]
    per = [one(Wt[:, b]) for b in range(Wt.shape[1])]
    Q, tt, B = (np.stack([p[i] for p in per]) for i in range(3))
    Bmean, Bm2 = summaries(B, B0)
    return dict(Q=Q, tt=tt, B=B, B0=B0, Bmean=Bmean, Bm2=Bm2)


def q_column_err(Qg, Qr):
    """per component: relative error of the Q column, sign-aligned on itself"""
    s = np.sign(np.einsum("ma,ma->a", Qr, Qg)); s[s == 0] = 1.0
    return np.linalg.norm(Qg * s - Qr, axis=0) / np.linalg.norm(Qr, axis=0)


def measure(got, y):
    """worst figures over the replicates of whatever `got` holds against the yardstick (or another result with `se`)"""
    from oracle import pls_oracle as po
    w = {}
    nrep = y["tt"].shape[0]
    if "B" in got:
        assert np.isfinite(got["B"]).all()
        w["B"] = max(po.rel_fro(got["B"][b], y["B"][b]) for b in range(nrep))
    for k in ("B0", "Bmean"):
        if k in got:
            w[k] = po.rel_fro(got[k], y[k])
    if "Q" in got:
        w["col"] = max(float(q_column_err(got["Q"][b], y["Q"][b]).max()) for b in range(nrep))
    if "tt" in got:
        w["tt"] = float((np.abs(got["tt"] - y["tt"]) / y["tt"]).max())
    if "Bm2" in got:
        w["se"] = po.rel_fro(y["se"], np.sqrt(np.maximum(got["Bm2"], 0.0)))
    return w


def check(got, y, what):
    """every output `got` holds against the yardstick y at the bars"""
    w = measure(got, y)
    rho = y["rho"]
    print(f"[resample] {what}: rho {rho:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    assert rho >= RHO_MIN, what
    for k in ("B", "B0", "Bmean"):
        if k in w:
            assert w[k] < TOL_B, (what, k)
    if "col" in w:
        assert w["col"] <= TOL_COL, what
    if "tt" in w:
        assert w["tt"] <= TOL_TT, what
    if "se" in w:
        assert w["se"] < 2.0 * TOL_B / rho, what
    return w


@pytest.mark.parametrize("name", list(CASES))
def test_resample_restatement_against_the_yardstick(name):
    N, K, M, A, nrep, dt, kind = CASES[name]
    X, Y, Wt = case_data(name)
    with np.errstate(all="ignore"):
        got = dual_resample(X, Y, A, Wt)
    assert got["B"].shape == (nrep, K, M) and got["Q"].shape == (nrep, M, A) and got["Bm2"].shape == (K, M)
    check(got, case_yardstick(name), f"{name} {CASES[name][:5]}")


def test_unit_weights_restate_the_unweighted_fit():
    """a replicate of unit weights is the fit of (X, Y): B_b == B0 exactly, Bm2 == 0, Bmean == B0"""
    X, Y, _ = case_data("17x1003")
    got = dual_resample(X, Y, 5, np.ones((17, 3)))
    assert np.array_equal(got["B"][1], got["B0"]) and not got["Bm2"].any() and np.array_equal(got["Bmean"], got["B0"])


# ---- the helpers ------------------------------------------------------------------------------------------------------------
def test_bootstrap_weights():
    import pls_amd
    W = pls_amd.bootstrap_weights(23, 7, 5)
    assert W.shape == (23, 7) and W.dtype == np.float64 and W.flags.f_contiguous
    assert (W.sum(axis=0) == 23).all() and (W >= 0).all() and np.array_equal(W, np.round(W))
    assert np.array_equal(W, pls_amd.bootstrap_weights(23, 7, 5))
    assert not np.array_equal(W, pls_amd.bootstrap_weights(23, 7, 6))


def test_jackknife_weights_are_the_complement_of_the_folds():
    import pls_amd
    N = 19
    W = pls_amd.jackknife_weights(N)
    idx = fold_indices(N, 1, N)
    assert W.shape == (N, N) and W.flags.f_contiguous
    for f in range(N):
        held = np.zeros(N, dtype=bool); held[idx[f]] = True
        assert np.array_equal(W[:, f], (~held).astype(np.float64))
    groups = np.array([2, 0, 1] * 6 + [2])
    Wg = pls_amd.jackknife_weights(N, groups)
    assert Wg.shape == (N, 3)
    for j, lab in enumerate((0, 1, 2)):
        assert np.array_equal(Wg[:, j], (groups != lab).astype(np.float64))
    with pytest.raises(pls_amd.PlsHipError):
        pls_amd.jackknife_weights(N, groups[:-1])


def test_resample_se_scaling():
    import pls_amd
    m2 = np.array([[4.0, 0.0], [9.0, -1e-30]])
    assert np.allclose(pls_amd.resample_se(m2, 5, "bootstrap"), np.sqrt(np.maximum(m2, 0) / 4.0), rtol=1e-15)
    assert np.allclose(pls_amd.resample_se(m2, 5, "jackknife"), np.sqrt(np.maximum(m2, 0) * 4.0 / 5.0), rtol=1e-15)
    with pytest.raises(pls_amd.PlsHipError):
        pls_amd.resample_se(m2, 5, "other")
    with pytest.raises(pls_amd.PlsHipError):
        pls_amd.resample_se(m2, 1, "bootstrap")


def test_python_surface_is_exported():
    import pls_amd
    for n in ("bootstrap_weights", "jackknife_weights", "resample_se"):
        assert n in pls_amd.__all__ and callable(getattr(pls_amd, n))
    assert callable(pls_amd.Handle.fit_resampled) and callable(pls_amd.Model.bootstrap) and callable(pls_amd.Model.jackknife)


def test_entry_point_rejects_the_null_handle():
    import pls_amd
    from pls_amd import _lib as L
    z = np.zeros(8)
    p = z.ctypes.data
    rc = pls_amd.lib().pls_hip_fit_resampled(None, p, 2, p, 2, 2, 2, 1, 1, p, 2, 1, L.F64, L.MEM_HOST, None, None, None, p, None, None)
    assert rc == L.ERR_INVALID and not z.any()
