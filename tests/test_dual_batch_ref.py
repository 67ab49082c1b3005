"""Batched fits under the sample-space plan (pls_hip_fit_batch with PLS_HIP_ALGO_DUAL): the parts that need no GPU.

dual_batch below restates the route in numpy, step for step as pls_amd/csrc/plan_dual_batch.hpp enqueues it: G = X X^T once,
then per problem the recursion of the plan on vectors of length N (tests/test_dual_ref.py: dual_fit) keeping U, C, Q and tt;
the recurrence of R in sample space, s_a = u_a - sum_{j<a} C[j, a] s_j, D = S Q^T, and the two back-projections R = X^T S and
B = X^T D.  ssy is the column sum of squares of the fp64 working copy of Y_b.

Yardstick: batch_yardstick of tests/test_fit_batch_ref.py, one oracle KERNEL_TYPE2 fit per problem; problem 0 is Y, problem b
is Y[make_perms(N, nprob - 1, 1)[b - 1]].  Beyond K = 32768 that yardstick's X^T X (K x K) is out of reach: there the oracle's
kernel form per problem, tt[a] = |X r_a|^2.  Bars, the project's own: B by po.rel_fro below 1e-10, the R and Q columns
(sign-aligned on R) below 1e-9, tt relative 1e-9, cumulative R^2 Y absolute 1e-12.  tests/test_gpu_dual_batch.py takes its
cases, its yardstick and its bars from here.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_dual_ref import TOL_B, TOL_COL, dominant_eigvec
from test_fit_batch_ref import batch_yardstick, make_perms, nir_z, stack_problems

TOL_TT = 1e-9    # relative
TOL_R2Y = 1e-12  # absolute, cumulative R^2 Y
PERM_SEED = 1

# name -> (N, K, M, A, nprob, storage, columns): columns = False asserts B and R^2 Y only
CASES = {
    "nir": (60, 401, 1, 3, 6, "f64", True),
    "smallest": (2, 40, 1, 1, 3, "f64", True),            # the smallest legal call
    "17x1003": (17, 1003, 1, 5, 5, "f64", True),
    "97x1500": (97, 1500, 3, 8, 4, "f64", True),
    "130x600-p21": (130, 600, 1, 3, 21, "f64", True),
    "largest-M": (150, 800, 32, 4, 2, "f64", True),
    # the late R columns are ill-determined, and the yardstick's own X^T X form is the weak side there
    "A-near-rank": (64, 300, 1, 40, 3, "f64", False),
    "129x40001": (129, 40001, 1, 6, 3, "f64", True),      # K beyond every other route, one row past a block of G
    "1031x3000-f32": (1031, 3000, 8, 8, 3, "f32", True),  # more than one row per thread of the step kernel
    # more than 32 columns per round; a second, ragged, 128-column block of both products
    "130x600-p140": (130, 600, 1, 3, 140, "f64", True),
}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import pls_oracle as po
    return po.OracleLib()


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, Ys) of a case: fp64 host images (of the fp32 data where the storage is fp32), read-only"""
    from oracle import pls_oracle as po
    oracle = _oracle()
    N, K, M, A, nprob, dt, _ = CASES[name]
    if name == "nir":
        X, Y = nir_z(po)
    else:
        X = oracle.synth_x(0, N, K); X = X - X.mean(axis=0)
        Y = oracle.synth_y(0, N, M); Y = Y - Y.mean(axis=0)
    Ys = stack_problems(Y, make_perms(N, nprob - 1, PERM_SEED))
    if dt == "f32":
        X, Ys = X.astype(np.float32).astype(np.float64), Ys.astype(np.float32).astype(np.float64)
    X, Ys = np.asfortranarray(X), np.asfortranarray(Ys)
    assert X.shape == (N, K) and Ys.shape == (N, nprob * M)
    X.setflags(write=False); Ys.setflags(write=False)
    return X, Ys


def kernel_form_yardstick(oracle, X, Ys, M, A):
    """batch_yardstick without X^T X: the oracle's kernel form per problem, tt[a] = |X r_a|^2"""
    out = {k: [] for k in ("R", "Q", "tt", "B", "ssy")}
    for b in range(Ys.shape[1] // M):
        Yb = np.asfortranarray(Ys[:, b * M:(b + 1) * M])
        ref = oracle.plsr(X, Yb, A)
        R, Q = np.asarray(ref["R"]), np.asarray(ref["Q"])
        out["R"].append(R); out["Q"].append(Q)
        out["tt"].append(((X @ R) ** 2).sum(axis=0))
        out["B"].append(R @ Q.T)
        out["ssy"].append((Yb * Yb).sum(axis=0))
    return {k: np.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """the yardstick of a case, computed once per session and left unchanged (read-only)"""
    N, K, M, A, nprob, _, _ = CASES[name]
    X, Ys = case_data(name)
    form = kernel_form_yardstick if K > 32768 else batch_yardstick
    # the problems are independent and the oracle is a C library (no interpreter lock while it runs): a few at a time
    with ThreadPoolExecutor(max_workers=8) as pool:
        per = list(pool.map(lambda b: form(_oracle(), X, np.asfortranarray(Ys[:, b * M:(b + 1) * M]), M, A), range(nprob)))
    y = {k: np.concatenate([p[k] for p in per]) for k in ("R", "Q", "tt", "B", "ssy")}
    for v in y.values():
        v.setflags(write=False)
    return y


def dual_batch(X, Ys, M, A, power_iters=48):
    """dict(R (nprob, K, A), Q (nprob, M, A), tt (nprob, A), B (nprob, K, M), ssy (nprob, M)) of the route, fp64"""
    X = np.asarray(X, dtype=np.float64); Ys = np.asarray(Ys, dtype=np.float64)
    N, K = X.shape
    nprob = Ys.shape[1] // M
    G = X @ X.T  # the only product with X besides the back-projections
    out = {k: [] for k in ("R", "Q", "tt", "B", "ssy")}
    for b in range(nprob):
        Ya = np.array(Ys[:, b * M:(b + 1) * M], order="F")
        out["ssy"].append((Ya * Ya).sum(axis=0))
        U = np.zeros((N, A)); T = np.zeros((N, A)); Q = np.zeros((M, A)); C = np.zeros((A, A)); tt = np.zeros(A)
        for a in range(A):
            Z = G @ Ya
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
            Ya -= np.outer(t, q)
            U[:, a], T[:, a], Q[:, a] = u / nw, t, q
        S = np.zeros((N, A))
        for a in range(A):
            S[:, a] = U[:, a] - S[:, :a] @ C[:a, a]
        D = S @ Q.T
        out["R"].append(X.T @ S); out["Q"].append(Q); out["tt"].append(tt); out["B"].append(X.T @ D)
    return {k: np.stack(v) for k, v in out.items()}


def column_err(Rg, Qg, Rr, Qr):
    """per component: the larger relative error of the R and the Q column, sign-aligned on R"""
    s = np.sign(np.einsum("ka,ka->a", Rr, Rg)); s[s == 0] = 1.0
    er = np.linalg.norm(Rg * s - Rr, axis=0) / np.linalg.norm(Rr, axis=0)
    eq = np.linalg.norm(Qg * s - Qr, axis=0) / np.linalg.norm(Qr, axis=0)
    return np.maximum(er, eq)


def measure(got, y):
    """worst figures over the problems of whatever `got` holds: B, col (needs R and Q), tt, r2y (needs Q, tt, ssy), ssy"""
    import pls_amd
    from oracle import pls_oracle as po
    w = {}
    nprob = y["ssy"].shape[0]
    if "B" in got:
        assert np.isfinite(got["B"]).all()
        w["B"] = max(po.rel_fro(got["B"][b], y["B"][b]) for b in range(nprob))
    if "R" in got and "Q" in got:
        w["col"] = max(float(column_err(got["R"][b], got["Q"][b], y["R"][b], y["Q"][b]).max()) for b in range(nprob))
    if "tt" in got:
        w["tt"] = float((np.abs(got["tt"] - y["tt"]) / y["tt"]).max())
    if "ssy" in got:
        w["ssy"] = float((np.abs(got["ssy"] - y["ssy"]) / y["ssy"]).max())
    if all(k in got for k in ("Q", "tt", "ssy")):
        r2 = pls_amd.r2y_by_components(got["Q"], got["tt"], got["ssy"])
        w["r2y"] = float(np.abs(r2 - pls_amd.r2y_by_components(y["Q"], y["tt"], y["ssy"])).max())
    return w


def check(got, y, what, columns=True):
    """every output `got` holds against the yardstick y (or another result) at the bars; columns = False: B and R^2 Y only"""
    w = measure(got, y)
    print(f"[dual-batch] {what}: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    if "B" in w:
        assert w["B"] < TOL_B, what
    if "r2y" in w:
        assert w["r2y"] <= TOL_R2Y, what
    if "ssy" in w:
        assert w["ssy"] <= 1e-13, what
    if columns:
        if "col" in w:
            assert w["col"] <= TOL_COL, what
        if "tt" in w:
            assert w["tt"] <= TOL_TT, what
    return w


@pytest.mark.parametrize("name", list(CASES))
def test_dual_batch_restatement_against_the_yardstick(name):
    N, K, M, A, nprob, dt, columns = CASES[name]
    X, Ys = case_data(name)
    with np.errstate(all="ignore"):
        got = dual_batch(X, Ys, M, A)
    assert got["R"].shape == (nprob, K, A) and got["B"].shape == (nprob, K, M)
    check(got, case_yardstick(name), f"{name} {CASES[name][:5]}", columns)


def test_sample_space_recurrence_is_the_recurrence_of_r():
    """R = X^T S with s_a = u_a - sum_j C[j, a] s_j is the r_a = w_a - sum_j C[j, a] r_j of the fit's plan, W = X^T U"""
    rng = np.random.default_rng(5)
    N, K, A = 9, 30, 4
    X = rng.standard_normal((N, K)); U = rng.standard_normal((N, A)); C = np.triu(rng.standard_normal((A, A)), 1)
    W = X.T @ U
    R = np.zeros((K, A)); S = np.zeros((N, A))
    for a in range(A):
        R[:, a] = W[:, a] - R[:, :a] @ C[:a, a]
        S[:, a] = U[:, a] - S[:, :a] @ C[:a, a]
    assert np.allclose(X.T @ S, R, rtol=1e-13, atol=1e-13)
