"""The sample-space fit plan (PLS_HIP_ALGO_DUAL): the parts that need no GPU.

dual_fit below restates the plan in numpy, step for step as pls_amd/csrc/plan_dual.hpp enqueues it: G = X X^T once, the
component loop on N-sized data (the scores are mutually orthogonal, so the deflated cross product is X^T Y_a with
Y_a = Y - T_a Q_a^T), W and P from one product X^T [U | T diag(1/tt)], R from the recurrence r_a = w_a - sum_j C[j, a] r_j
whose coefficients C[j, a] = p_j^T w_a fall out of the orthogonalisation of the scores.  It is checked against the
oracle's kernel form at the bars of tests/test_gpu_parity.py.
"""
import os

import numpy as np
import pytest

from conftest import DATA

TOL_B = 1e-10
TOL_COL = 1e-9
TOL_INV = 1e-8


def dominant_eigvec(S, iters=48):
    """the library's direction solve (small_kernels.hpp: dominant_eigvec_lds): repeated squaring of S / tr S, two polishing
    steps on S, largest-|.| entry positive"""
    B = S / np.trace(S)
    for _ in range(iters):
        C = B @ B
        nb = C / np.trace(C)
        same = np.all(np.abs(nb - B) <= 4.0e-16 * np.abs(nb) + 1.0e-18)
        B = nb
        if same:
            break
    q = B[:, int(np.argmax(np.diag(B)))].copy()
    for _ in range(2):
        q = S @ q
        q /= np.sqrt(q @ q)
    return q * (-1.0 if q[int(np.argmax(np.abs(q)))] < 0 else 1.0)


def dual_fit(X, Y, A, power_iters=48):
    """dict(W, P, Q, R, T, B, tt) of the sample-space plan, fp64"""
    X = np.asarray(X, dtype=np.float64); Ya = np.array(Y, dtype=np.float64, order="F")
    N, K = X.shape
    M = Ya.shape[1]
    G = X @ X.T
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
    WP = X.T @ np.concatenate([U, T / tt], axis=1)
    W, P = WP[:, :A], WP[:, A:]
    R = np.zeros((K, A))
    for a in range(A):
        R[:, a] = W[:, a] - R[:, :a] @ C[:a, a]
    return dict(W=W, P=P, Q=Q, R=R, T=T, B=R @ Q.T, tt=tt)


def table_cases(oracle, po):
    """(name, X, Y, A): the six rows of the table in INTEGRATION.md's section on the plan"""
    z = lambda f: np.asfortranarray(oracle.z_scores(po.read_csv(os.path.join(DATA, f))))
    rng = np.random.default_rng(20261017)
    yield "toy", z("toyX.csv"), z("toyY.csv"), 2
    yield "nir", z("nir.csv"), z("octane.csv"), 10
    for N, K, M, A in ((97, 1500, 1, 12), (200, 5000, 3, 10), (513, 4100, 2, 20)):
        yield f"synth{N}x{K}", oracle.synth_x(0, N, K), oracle.synth_y(0, N, M), A
    yield "normal", np.asfortranarray(rng.standard_normal((33, 2000))), np.asfortranarray(rng.standard_normal((33, 4))), 8


@pytest.mark.parametrize("row", range(6))
def test_dual_restatement_against_oracle(oracle, po, row):
    name, X, Y, A = list(table_cases(oracle, po))[row]
    ref = oracle.plsr(X, Y, A)
    alt = oracle.plsr(X, Y, A, nipals=True)
    col_err = po.column_errors(ref, alt)
    Bref = oracle.coefficients(ref["R"], ref["Q"])
    got = dual_fit(X, Y, A)
    err_b = po.rel_fro(got["B"], Bref)
    refd = {k: np.asarray(ref[k]) for k in "WPQR"}
    refd["T"] = X @ refd["R"]
    err = po.column_errors(refd, got)
    inv = np.abs(got["P"].T @ got["R"] - np.eye(A)).max()
    print(f"{name}: B {err_b:.2e}  columns {err.max():.2e}  |P^T R - I| {inv:.2e}  col_err {np.max(col_err):.2e}")
    assert err_b < TOL_B
    assert (err <= np.maximum(TOL_COL, 20.0 * np.asarray(col_err))).all(), f"column errors {err}"
    assert inv < TOL_INV
    assert np.allclose((got["W"] ** 2).sum(0), 1.0, atol=1e-12)


def test_algo_dual_constant():
    import pls_amd
    assert pls_amd.ALGO_DUAL == 4
    assert "ALGO_DUAL" in pls_amd.__all__
