"""Cross-validation folds under the sample-space plan (pls_hip_cv_folds with PLS_HIP_ALGO_DUAL): the parts that need no GPU.

dual_cv_folds below restates the route in numpy, step for step as pls_amd/csrc/plan_dual_cv.hpp enqueues it: G = X X^T once,
then per fold the recursion of the plan on vectors of length N with the 0/1 mask m of the fold's training rows --
Y_0 = diag(m) Y, Z = G Y_a on all rows, c_j and tt summed over the training rows, the score t formed for EVERY row (on a
held-out row it is that row's score under the fold's model), Y_a deflated on the training rows, and
E[m][fold ts + i, a] = Y[row_i, m] - sum_{a' <= a} t_a'[row_i] q_a'[m].  It is checked against one oracle refit per fold at the
bar of test_batched_cv_folds.  tests/test_gpu_dual_cv.py takes its cases and its reference from here.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import DATA
from test_dual_ref import dominant_eigvec

BAR = 1e-8  # max|E - ref| < BAR * max(max|ref|, 1): test_batched_cv_folds

# name -> (N, K, M, A, ts, nf, storage)
CASES = {
    "nir-loo": (60, 401, 1, 10, 1, 60, "f64"),
    "nir-25x18": (60, 401, 1, 6, 18, 25, "f64"),
    "toy-loo": (10, 15, 2, 2, 1, 10, "f64"),
    "smallest": (2, 40, 1, 1, 1, 2, "f64"),              # the smallest legal call
    "one-training-row": (9, 40, 2, 1, 8, 3, "f64"),
    "17x1003": (17, 1003, 1, 5, 1, 17, "f64"),
    "97x1500": (97, 1500, 3, 8, 10, 12, "f64"),
    "130-columns": (130, 600, 1, 3, 1, 130, "f64"),      # two column blocks of the matrix-core product, the second ragged
    "129x70001": (129, 70001, 1, 6, 1, 129, "f64"),      # K beyond the batched route, one row past a block of G
    "513x4100": (513, 4100, 2, 20, 51, 10, "f64"),
    "largest-M": (300, 2000, 32, 4, 30, 6, "f64"),
    "A-near-rank": (64, 300, 1, 40, 4, 16, "f64"),       # 60 training rows
    "1031x9000-f32": (1031, 9000, 8, 8, 100, 5, "f32"),  # more than one row per thread of the step kernel
    "2049x3001-f32": (2049, 3001, 4, 6, 512, 4, "f32"),
}


def fold_indices(N, ts, nf):
    """leave-one-out in row order, or nf draws of ts distinct rows (as test_batched_cv_folds draws them)"""
    if ts == 1 and nf == N:
        return np.arange(N, dtype=np.int64)[:, None]
    rng = np.random.default_rng(7)
    return np.ascontiguousarray(np.stack([rng.permutation(N)[:ts] for _ in range(nf)]), dtype=np.int64)


def case_data(name):
    """(X, Y, A, idx) of a case: fp64 host images (of the fp32 data where the storage is fp32)"""
    from oracle import pls_oracle as po
    oracle = _oracle()
    N, K, M, A, ts, nf, dt = CASES[name]
    z = lambda f: np.asfortranarray(oracle.z_scores(po.read_csv(os.path.join(DATA, f))))
    if name.startswith("nir"):
        X, Y = z("nir.csv"), z("octane.csv")
    elif name.startswith("toy"):
        X, Y = z("toyX.csv"), z("toyY.csv")
    else:
        X, Y = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    if dt == "f32":
        X, Y = X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    assert X.shape == (N, K) and Y.shape == (N, M)
    return np.asfortranarray(X), np.asfortranarray(Y), A, fold_indices(N, ts, nf)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import pls_oracle as po
    return po.OracleLib()


def fold_reference(X, Y, A, idx):
    """(M, nobs, A): one oracle refit per fold on its training rows, residuals of the held-out rows under R[:, :c] Q[:, :c]^T"""
    oracle = _oracle()
    N, M = Y.shape
    nf, ts = idx.shape
    ref = np.zeros((M, nf * ts, A))

    def fold(f):
        test = idx[f]
        train = np.setdiff1d(np.arange(N), test)
        c = oracle.plsr(np.asfortranarray(X[train]), np.asfortranarray(Y[train]), A)
        R, Q = np.asarray(c["R"]), np.asarray(c["Q"])
        S = X[test] @ R  # (ts, A)
        for nc in range(1, A + 1):
            ref[:, f * ts:(f + 1) * ts, nc - 1] = (Y[test] - S[:, :nc] @ Q[:, :nc].T).T

    # the folds are independent and the oracle is a C library (no interpreter lock while it runs): a few at a time
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(fold, range(nf)))
    return ref


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the reference of a case, computed once per session and left unchanged (read-only)"""
    X, Y, A, idx = case_data(name)
    ref = fold_reference(X, Y, A, idx)
    ref.setflags(write=False)
    return ref


def dual_cv_folds(X, Y, A, idx, power_iters=48):
    """E (M, nobs, A) of the route, fp64"""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    N, M = Y.shape
    nf, ts = idx.shape
    G = X @ X.T  # the only product with X
    E = np.zeros((M, nf * ts, A))
    for f in range(nf):
        te = idx[f]
        m = np.ones(N); m[te] = 0.0
        Ya = np.array(Y * m[:, None], order="F")  # Y_0 = diag(m) Y
        T = np.zeros((N, A)); tt = np.zeros(A)
        pred = np.zeros((ts, M))
        for a in range(A):
            Z = G @ Ya  # all N rows: those of the test set come for free
            if M == 1:
                u, g = Ya[:, 0].copy(), Z[:, 0].copy()
            else:
                S = Ya.T @ Z
                S = np.triu(S) + np.triu(S, 1).T
                qh = dominant_eigvec(S, power_iters)
                u, g = Ya @ qh, Z @ qh
            nw = np.sqrt(u @ g)
            c = ((m[:, None] * T[:, :a]).T @ g) / tt[:a]
            t = (g - T[:, :a] @ c) / nw  # every row
            T[:, a] = t
            tt[a] = (m * t) @ t
            q = (Ya.T @ t) / tt[a]
            Ya -= np.outer(m * t, q)
            pred += np.outer(t[te], q)
            E[:, f * ts:(f + 1) * ts, a] = (Y[te] - pred).T
    return E


def rel_err(E, ref):
    return np.abs(E - ref).max() / max(np.abs(ref).max(), 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_dual_cv_restatement_against_oracle_refits(name):
    X, Y, A, idx = case_data(name)
    ref = case_reference(name)
    with np.errstate(all="ignore"):
        E = dual_cv_folds(X, Y, A, idx)
    err = rel_err(E, ref)
    print(f"{name}: {CASES[name]}  max|E - ref| / max(max|ref|, 1) = {err:.2e}")
    assert err < BAR
