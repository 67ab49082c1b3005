"""Cross-validated fits of many response sets under the sample-space plan (pls_hip_cv_press_batch with PLS_HIP_ALGO_DUAL): the
parts that need no GPU.

dual_cv_press_batch below restates the route in numpy, step for step as pls_amd/csrc/plan_dual_cvbatch.hpp enqueues it:
G = X X^T once; the table pos (position of a row in a fold's test set, -1: a training row) once per FOLD, shared by the
problems; the work items item = b num_folds + f in that order, in rounds; per item the masked recursion of
tests/test_dual_cv_ref.py on Y_0 = diag(m_f) Y_b -- the held-out rows of Y_0 are set to zero, so they never enter the model --
with the residual of a held-out row stored at its test position and the item's partial PRESS summed over the positions; after
every round the partials added to PRESS_b in item order, continuing the running sum, so every (b, m, c) adds its folds in fold
order wherever the round boundaries fall.  ssy likewise from the held-out responses.

Problem 0 is Y, problem b a seeded row permutation of Y.  The reference is one oracle refit per fold and problem on the rows
outside the fold (fold_reference of tests/test_dual_cv_ref.py applied to Y_b), at that module's bar for cross-validation
residuals.  tests/test_gpu_dual_cvbatch.py takes its cases and its reference from here.
"""
import functools

import numpy as np
import pytest

from test_dual_cv_ref import BAR, CASES, case_data, fold_reference, rel_err
from test_dual_ref import dominant_eigvec

PRESS_TOL = 1e-12  # |PRESS - sum E^2| <= PRESS_TOL * sum E^2, entry by entry: a sum of at most 2730 squares, every term
                   # positive, is off by at most nobs eps = 3e-13 of itself in ANY order of summation

# name -> (case of test_dual_cv_ref, K, nprob): the smallest shapes at which each code path can go wrong
CASES_B = {
    "smallest": ("smallest", 40, 3),                  # 2 x 40, leave-one-out: the smallest legal call
    "one-training-row": ("one-training-row", 40, 2),  # 9 x 40, 3 folds of 8
    "17x1003": ("17x1003", 1003, 5),                  # ragged K
    "97x1500": ("97x1500", 1500, 4),                  # 12 folds of 10, rows repeated across folds, not all rows covered: ssy over
                                                      # observations; 144 product columns, so the matrix-core product
    "130-columns": ("130-columns", 600, 21),          # leave-one-out: 2730 items
    "largest-M": ("largest-M", 2000, 2),              # M = 32
    "1031x3000-f32": ("1031x9000-f32", 3000, 3),      # N > 1024: more than one row per thread of the step kernel
}


def problem_rows(N, nprob):
    """(nprob, N): the identity, then seeded permutations of the rows"""
    return np.stack([np.arange(N)] + [np.random.default_rng(1000 + b).permutation(N) for b in range(1, nprob)])


@functools.lru_cache(maxsize=None)
def case_data_b(name):
    """(X, Ys, M, A, idx, nprob): fp64 host images; Ys is N x (nprob M), problem b the columns [b M, (b + 1) M)"""
    base, K, nprob = CASES_B[name]
    X, Y, A, idx = case_data(base)
    X = np.asfortranarray(X[:, :K])
    N, M = Y.shape
    Ys = np.asfortranarray(np.concatenate([Y[r] for r in problem_rows(N, nprob)], axis=1))
    for a in (X, Ys, idx):
        a.setflags(write=False)
    return X, Ys, M, A, idx, nprob


@functools.lru_cache(maxsize=None)
def case_reference_b(name):
    """(nprob, M, nobs, A): one oracle refit per fold and problem, computed once per session and left unchanged (read-only)"""
    X, Ys, M, A, idx, nprob = case_data_b(name)
    ref = np.stack([fold_reference(X, np.asfortranarray(Ys[:, b * M:(b + 1) * M]), A, idx) for b in range(nprob)])
    ref.setflags(write=False)
    return ref


def dual_cv_press_batch(X, Ys, M, A, idx, round_cap=None, power_iters=48):
    """(PRESS (nprob, M, A), ssy (nprob, M), E (nprob, M, nobs, A)) of the route, fp64"""
    X = np.asarray(X, dtype=np.float64); Ys = np.asarray(Ys, dtype=np.float64)
    N = X.shape[0]
    nprob = Ys.shape[1] // M
    nf, ts = idx.shape
    nobs = nf * ts
    G = X @ X.T  # the only product with X
    pos = np.full((nf, N), -1)  # once per fold
    for f in range(nf):
        pos[f, idx[f]] = np.arange(ts)
    items = nprob * nf
    nround = items if not round_cap else min(round_cap, items)
    PRESS = np.full((nprob, M, A), np.nan); ssy = np.full((nprob, M), np.nan)
    E = np.zeros((nprob, M, nobs, A))
    for i0 in range(0, items, nround):
        nb = min(nround, items - i0)
        pressp = np.zeros((nb, M, A)); ssyp = np.zeros((nb, M))
        for it in range(nb):
            b, f = divmod(i0 + it, nf)
            te = idx[f]
            m = (pos[f] < 0).astype(np.float64)
            Yb = Ys[:, b * M:(b + 1) * M]
            Ya = np.array(Yb * m[:, None], order="F")  # Y_0 = diag(m_f) Y_b: the held-out rows are zero and stay zero
            yte = Yb[te].copy()                        # (ts, M), by test position
            ssyp[it] = (yte * yte).sum(axis=0)
            T = np.zeros((N, A)); tt = np.zeros(A)
            pred = np.zeros((ts, M))
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
                c = ((m[:, None] * T[:, :a]).T @ g) / tt[:a]
                t = (g - T[:, :a] @ c) / nw  # every row
                T[:, a] = t
                tt[a] = (m * t) @ t
                q = (Ya.T @ t) / tt[a]
                Ya -= np.outer(m * t, q)
                pred += np.outer(t[te], q)
                e = yte - pred  # at the test positions
                E[b, :, f * ts:(f + 1) * ts, a] = e.T
                pressp[it, :, a] = (e * e).sum(axis=0)
        for it in range(nb):  # the reduce kernel: item order, continuing the running sum
            b, f = divmod(i0 + it, nf)
            if f == 0:
                PRESS[b] = 0.0; ssy[b] = 0.0
            PRESS[b] += pressp[it]; ssy[b] += ssyp[it]
    return PRESS, ssy, E


def press_err(PRESS, E):
    """max over the entries of |PRESS - sum_o E^2| / sum_o E^2 (0 where both are 0)"""
    S = (E * E).sum(axis=-2)
    d = np.abs(PRESS - S)
    with np.errstate(all="ignore"):
        r = np.where(S > 0, d / S, np.where(d == 0, 0.0, np.inf))
    return float(np.max(r))


def ssy_of(Ys, M, idx):
    """(nprob, M): the sum of squares of every problem's responses over the held-out observations"""
    rows = idx.reshape(-1)
    nprob = Ys.shape[1] // M
    return (Ys[rows] ** 2).sum(axis=0).reshape(nprob, M)


@pytest.mark.parametrize("name", list(CASES_B))
def test_dual_cvbatch_restatement_against_oracle_refits(name):
    X, Ys, M, A, idx, nprob = case_data_b(name)
    ref = case_reference_b(name)
    with np.errstate(all="ignore"):
        PRESS, ssy, E = dual_cv_press_batch(X, Ys, M, A, idx)
    err = rel_err(E, ref)
    perr = press_err(PRESS, E)
    print(f"{name}: {X.shape[0]} x {X.shape[1]}, M = {M}, A = {A}, folds {idx.shape[0]} x {idx.shape[1]}, nprob = {nprob}:  "
          f"max|E - ref| / max(max|ref|, 1) = {err:.2e}   max rel |PRESS - sum E^2| = {perr:.2e}")
    assert err < BAR
    assert perr <= PRESS_TOL
    S = ssy_of(Ys, M, idx)
    assert np.all(np.abs(ssy - S) <= PRESS_TOL * S)
    assert np.isfinite(PRESS).all() and np.isfinite(ssy).all()


@pytest.mark.parametrize("cap", [1, 5, 7])
def test_dual_cvbatch_restatement_rounds(cap):
    """a problem's 12 folds straddle rounds of 5 and 7 and leave a ragged last round: the same bits as in one round"""
    X, Ys, M, A, idx, nprob = case_data_b("97x1500")
    with np.errstate(all="ignore"):
        one = dual_cv_press_batch(X, Ys, M, A, idx)
        capped = dual_cv_press_batch(X, Ys, M, A, idx, round_cap=cap)
    for a, b in zip(one, capped):
        assert np.array_equal(a, b)


def test_cases_are_those_of_the_fold_tests():
    for name, (base, K, nprob) in CASES_B.items():
        assert base in CASES and K <= CASES[base][1] and nprob >= 2
