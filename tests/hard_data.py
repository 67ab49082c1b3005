"""Hard input families for the accuracy tests: what the data looks like, not what shape it has.

Every family is built from the seeded generator (oracle/pls_oracle.py: synth_x / synth_y) by elementwise IEEE operations in
a fixed order -- no BLAS product, no transcendental function -- so (family, N, K, M, seed) reproduces the inputs bit for bit
on any machine; the fixtures tests/golden/hard/h_*.npz hold checksums, not matrices.  tests/golden/make_golden.py --hard-only
fits every case in 80-digit arithmetic (mpmath, generator only) and stores B for every component count, the residuals of
three contiguous folds, the B of a second response set (Y with its rows reversed), and err_form: how far each plain-fp64 restatement in the tree --
the oracle's kernel form, its NIPALS form, its type-2 form, dual_fit of tests/test_dual_ref.py -- lands from that reference
on the CPU.  tests/test_hard_data_ref.py pins the fixtures to the live restatements; tests/test_gpu_hard_data.py holds every
route of the library to max(FLOOR, 10 x err_form[its form]).

Nothing here needs a GPU or mpmath.
"""
import os

import numpy as np

from conftest import GOLDEN

A = 6
FAMILIES = ("plain", "offset", "offset_x", "graded", "collinear", "spectra")
# (N, K, M): tall -- three workgroups of the resident fit with a ragged last one, 48 columns (both single-launch resident
# kernels, both first phases of the X^T X form: blocks for M = 1, rows for M = 3), enough rows for the SYRK; wide -- 60 x 400
SHAPES = ((1301, 48, 1), (1301, 48, 3), (60, 400, 1), (60, 400, 2))
SEED = 0x504C5301
TS = {1301: 20, 60: 5}         # held-out rows per fold: folds f = 0, 1, 2 hold rows [f ts, (f + 1) ts)
FORMS = ("kernel", "nipals", "type2", "dual")

# noise levels, tuned on the CPU until the conditions of tests/test_hard_data_ref.py hold (largest err_form <= 1e-5)
COLLINEAR_NOISE_EXP = 12       # X = rank 3 + 2^-12 synth_x
SPECTRA_NOISE_EXP = 10         # X = 1 + bands + 2^-10 synth_x
# the fp32-storage case: `offset` with offsets that fp32 holds exactly, inputs rounded once to fp32
F32_CASE = ("offset", 1301, 48, 1)
F32_OFFSET = 1024.0


def case_name(family, N, K, M, f32=False):
    return f"h_{family}_{N}x{K}_m{M}" + ("_f32" if f32 else "")


def all_cases():
    """(family, N, K, M, f32) of every fixture"""
    out = [(fam, N, K, M, False) for fam in FAMILIES for N, K, M in SHAPES]
    out.append(F32_CASE + (True,))
    return out


def fixture_path(family, N, K, M, f32=False):
    return os.path.join(GOLDEN, "hard", case_name(family, N, K, M, f32) + ".npz")


def fold_indices(N):
    ts = TS[N]
    return np.arange(3 * ts, dtype=np.int64).reshape(3, ts)


def _band(K, centre, half):
    """(1 - u^2)^2 on |u| < 1, u = (k - centre) / half: a C^1 piecewise polynomial"""
    u = (np.arange(K, dtype=np.float64) - centre) / half
    v = 1.0 - u * u
    return np.where(np.abs(u) < 1.0, v * v, 0.0)


def hard_inputs(po, family, N, K, M, seed=SEED, f32=False):
    """(X, Y) of a case: fp64, column-major.  f32: rounded once to fp32 (and held in fp64)."""
    X = np.array(po.synth_x(0, N, K, seed), order="F")
    Y = np.array(po.synth_y(0, N, M, seed), order="F")
    k = np.arange(K)
    if family == "plain":
        pass
    elif family in ("offset", "offset_x"):   # uncentred data; offset_x: X only (the kernel form keeps its digits there)
        off = (F32_OFFSET if f32 else 1.0e4) * (1.0 + (k % 3).astype(np.float64))
        X = X + off[None, :]
        if family == "offset":
            Y = Y + 100.0
    elif family == "graded":            # exact column scaling over 24 binades
        X = np.ldexp(X, -(k % 24)[None, :])
    elif family == "collinear":         # rank 3 plus small noise
        Lt = np.asarray(po.synth_x(0, N, 3, seed ^ 0x1000))       # three latent columns
        V = np.asarray(po.synth_x(0, 3, K, seed ^ 0x2000))        # three loading rows
        S = np.zeros((N, K))
        for j in range(3):
            S = S + Lt[:, j:j + 1] * V[j:j + 1, :]
        X = S + np.ldexp(X, -COLLINEAR_NOISE_EXP)
        Z = np.zeros((N, M))
        for m in range(M):
            for j in range(3):
                Z[:, m] = Z[:, m] + (1.0 + (j + m) % 3) * Lt[:, j]
        Y = Z + np.ldexp(Y, -10)
    elif family == "spectra":           # baseline 1, three smooth overlapping bands, per-row concentrations
        C = 1.0 + np.ldexp(np.asarray(po.synth_x(0, N, 3, seed ^ 0x3000)), -4)
        S = np.ones((N, K))
        for j in range(3):
            S = S + C[:, j:j + 1] * _band(K, K * (j + 1) / 4.0, K / 5.0)[None, :]
        X = S + np.ldexp(X, -SPECTRA_NOISE_EXP)
        Y = np.array(C[:, :M])
    else:
        raise ValueError(family)
    if f32:
        X = X.astype(np.float32).astype(np.float64)
        Y = Y.astype(np.float32).astype(np.float64)
    return np.asfortranarray(X), np.asfortranarray(Y)


def checksum(a):
    return float(np.abs(a).sum())


def load_case(po, family, N, K, M, f32=False):
    """(X, Y, fixture) with the checksums verified"""
    fx = np.load(fixture_path(family, N, K, M, f32))
    X, Y = hard_inputs(po, family, N, K, M, int(fx["seed"]), f32)
    assert checksum(X) == float(fx["x_checksum"]) and checksum(Y) == float(fx["y_checksum"]), (family, N, K, M)
    return X, Y, fx


def second_responses(Y):
    """the second response set of a case: Y with its rows reversed"""
    return np.asfortranarray(Y[::-1])


def fold_residuals(X, Y, idx, fit_B):
    """E (M, nf ts, A): E[m, f ts + i, c - 1] = Y[row, m] - X[row] B_c[:, m] with B_c = fit_B(Xtrain, Ytrain)[c - 1]"""
    nf, ts = idx.shape
    M = Y.shape[1]
    E = np.zeros((M, nf * ts, A))
    for f in range(nf):
        keep = np.ones(X.shape[0], dtype=bool)
        keep[idx[f]] = False
        Bs = fit_B(np.asfortranarray(X[keep]), np.asfortranarray(Y[keep]))
        for c in range(A):
            E[:, f * ts:(f + 1) * ts, c] = (Y[idx[f]] - X[idx[f]] @ Bs[c]).T
    return E


def b_by_components(R, Q):
    """[B_1 .. B_A], B_c = R[:, :c] Q[:, :c]^T"""
    R, Q = np.asarray(R), np.asarray(Q)
    return np.stack([R[:, :c] @ Q[:, :c].T for c in range(1, R.shape[1] + 1)])


def form_fits(oracle, dual_fit, f32=False):
    """name -> (X, Y) -> [B_1 .. B_A]: the plain-fp64 restatements in the tree"""
    fits = {
        "kernel": lambda X, Y: oracle.plsr(X, Y, A),
        "nipals": lambda X, Y: oracle.plsr(X, Y, A, nipals=True),
        "type2": lambda X, Y: oracle.plsr(X, Y, A, method=1),
        "dual": lambda X, Y: dual_fit(X, Y, A),
    }
    if f32:
        fits["f32_storage"] = lambda X, Y: oracle.plsr(X, Y, A, f32_storage=True)
    wrap = lambda f: (lambda X, Y: (lambda c: b_by_components(c["R"], c["Q"]))(f(X, Y)))
    return {k: wrap(f) for k, f in fits.items()}


def rel_fro(a, b):
    d = np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    n = np.linalg.norm(np.asarray(b, dtype=np.float64))
    return d / n if n > 0 else d


def row_orders(N):
    """the same data in three row orders -- as given, reversed, even rows then odd rows.  The order of the rows changes no
    product of the fit (X^T X, X^T Y, X X^T up to a symmetric permutation), only the order of every sum over the rows:
    how far the results of one restatement spread over them is that form's own summation noise"""
    idx = np.arange(N)
    return (idx, idx[::-1], np.concatenate([idx[0::2], idx[1::2]]))


def _worst_over_orders(fit, X, Y, err):
    return np.max([err(fit(np.asfortranarray(X[o]), np.asfortranarray(Y[o]))) for o in row_orders(X.shape[0])], axis=0)


def measure_err_form(oracle, dual_fit, X, Y, fx, f32=False):
    """(err_form, err_form2, err_form_E): per form rel_fro(B_c, B_ref[c]) for c = 1..A (an array of A), the same for the
    second response set against B2_ref (another problem on the same X: its own figures), and the error of the form's fold
    residuals against the reference's, in units of the norm of the held-out responses (a number) -- each the largest over
    row_orders: on the hard families one component count of one run can sit a factor 15 below the next run of the SAME
    restatement with its sums split differently (the oracle's serial and OpenMP builds on offset_x, c = 2: 2.2e-9, 3.2e-8)"""
    idx = fold_indices(X.shape[0])
    ynorm = np.linalg.norm(Y[idx.reshape(-1)])
    Y2 = second_responses(Y)
    eb, eb2, ee = {}, {}, {}
    for name, fit in form_fits(oracle, dual_fit, f32).items():
        eb[name] = _worst_over_orders(fit, X, Y, lambda Bs: np.array([rel_fro(Bs[c], fx["B_ref"][c]) for c in range(A)]))
        eb2[name] = _worst_over_orders(fit, X, Y2, lambda Bs: np.array([rel_fro(Bs[c], fx["B2_ref"][c]) for c in range(A)]))
        ee[name] = max(np.linalg.norm(fold_residuals(X, Y, idx, lambda Xt, Yt, k=k: fit(
            np.asfortranarray(Xt[row_orders(Xt.shape[0])[k]]), np.asfortranarray(Yt[row_orders(Xt.shape[0])[k]]))) - fx["E_ref"]) / ynorm
                       for k in range(3))
    return eb, eb2, ee
