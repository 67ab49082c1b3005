"""Hard input families for the accuracy tests: what the data looks like, not what shape it has.

Every family is built from the seeded generator (oracle/pls_oracle.py: synth_x / synth_y) by elementwise IEEE operations in
a fixed order -- no BLAS product, no transcendental function -- so (family, N, K, M, seed) reproduces the inputs bit for bit
on any machine; the fixtures tests/golden/hard/h_*.npz hold checksums, not matrices.  tests/golden/make_golden.py --hard-only
fits every case in 80-digit arithmetic (mpmath, generator only) and stores B for every component count, the residuals of
three contiguous folds, the B of a second response set (Y with its rows reversed), and err_form: how far each plain-fp64 restatement in the tree --
the oracle's kernel form, its NIPALS form, its type-2 form, dual_fit of tests/test_dual_ref.py -- lands from that reference
on the CPU.  tests/test_hard_data_ref.py pins the fixtures to the live restatements; tests/test_gpu_hard_data.py holds every
route of the library to max(FLOOR, 10 x err_form[its form]).

The same cases carry the inputs of the entry points that are not fits of (X, Y) alone: seven columns of row weights
(resample_weights), two layouts of missing cells (missing_mask) -- both reproducible bit for bit as well -- and, in
tests/golden/hard/e_*.npz, the 80-digit figures of the row-weighted replicates, of PRESS and ssy over the folds of both response
sets, of the NIPALS fit with missing cells and of the column statistics of the masked X, with the err_form of every restatement
against them (measure_entry_forms).  tests/test_gpu_hard_entry.py holds pls_hip_fit_resampled, pls_hip_cv_press_batch,
pls_hip_fit_missing and its companions to them.

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



# ---- inputs of the resampling, PRESS and missing-value entry points (tests/golden/hard/e_*.npz) ---------------------------------
NREP = 7                       # six bootstrap draws (integer counts, rows dropping out) and one column of fractional weights
WEIGHT_SEED = 11
MISSING_PATTERNS = ("mcar", "blocks")
MCAR_FRACTION, BLOCKS_FRACTION = 0.15, 0.05
# "blocks": N -> (rows, columns) of the tile that is missing entirely, then (column kc, its one observed row), (row ir, its one
# observed column) -- all outside the tile.  A row with one observed cell has the score x / w_k, a column with one the weight
# x / u_i: with M > 1 the iteration is no longer a power iteration and, at 60 x 400, cycles for most positions of the two cells
# on at least one family (fit_missing_ref in fp64: of 384 random draws 7 converged on every family).  With these positions no
# component needs more than 52 iterations and fp64 stays within 2e-11 of the reference, which tests/test_hard_data_ref.py
# asserts: a condition on the inputs, tuned on the CPU like the noise levels above.
BLOCKS = {1301: ((64, 128), (16, 32), (40, 700), (900, 5)), 60: ((16, 48), (128, 192), (30, 44), (1, 6))}
# M > 1 iterates: the 80-digit restatement is made at 60 x 400 for every family, at 1301 x 48 for these two
MISSING_MULTI_TALL = ("offset", "collinear")


def entry_name(family, N, K, M, f32=False):
    return "e" + case_name(family, N, K, M, f32)[1:]


def entry_path(family, N, K, M, f32=False):
    return os.path.join(GOLDEN, "hard", entry_name(family, N, K, M, f32) + ".npz")


def has_missing_reference(family, N, K, M):
    return M == 1 or N == 60 or family in MISSING_MULTI_TALL


def resample_weights(N):
    """(N, 7) fp64, column-major: pls_amd.bootstrap_weights(N, 6, 11), then 0.25 + 3.75 u with u = synth_x / 32 + 1 / 2 (the
    generator's one-column matrix lies inside (-9, 9): an exact affine step into [0, 1))"""
    import pls_amd
    from oracle import pls_oracle as po
    x = np.asarray(po.synth_x(0, N, 1, SEED ^ 0x4000))[:, 0]
    u = np.ldexp(x, -5) + 0.5
    assert (u >= 0).all() and (u < 1).all()
    Wt = np.concatenate([pls_amd.bootstrap_weights(N, NREP - 1, WEIGHT_SEED), (0.25 + 3.75 * u)[:, None]], axis=1)
    return np.asfortranarray(Wt, dtype=np.float64)


def missing_mask(N, K, pattern):
    """(N, K) bool, True = missing.  "mcar": 15 % of the cells, uniformly at random.  "blocks": one whole 64 x 16 tile (at
    60 x 400: 32 x 64 cells), one column and one row with a single observed cell each, and 5 % random cells on top (the two
    single cells and the rest of their column and row are set last)"""
    rng = np.random.default_rng([int(b) for b in f"{pattern}_{N}x{K}".encode()])
    if pattern == "mcar":
        return rng.random((N, K)) < MCAR_FRACTION
    if pattern != "blocks":
        raise ValueError(pattern)
    (r0, r1), (k0, k1), (kc, rc), (ir, kr) = BLOCKS[N]
    m = rng.random((N, K)) < BLOCKS_FRACTION
    m[r0:r1, k0:k1] = True
    m[:, kc] = True
    m[ir, :] = True
    m[rc, kc] = False
    m[ir, kr] = False
    assert (~m[:, kc]).sum() == 1 and (~m[ir, :]).sum() == 1
    return m


def with_missing(X, mask):
    Xn = np.array(X, order="F")
    Xn[mask] = np.nan
    return Xn


def load_entry(po, family, N, K, M, f32=False):
    """(X, Y, Wt, fixture of the fits, fixture of the entry points) with every checksum verified"""
    X, Y, fx = load_case(po, family, N, K, M, f32)
    ex = np.load(entry_path(family, N, K, M, f32))
    Wt = resample_weights(N)
    assert checksum(Wt) == float(ex["w_checksum"]), (family, N, K, M)
    for pat in MISSING_PATTERNS:
        m = missing_mask(N, K, pat)
        assert int(m.sum()) == int(ex["mask_count_" + pat]) and checksum(np.where(m, X, 0.0)) == float(ex["mask_checksum_" + pat]), pat
    return X, Y, Wt, fx, ex


def press_of(E):
    """column sums of squares of fold residuals E (..., nobs, A) -> (..., A)"""
    return (np.asarray(E) ** 2).sum(axis=-2)


def se_of(Bm2):
    return np.sqrt(np.maximum(np.asarray(Bm2, dtype=np.float64), 0.0))


def resample_forms(oracle):
    """name -> (X, Y, Wt) -> dict(Q (nrep, M, A), tt (nrep, A), B (nrep, K, M), B0, Bmean, Bm2): the oracle's kernel form on the
    scaled rows, and the restatement of the sample-space route"""
    from test_resample_ref import dual_resample, summaries

    def kernel(X, Y, Wt):
        def one(w):
            s = np.sqrt(w)[:, None]
            c = oracle.plsr(np.asfortranarray(s * X), np.asfortranarray(s * Y), A)
            return np.asarray(c["Q"]), (np.asarray(c["T"]) ** 2).sum(axis=0), np.asarray(c["R"]) @ np.asarray(c["Q"]).T
        B0 = one(np.ones(X.shape[0]))[2]
        Q, tt, B = (np.stack(v) for v in zip(*[one(Wt[:, b]) for b in range(Wt.shape[1])]))
        Bmean, Bm2 = summaries(B, B0)
        return dict(Q=Q, tt=tt, B=B, B0=B0, Bmean=Bmean, Bm2=Bm2)

    def dual(X, Y, Wt):
        with np.errstate(all="ignore"):
            return dual_resample(X, Y, A, Wt)
    return {"kernel": kernel, "dual": dual}


RESAMPLE_FIGURES = ("r", "se", "Bmean", "Q", "tt")


def resample_errors(got, ex):
    """RESAMPLE_FIGURES of a resampling result against the 80-digit figures of the fixture: B (the worst replicate), se =
    sqrt(max(Bm2, 0)), Bmean by rel_fro; the worst column of Q, sign-aligned on itself; the worst relative error of t^T t"""
    from test_resample_ref import q_column_err
    nrep = ex["Br_ref"].shape[0]
    eb = max(rel_fro(got["B"][b], ex["Br_ref"][b]) for b in range(nrep))
    eq = max(float(q_column_err(got["Q"][b], ex["Qr_ref"][b]).max()) for b in range(nrep))
    et = float((np.abs(got["tt"] - ex["ttr_ref"]) / ex["ttr_ref"]).max())
    return np.array([eb, rel_fro(se_of(got["Bm2"]), ex["se_ref"]), rel_fro(got["Bmean"], ex["Bmean_ref"]), eq, et])


def press_errors(P, Pref):
    """largest entrywise |P - Pref| / Pref"""
    return float(np.max(np.abs(np.asarray(P) - Pref) / Pref))


def missing_errors(got, ex, pat):
    """per component count c: the larger of rel_fro(B_c, Bm_ref[c]) and the relative error of column c of T"""
    Bs = b_by_components(got["R"], got["Q"])
    T = np.asarray(got["T"], dtype=np.float64)
    Bref, Tref = ex["Bm_ref_" + pat], ex["Tm_ref_" + pat]
    return (np.array([rel_fro(Bs[c], Bref[c]) for c in range(A)]),
            np.array([rel_fro(T[:, c], Tref[:, c]) for c in range(A)]))


def measure_entry_forms(oracle, dual_fit, X, Y, Wt, fx, ex, f32=False):
    """name -> figure, every err_form_* and sens_m_* of an e_*.npz fixture: what the plain-fp64 restatements in the tree
    achieve against the 80-digit figures, each the largest over row_orders"""
    from test_missing_ref import fit_missing_ref, measure as missing_measure
    N, K = X.shape
    M = Y.shape[1]
    out = {}
    for name, fit in resample_forms(oracle).items():
        e = np.max([resample_errors(fit(np.asfortranarray(X[o]), np.asfortranarray(Y[o]), np.asfortranarray(Wt[o])), ex)
                    for o in row_orders(N)], axis=0)
        for k, v in zip(RESAMPLE_FIGURES, e):
            out[f"err_form_{k}_{name}"] = float(v)
    idx = fold_indices(N)
    fits = form_fits(oracle, dual_fit, f32)
    Ys = (Y, second_responses(Y))
    for name in ("type2", "dual"):
        worst = 0.0
        for k in range(3):
            reorder = lambda Xt, Yt, k=k, fit=fits[name]: fit(np.asfortranarray(Xt[row_orders(Xt.shape[0])[k]]),
                                                               np.asfortranarray(Yt[row_orders(Xt.shape[0])[k]]))
            for p in range(2):
                worst = max(worst, press_errors(press_of(fold_residuals(X, Ys[p], idx, reorder)), ex["PRESS_ref"][p]))
        out["err_form_P_" + name] = worst
    for pat in MISSING_PATTERNS:
        if not has_missing_reference(fx_family(ex), N, K, M):
            continue
        Xn = with_missing(X, missing_mask(N, K, pat))
        eb, et, its = np.zeros(A), np.zeros(A), np.zeros(A, dtype=np.int64)
        for o in row_orders(N):
            got = fit_missing_ref(Xn[o], Y[o], A)
            got["T"] = got["T"][np.argsort(o)]
            b, t = missing_errors(got, ex, pat)
            eb, et, its = np.maximum(eb, b), np.maximum(et, t), np.maximum(its, got["iters"])
        out["err_form_m_" + pat], out["err_form_mT_" + pat], out["iters_fp64_" + pat] = eb, et, its
        if M > 1:
            w = missing_measure(fit_missing_ref(Xn, Y, A), fit_missing_ref(Xn, Y, A, tol=1e-14, max_iters=5000), True)
            out["sens_m_" + pat] = max(w["B"], w["T"])
        else:
            out["sens_m_" + pat] = 0.0
    return out


def fx_family(ex):
    return str(ex["family"])


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
