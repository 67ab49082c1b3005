"""Regenerates tests/golden/*.npz.  Run from the repo root:  python tests/golden/make_golden.py

The reference holds no golden vectors and cannot be built here (Eigen absent), so these
fixtures are produced by the C restatement in oracle/pls_oracle.c and are only written when two
independent routes agree with it: the numpy restatement (oracle/pls_oracle.py) and, for m == 1 or
well-separated directions, scikit-learn's NIPALS PLSRegression(scale=False, tol=1e-30).
Inputs: the reference's own example data (tests/golden/data/*.csv, copied verbatim from
/root/reference/{toyX,toyY,nir,octane}.csv) z-scored as src/main.cpp:24-25 does, and seeded
synthetic matrices (generator spec in DESIGN.md) identified by (N, K, M, seed) only.

python tests/golden/make_golden.py --hard-only   writes the hard/h_*.npz and hard/e_*.npz fixtures of tests/hard_data.py alone:
hard input families fitted in 80-digit arithmetic (mpmath, needed by this mode only), byte-identical from run to run.  h_*:
the fits and the fold residuals; e_*: the row-weighted replicates, PRESS and ssy of both response sets, the NIPALS fit with
missing cells and the column statistics of the masked X (about 45 CPU-minutes for all 25 cases).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pls_oracle as po  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")

# (name, N, K, M, A) -- ragged shapes on purpose (non-multiples of every tile size)
SYNTH_CASES = [
    ("s_9x7_m1", 9, 7, 1, 5),
    ("s_9x7_m2", 9, 7, 2, 4),
    ("s_1000x7_m4", 1000, 7, 4, 7),
    ("s_1000x64_m1", 1000, 64, 1, 20),
    ("s_1000x64_m4", 1000, 64, 4, 12),
    ("s_1000x513_m8", 1000, 513, 8, 8),
    ("s_4097x64_m2", 4097, 64, 2, 16),
    ("s_4097x513_m1", 4097, 513, 1, 8),
    ("s_4097x7_m8", 4097, 7, 8, 7),
    ("s_2048x512_m1", 2048, 512, 1, 20),   # small-N twin of BASELINE config 3
    ("s_2048x1024_m4", 2048, 1024, 4, 6),  # small-N twin of config 5
]

# Twins of BASELINE configs 4 and 5 at the configs' OWN K, M and A (only N is reduced).  They hold what pins the
# live oracle -- B, Q, tt and the per-component conditioning -- not the K x A matrices (the GPU tests recompute
# W, P, R, T with the oracle at run time and require its B to reproduce the committed one).
#   (name, N, K, M, A, fp32 storage)
CONFIG_TWINS = [
    ("c4twin_4096x4096_m8_A50_f32", 4096, 4096, 8, 50, True),   # config 4: fp32 storage, 50 components
    ("c5twin_4096x1024_m4_A20", 4096, 1024, 4, 20, False),      # config 5: one shard's K, M, A
]


def sklearn_B(X, Y, A):
    from sklearn.cross_decomposition import PLSRegression
    sk = PLSRegression(n_components=A, scale=False, tol=1e-30, max_iter=200000).fit(X, Y)
    return sk.x_rotations_ @ sk.y_loadings_.T


def fit_and_check(ora, X, Y, A, name, tol=1e-9, with_sklearn=True):
    c = ora.plsr(X, Y, A)
    B = ora.coefficients(c["R"], c["Q"])
    n = po.plsr(X, Y, A)
    e_np = po.rel_fro(po.coefficients(n["R"], n["Q"]), B)
    c2 = ora.plsr(X, Y, A, nipals=True)
    e_ni = po.rel_fro(ora.coefficients(c2["R"], c2["Q"]), B)
    e_sk = 0.0
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if with_sklearn:
                # scikit-learn always centres X and Y; compare on centred copies of the same data
                Xc, Yc = X - X.mean(0), Y - Y.mean(0)
                cc = ora.plsr(Xc, Yc, A)
                e_sk = po.rel_fro(sklearn_B(Xc, Yc, A), ora.coefficients(cc["R"], cc["Q"]))
    print(f"{name:18s} B rel-err vs numpy {e_np:.1e}  vs nipals-form {e_ni:.1e}  vs sklearn "
          + (f"{e_sk:.1e}" if with_sklearn else "(not run)"))
    assert e_np < tol and e_ni < tol and e_sk < 1e-7, name
    # Per-component conditioning: once the latent structure is exhausted the directions of the
    # noise components are nearly degenerate and W/P/R/Q/T columns (not B) of two correct fp64
    # implementations drift apart by a growing factor per component.  Record how far the two
    # independent CPU routes are from the C oracle, column by column; the GPU tests require the
    # HIP path to agree with the oracle to max(1e-10, 20 x this).
    c["col_err"] = np.maximum(po.column_errors(c, n), po.column_errors(c, c2))
    return c, B


def main():
    ora = po.OracleLib()
    if len(sys.argv) > 1 and sys.argv[1] == "--twins-only":
        return twins(ora)
    if len(sys.argv) > 1 and sys.argv[1] == "--hard-only":
        return hard(ora)
    # --- reference example data ---------------------------------------------------------
    for name, fx, fy, A in (("toy_A2", "toyX.csv", "toyY.csv", 2), ("nir_A10", "nir.csv", "octane.csv", 10)):
        X = ora.z_scores(po.read_csv(os.path.join(DATA, fx)))
        Y = ora.z_scores(po.read_csv(os.path.join(DATA, fy)))
        c, B = fit_and_check(ora, X, Y, A, name)
        ev = np.array([po.explained_variance(X, Y, c["R"], c["Q"], k)[0] for k in range(1, A + 1)])
        sse = np.array([po.explained_variance(X, Y, c["R"], c["Q"], k)[1] for k in range(1, A + 1)])
        np.savez(os.path.join(HERE, name + ".npz"), A=A, W=c["W"], P=c["P"], Q=c["Q"], R=c["R"], T=c["T"],
                 B=B, explained_variance=ev, SSE=sse, tt=(c["T"] ** 2).sum(0), col_err=c["col_err"])
    # --- seeded synthetic shapes ----------------------------------------------------------
    for name, N, K, M, A in SYNTH_CASES:
        X = ora.synth_x(0, N, K)
        Y = ora.synth_y(0, N, M)
        c, B = fit_and_check(ora, X, Y, A, name)
        out = dict(N=N, K=K, M=M, A=A, seed=po.SEED_DEFAULT, W=c["W"], P=c["P"], Q=c["Q"], R=c["R"], B=B,
                   tt=(c["T"] ** 2).sum(0), col_err=c["col_err"], x_checksum=float(np.abs(X).sum()), y_checksum=float(np.abs(Y).sum()))
        if N <= 1000:
            out["T"] = c["T"]
        np.savez(os.path.join(HERE, name + ".npz"), **out)
    twins(ora)


def twins(ora):
    # --- twins of configs 4 and 5 at their own K, M, A ------------------------------------------
    for name, N, K, M, A, f32 in CONFIG_TWINS:
        X = ora.synth_x(0, N, K)
        Y = ora.synth_y(0, N, M)
        if f32:  # fp32 storage = the generator's value rounded once; the oracle runs in fp64 on those values
            X = np.asfortranarray(X.astype(np.float32).astype(np.float64))
            Y = np.asfortranarray(Y.astype(np.float32).astype(np.float64))
        # scikit-learn's inner NIPALS loop needs ~1e5 sweeps per component at these sizes: two routes only
        c, B = fit_and_check(ora, X, Y, A, name, with_sklearn=False)
        col_err = c["col_err"]
        if f32:
            # The reference has no fp32 mode; what a correct fp32-STORAGE implementation can reproduce of each
            # component is bounded by the storage rounding of the scores (and of the deflated matrix), amplified by
            # the component's conditioning.  Measure it with two independent routes that emulate that storage
            # (oracle/pls_oracle.c, oracle_set_f32_storage): kernel form and NIPALS-deflation form, fp64 sums.
            k32 = ora.plsr(X, Y, A, f32_storage=True)
            n32 = ora.plsr(X, Y, A, nipals=True, f32_storage=True)
            col_err = np.maximum(col_err, np.maximum(po.column_errors(c, k32), po.column_errors(k32, n32)))
            e32 = po.rel_fro(ora.coefficients(k32["R"], k32["Q"]), B)
            print(f"{name:18s} fp32-storage emulation: B moves by {e32:.1e}; column conditioning {col_err.min():.1e} .. {col_err.max():.1e}")
        np.savez(os.path.join(HERE, name + ".npz"), N=N, K=K, M=M, A=A, seed=po.SEED_DEFAULT, f32=int(f32), Q=c["Q"], B=B,
                 tt=(c["T"] ** 2).sum(0), col_err=col_err, x_checksum=float(np.abs(X).sum()),
                 y_checksum=float(np.abs(Y).sum()))


# --- hard input families with an extended-precision reference (tests/hard_data.py) ---------------------------------------
# python tests/golden/make_golden.py --hard-only      (needs mpmath; no test imports it)
MP_DIGITS = 80


def _mp():
    import mpmath
    mpmath.mp.dps = MP_DIGITS
    return mpmath


def _to_mp(a):
    mp = _mp()
    return np.vectorize(mp.mpf, otypes=[object])(np.asarray(a, dtype=np.float64))


def _to_f64(a):
    """every entry rounded ONCE, to nearest (float(mpf) truncates)"""
    from mpmath import libmp
    return np.vectorize(lambda v: libmp.to_float(v._mpf_, rnd=libmp.round_nearest), otypes=[np.float64])(a)


def _mp_norm(v):
    return _mp().sqrt(v.dot(v))


def mp_direction(S):
    """dominant_direction of oracle/pls_oracle.py: M == 1: w = S; else w = S q, q the dominant eigenvector of S^T S by
    power iteration (in steps of (S^T S)^64, then on S^T S itself) to 1e-45, largest-|.| entry positive"""
    mp = _mp()
    K, M = S.shape
    if M == 1:
        w = S[:, 0].copy()
        return w / _mp_norm(w)
    G = S.T.dot(S)
    P = G / sum(G[i, i] for i in range(M))
    for _ in range(6):
        P = P.dot(P)
        P = P / sum(P[i, i] for i in range(M))
    q = P[:, int(np.argmax([P[i, i] for i in range(M)]))].copy()
    q = q / _mp_norm(q)
    for it in range(100000):
        z = (P if it % 2 == 0 else G).dot(q)      # (the last steps alternate with S^T S itself: no trace of the squaring)
        z = z / _mp_norm(z)
        done = max(abs(z[i] - q[i]) for i in range(M)) < mp.mpf(10) ** -45
        q = z
        if done and it % 2 == 1:
            break
    else:
        raise AssertionError("power iteration did not converge")
    lam = q.dot(G.dot(q))
    assert max(abs(v) for v in (G.dot(q) - lam * q)) < mp.mpf(10) ** -44 * lam   # an eigenpair, whatever route led here
    if q[int(np.argmax([abs(v) for v in q]))] < 0:
        q = -q
    w = S.dot(q)
    return w / _mp_norm(w)


def mp_plsr(X, Y, A, nipals=False):
    """oracle/pls_oracle.py: plsr(method 0) / plsr_nipals on object arrays of mpf: dict(R, Q, tt)"""
    K, M = X.shape[1], Y.shape[1]
    zero = _mp().mpf(0)
    P = np.full((K, A), zero, dtype=object); R = P.copy(); Q = np.full((M, A), zero, dtype=object)
    tts = np.full(A, zero, dtype=object)
    XY = X.T.dot(Y)
    Xd = X.copy()
    for i in range(A):
        w = mp_direction(Xd.T.dot(Y) if nipals else XY)
        r = w.copy()
        for j in range(i):
            r = r - P[:, j].dot(w) * R[:, j]
        t = Xd.dot(w) if nipals else X.dot(r)
        tt = t.dot(t)
        p = (Xd if nipals else X).T.dot(t) / tt
        if nipals:
            q = Y.T.dot(t) / tt
            Xd = Xd - np.outer(t, p)
        else:
            q = XY.T.dot(r) / tt
            XY = XY - np.outer(p, q) * tt
        P[:, i] = p; R[:, i] = r; Q[:, i] = q; tts[i] = tt
    return dict(R=R, Q=Q, tt=tts)


def mp_b_by_components(c):
    A = c["R"].shape[1]
    return [c["R"][:, :n].dot(c["Q"][:, :n].T) for n in range(1, A + 1)]


def _mp_rel(a, b):
    mp = _mp()
    d = a - b
    return mp.sqrt(sum(v * v for v in d.reshape(-1))) / mp.sqrt(sum(v * v for v in b.reshape(-1)))


def save_npz(path, **arrays):
    """np.savez without the time stamps: the same arrays give the same bytes"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def _mp_quot(num, den):
    """num / den entry by entry; a quotient whose denominator is exactly 0 is 0"""
    zero = _mp().mpf(0)
    if np.ndim(num) == 0:
        return zero if den == 0 else num / den
    if np.ndim(den) == 0:
        return np.array([zero if den == 0 else n / den for n in num], dtype=object)
    return np.array([zero if d == 0 else n / d for n, d in zip(num, den)], dtype=object)


def mp_fit_missing(X, Y, mask, A, tol=1e-10, max_iters=500):
    """fit_missing_ref of tests/test_missing_ref.py on object arrays of mpf (mask: True = missing): the same algorithm, the
    same stopping rule.  dict(R, Q, T, iters)"""
    mp = _mp()
    zero = mp.mpf(0)
    N, K = X.shape
    M = Y.shape[1]
    O = np.where(mask, 0, 1).astype(object)            # (Python ints: exact)
    Xa = np.where(mask, zero, X)
    Ya = Y.copy()
    P = np.full((K, A), zero, dtype=object); R = P.copy(); Q = np.full((M, A), zero, dtype=object)
    T = np.full((N, A), zero, dtype=object)
    iters = np.zeros(A, dtype=np.int64)
    tol2 = mp.mpf(tol) * mp.mpf(tol)
    for a in range(A):
        u = Ya[:, int(np.argmax([Ya[:, m].dot(Ya[:, m]) for m in range(M)]))].copy()
        t_prev, it = None, 0
        while True:
            it += 1
            w = _mp_quot(Xa.T.dot(u), O.T.dot(u * u))
            w = _mp_quot(w, mp.sqrt(w.dot(w)))
            t = _mp_quot(Xa.dot(w), O.dot(w * w))
            tt = t.dot(t)
            q = _mp_quot(Ya.T.dot(t), tt)
            if M == 1:
                break
            if it >= 2 and (t - t_prev).dot(t - t_prev) <= tol2 * tt:
                break
            if it >= max_iters:
                break
            t_prev = t
            u = _mp_quot(Ya.dot(q), q.dot(q))
        p = _mp_quot(Xa.T.dot(t), O.T.dot(t * t))
        Xa = Xa - np.outer(t, p) * O
        Ya = Ya - np.outer(t, q)
        r = w.copy()
        for j in range(a):
            r = r - R[:, j] * P[:, j].dot(w)
        P[:, a], R[:, a], Q[:, a], T[:, a], iters[a] = p, r, q, t, it
    return dict(R=R, Q=Q, T=T, iters=iters)


def entry_case(case, ora, X, Y, Xm, Ym, B0m, E1, fx):
    """tests/golden/hard/e_<case>.npz: the 80-digit figures of the resampling, PRESS and missing-value entry points"""
    import hard_data as hd
    from test_dual_ref import dual_fit
    mp = _mp()
    family, N, K, M, f32 = case
    A = hd.A
    Wt = hd.resample_weights(N)
    ex = dict(family=family, N=N, K=K, M=M, A=A, seed=hd.SEED, f32=int(f32), w_checksum=hd.checksum(Wt))
    # resampling: per weight column the fit of (diag(s) X, diag(s) Y), s = sqrt(w); a row of weight 0 is a row of zeros
    fits = []
    for b in range(Wt.shape[1]):
        keep = Wt[:, b] > 0
        s = np.array([mp.sqrt(mp.mpf(float(v))) for v in Wt[keep, b]], dtype=object)
        fits.append(mp_plsr(Xm[keep] * s[:, None], Ym[keep] * s[:, None], A))
    Br = [c["R"].dot(c["Q"].T) for c in fits]
    nrep = len(Br)
    Bmean = sum(Br[1:], Br[0]) / nrep
    Bm2 = sum(((B - Bmean) ** 2 for B in Br[1:]), (Br[0] - Bmean) ** 2)
    dev2 = sum(sum(v * v for v in (B - B0m).reshape(-1)) for B in Br) / nrep
    ex.update(Qr_ref=np.stack([_to_f64(c["Q"]) for c in fits]), ttr_ref=np.stack([_to_f64(c["tt"]) for c in fits]),
              Br_ref=np.stack([_to_f64(B) for B in Br]), Bmean_ref=_to_f64(Bmean),
              se_ref=_to_f64(np.vectorize(mp.sqrt, otypes=[object])(Bm2)),
              rho=float(mp.sqrt(dev2) / mp.sqrt(sum(v * v for v in B0m.reshape(-1)))))
    # PRESS: the folds of the second response set, and both problems' sums from the unrounded residuals
    idx = hd.fold_indices(N)
    nf, ts = idx.shape
    Y2 = Ym[::-1].copy()
    E2 = np.zeros((M, nf * ts, A), dtype=object)
    for f in range(nf):
        keep = np.ones(N, dtype=bool); keep[idx[f]] = False
        Bf = mp_b_by_components(mp_plsr(Xm[keep], Y2[keep], A))
        for c in range(A):
            E2[:, f * ts:(f + 1) * ts, c] = (Y2[idx[f]] - Xm[idx[f]].dot(Bf[c])).T
    held = idx.reshape(-1)
    ex.update(E2_ref=_to_f64(E2), PRESS_ref=np.stack([_to_f64((E * E).sum(axis=1)) for E in (E1, E2)]),
              ssy_ref=np.stack([_to_f64((Yp[held] * Yp[held]).sum(axis=0)) for Yp in (Ym, Y2)]))
    # missing values
    for pat in hd.MISSING_PATTERNS:
        mask = hd.missing_mask(N, K, pat)
        ex["mask_count_" + pat] = int(mask.sum())
        ex["mask_checksum_" + pat] = hd.checksum(np.where(mask, X, 0.0))
        nobs = (~mask).sum(axis=0)
        mean = np.array([Xm[~mask[:, k], k].sum() / int(nobs[k]) for k in range(K)], dtype=object)
        sd = np.array([mp.sqrt(((Xm[~mask[:, k], k] - mean[k]) ** 2).sum() / int(nobs[k] - 1)) if nobs[k] > 1 else mp.nan
                       for k in range(K)], dtype=object)
        ex.update({"zmean_ref_" + pat: _to_f64(mean), "znobs_" + pat: nobs.astype(np.int64),
                   "zsd_ref_" + pat: np.array([float("nan") if nobs[k] < 2 else _to_f64(sd[k:k + 1])[0] for k in range(K)])})
        if not hd.has_missing_reference(family, N, K, M):
            continue
        c = mp_fit_missing(Xm, Ym, mask, A)
        ex.update({"Bm_ref_" + pat: np.stack([_to_f64(b) for b in mp_b_by_components(c)]), "Tm_ref_" + pat: _to_f64(c["T"]),
                   "iters_ref_" + pat: c["iters"]})
    ex.update(hd.measure_entry_forms(ora, dual_fit, X, Y, Wt, fx, ex, f32))
    name = hd.entry_name(family, N, K, M, f32)
    save_npz(os.path.join(HERE, "hard", name + ".npz"), **ex)
    miss = "  ".join(f"{pat}: B {np.max(ex['err_form_m_' + pat]):.1e} T {np.max(ex['err_form_mT_' + pat]):.1e} sens "
                     f"{ex['sens_m_' + pat]:.1e} iters {ex['iters_ref_' + pat].max()}" for pat in hd.MISSING_PATTERNS
                     if "Bm_ref_" + pat in ex)
    return (f"{name:32s} rho {ex['rho']:.2e}   err_form B_b kernel {ex['err_form_r_kernel']:.1e} dual {ex['err_form_r_dual']:.1e}   "
            f"se {ex['err_form_se_kernel']:.1e} {ex['err_form_se_dual']:.1e}   Bmean {ex['err_form_Bmean_kernel']:.1e} "
            f"{ex['err_form_Bmean_dual']:.1e}   PRESS type2 {ex['err_form_P_type2']:.1e} dual {ex['err_form_P_dual']:.1e}   {miss}")


def hard_case(case):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hard_data as hd
    from test_dual_ref import dual_fit
    family, N, K, M, f32 = case
    name = hd.case_name(family, N, K, M, f32)
    ora = po.OracleLib()
    A = hd.A
    X, Y = hd.hard_inputs(po, family, N, K, M, hd.SEED, f32)
    Xm, Ym = _to_mp(X), _to_mp(Y)
    ker = mp_plsr(Xm, Ym, A)
    Bk = mp_b_by_components(ker)
    # the independent check of the reference: the NIPALS form in the same arithmetic
    Bn = mp_b_by_components(mp_plsr(Xm, Ym, A, nipals=True))
    agree = max(_mp_rel(Bn[c], Bk[c]) for c in range(A))
    assert agree < _mp().mpf(10) ** -30, (name, agree)
    B2 = mp_b_by_components(mp_plsr(Xm, Ym[::-1].copy(), A))           # second response set: rows of Y reversed
    idx = hd.fold_indices(N)
    nf, ts = idx.shape
    E = np.zeros((M, nf * ts, A), dtype=object)
    for f in range(nf):
        keep = np.ones(N, dtype=bool); keep[idx[f]] = False
        Bf = mp_b_by_components(mp_plsr(Xm[keep], Ym[keep], A))
        for c in range(A):
            E[:, f * ts:(f + 1) * ts, c] = (Ym[idx[f]] - Xm[idx[f]].dot(Bf[c])).T
    fx = dict(N=N, K=K, M=M, A=A, seed=hd.SEED, f32=int(f32), x_checksum=hd.checksum(X), y_checksum=hd.checksum(Y),
              B_ref=np.stack([_to_f64(b) for b in Bk]), tt_ref=_to_f64(ker["tt"]), B2_ref=np.stack([_to_f64(b) for b in B2]),
              E_ref=_to_f64(E), fold_idx=idx)
    eb, eb2, ee = hd.measure_err_form(ora, dual_fit, X, Y, fx, f32)
    for k in eb:
        fx["err_form_" + k] = eb[k]
        fx["err_form2_" + k] = eb2[k]
        fx["err_form_E_" + k] = ee[k]
    save_npz(os.path.join(HERE, "hard", name + ".npz"), **fx)
    entry = entry_case(case, ora, X, Y, Xm, Ym, Bk[A - 1], E, fx)
    return entry + "\n" + (f"{name:32s} mp forms agree {float(agree):.1e}   err_form B " + " ".join(f"{k} {v.max():.1e}" for k, v in eb.items())
            + "   2nd set " + " ".join(f"{k} {v.max():.1e}" for k, v in eb2.items()) + "   E " + " ".join(f"{k} {v:.1e}" for k, v in ee.items()))


def hard(ora):
    import multiprocessing
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hard_data as hd
    only = sys.argv[2:]                                     # (family names: a subset, while tuning the noise levels)
    cases = [c for c in hd.all_cases() if not only or c[0] in only]
    os.makedirs(os.path.join(HERE, "hard"), exist_ok=True)
    with multiprocessing.Pool(min(len(cases), max(1, (os.cpu_count() or 2) // 2), 16)) as pool:
        for line in pool.imap(hard_case, cases):
            print(line, flush=True)


if __name__ == "__main__":
    main()
