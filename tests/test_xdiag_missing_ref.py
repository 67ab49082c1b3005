"""X-space diagnostics of rows with missing cells (pls_hip_x_diagnostics_missing): the parts that need no GPU.

xdiag_missing_ref restates the definition of include/pls_hip.h in numpy.  NaN in X marks a missing cell; for row i with observed
columns O:  q_0 = sum_O x_k^2;  for a = 0 .. A-1:  t_a = sum_O x_k W[k,a] / sum_O W[k,a]^2 (denominator exactly 0: 0),
x_k <- x_k - t_a P[k,a] on O,  q_{a+1} = sum_O x_k^2.  S[i,a] = t_a, Q[i,c-1] = q_c, T2[i,c-1] = sum_{a<c} t_a^2 / tvar[a],
ssx = [sum_i q_0, column sums of Q], sst = column sums of S^2, nobs = |O|; tvar None: sst / (N - 1).
tests/test_gpu_xdiag_missing.py and tests/test_xdiagmiss_layout.py take their cases, the yardstick and the bars from here.

Cases: those of tests/test_missing_ref.py (their data, W and P from their yardstick fit), and the smallest shapes on either side
of every threshold of xdiagmiss_geom_of (pls_amd/csrc/xdiagmiss_layout.hpp) on a device of 256 compute units, with data by the
same recipe and W, P from fit_missing_ref.  Each case names the route and the tile rows it claims; tests/cpp/xdiagmiss_layout.cpp
holds the header to that.  The last five straddle the batch tails of the streaming sweep's lane walk.

Self-checks of the yardstick:
  * its S equals scores_missing_ref; on the training X it equals the yardstick fit's T;
  * on the complete data Xc, with S = Xc R: Q, ssx and T2 equal the direct form F_c = Xc - S[:, :c] P[:, :c]^T;
  * float64 against longdouble stays below 1e-13 on S, Q (whole matrix and worst row), T2 and ssx.  Measured for the cases
    of test_missing_ref: S <= 2.7e-15, Q <= 4.2e-16, worst row of Q (worst_row below) <= 1.5e-15; over all cases T2 <= 7.8e-15, ssx <= 3.9e-15;
  * the smallest Q / row sum of squares is 1.1e-3 over those cases: the residual is not a cancellation of leading digits.
"""
import functools

import numpy as np
import pytest

from test_missing_ref import CASES as FIT_CASES
from test_missing_ref import TOL_F32, TOL_F64, _quot, case_data, case_yardstick, fit_missing_ref, rel, scores_missing_ref

TOL_LONGDOUBLE = 1e-13
NUM_CU = 256  # the device the claimed routes are for (MI355X)

RESIDENT, STREAM = "resident", "stream"

# name -> (N, K, A, missing fraction, storage, route, tile rows of the resident route (0: streaming))
CASES = {n: (c[0], c[1], c[3], c[4], c[5], STREAM, 0) for n, c in FIT_CASES.items()}
CASES["5000x40"] = (5000, 40, 3, 0.10, "f64", RESIDENT, 16)   # N >= 8 rows per CU; 5000 / 256 -> 16-row tiles
CASES.update({
    # route, N: at least XDM_RT_MIN = 8 rows per compute unit (2048 rows)
    "2047x24": (2047, 24, 2, 0.10, "f64", STREAM, 0),
    "2048x24": (2048, 24, 2, 0.10, "f64", RESIDENT, 8),
    "2048x24-f32": (2048, 24, 2, 0.10, "f32", RESIDENT, 8),      # fp32 storage on the resident route (streaming: 1031x130-f32)
    # route, K: a row of 8-row tiles fits XDM_TILE_BYTES = 64 KiB (K <= 1024)
    "2048x1024": (2048, 1024, 2, 0.10, "f64", RESIDENT, 8),
    "2048x1025": (2048, 1025, 2, 0.10, "f64", STREAM, 0),
    # tile rows from N: the power of two below N / 256, so that every CU has a tile (16 from 4096, 32 from 8192, 64 from 16384)
    "4095x12": (4095, 12, 2, 0.10, "f64", RESIDENT, 8),
    "4096x12": (4096, 12, 2, 0.10, "f64", RESIDENT, 16),
    "8191x12": (8191, 12, 2, 0.10, "f64", RESIDENT, 16),
    "8192x12": (8192, 12, 2, 0.10, "f32", RESIDENT, 32),
    "16383x12": (16383, 12, 2, 0.10, "f64", RESIDENT, 32),
    "16384x12": (16384, 12, 2, 0.10, "f64", RESIDENT, 64),
    # tile rows from K: rows x K x 8 bytes <= 64 KiB (64 rows up to K = 128, 32 up to 256, 16 up to 512, 8 up to 1024)
    "16384x128": (16384, 128, 2, 0.10, "f64", RESIDENT, 64),
    "16384x129": (16384, 129, 2, 0.10, "f64", RESIDENT, 32),
    "8192x256": (8192, 256, 2, 0.10, "f64", RESIDENT, 32),
    "8192x257": (8192, 257, 2, 0.10, "f64", RESIDENT, 16),
    "4096x512": (4096, 512, 2, 0.10, "f64", RESIDENT, 16),
    "4096x513": (4096, 513, 2, 0.10, "f64", RESIDENT, 8),
    # the batch tails of the streaming sweep's lane walk (miss_row_walk: 4 columns in flight per lane, then a column at a time):
    # the columns a lane owns in the LAST K range, by miss_row_split for 256 compute units and 16-byte packs.  Several column
    # lanes per row: 25 columns left for 8 lanes = 3 or 4 per lane, 65 left for 16 lanes = 4 or 5; one column lane (ranges of 9
    # columns): 3, 4 and 5 left.  N = 42, 601 and 603 are no multiples of the pack.  A = 7: the deflation chain takes its
    # components four (two for fp32 packs) at a time, so the sweeps for a = 0 .. 7 see every group count and every remainder.
    "40x601": (40, 601, 7, 0.10, "f64", STREAM, 0),
    "42x641-f32": (42, 641, 7, 0.10, "f32", STREAM, 0),
    "600x300": (600, 300, 7, 0.10, "f64", STREAM, 0),
    "601x301-f32": (601, 301, 7, 0.10, "f32", STREAM, 0),
    "603x302": (603, 302, 7, 0.10, "f64", STREAM, 0),
})
# name -> (fewest, most) columns a lane owns in the LAST K range of the streaming sweep, aligned layout, 256 compute units: what the
# comments above claim.  tests/test_xdiagmiss_layout.py holds miss_row_split to it (the fit's cases: TAILS of test_missing_ref).
TAILS = {"40x601": (3, 4), "42x641-f32": (4, 5), "600x300": (3, 3), "601x301-f32": (4, 4), "603x302": (5, 5)}
# The streaming route has the geometry of miss_row_kernel, whose thresholds the first twelve cases sit on: one K range (67x19, 5x12)
# against several (130x70, 33x20011), column lanes that meet in LDS (130x70) against none (257x33-m3), one row block (512x24)
# against two (513x24; fp32: 1031x130-f32).


def _seed(name):
    return [int(b) for b in name.encode()]


@functools.lru_cache(maxsize=None)
def xd_case(name):
    """(X with NaN, X complete, dict(W, P, R, T) of the yardstick fit): read-only; the cases of test_missing_ref as they are"""
    N, K, A, frac, st, _, _ = CASES[name]
    if name in FIT_CASES:
        X, _, Xc = case_data(name)
        y = case_yardstick(name)
        return X, Xc, {k: y[k] for k in "WPRT"}
    rng = np.random.default_rng(_seed(name))
    L = rng.standard_normal((N, 8))
    V = rng.standard_normal((K, 8))
    Xc = (L * np.linspace(3.0, 1.0, 8)) @ V.T + 0.05 * rng.standard_normal((N, K))
    Y = L[:, :3] @ rng.standard_normal((3, 1)) + 0.1 * rng.standard_normal((N, 1))
    Xc = Xc - Xc.mean(axis=0)
    Y = Y - Y.mean(axis=0)
    if st == "f32":
        Xc, Y = Xc.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64)
    X = Xc.copy()
    X[rng.random((N, K)) < frac] = np.nan
    X, Xc = np.asfortranarray(X), np.asfortranarray(Xc)
    y = fit_missing_ref(X, Y, A)
    m = {k: y[k] for k in "WPRT"}
    for a in (X, Xc, *m.values()):
        a.setflags(write=False)
    return X, Xc, m


def xdiag_missing_ref(X, W, P, tvar=None, dtype=np.float64):
    """dict(S, Q, T2, ssx, sst, nobs, q0) of the definition in arithmetic `dtype`"""
    X = np.asarray(X, dtype=dtype)
    obs = ~np.isnan(X)
    O = obs.astype(dtype)
    Xa = np.where(obs, X, 0).astype(dtype)
    N = X.shape[0]
    A = W.shape[1]
    S = np.zeros((N, A), dtype=dtype)
    Q = np.zeros((N, A), dtype=dtype)
    q0 = (Xa * Xa).sum(axis=1)
    for a in range(A):
        w = np.asarray(W[:, a], dtype=dtype)
        t = _quot(Xa @ w, O @ (w * w))
        Xa = Xa - np.outer(t, np.asarray(P[:, a], dtype=dtype)) * O
        S[:, a] = t
        Q[:, a] = (Xa * Xa).sum(axis=1)
    sst = (S * S).sum(axis=0)
    with np.errstate(all="ignore"):
        tv = sst / dtype(N - 1) if tvar is None else np.asarray(tvar, dtype=dtype)
        T2 = np.cumsum(S * S / tv, axis=1)
    ssx = np.concatenate([[q0.sum()], Q.sum(axis=0)])
    return dict(S=S, Q=Q, T2=T2, ssx=ssx, sst=sst, nobs=obs.sum(axis=1).astype(np.int64), q0=q0)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """the float64 yardstick on the case's training X (tvar from its own scores), computed once"""
    X, _, m = xd_case(name)
    y = xdiag_missing_ref(X, m["W"], m["P"])
    for v in y.values():
        v.setflags(write=False)
    return y


def worst_row(got, ref):
    """the worst relative error of a row of Q (rows of the reference that are zero: absolute)"""
    got = np.asarray(got, dtype=np.longdouble); ref = np.asarray(ref, dtype=np.longdouble)
    d = np.sqrt(((got - ref) ** 2).sum(axis=1))
    n = np.sqrt((ref ** 2).sum(axis=1))
    return float((d / np.where(n > 0, n, 1)).max())


def gpu_bar(name):
    return TOL_F32 if CASES[name][4] == "f32" else TOL_F64


# ---- self-checks of the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_scores_are_those_of_scores_missing_ref(name):
    X, _, m = xd_case(name)
    y = case_ref(name)
    assert np.array_equal(y["S"], scores_missing_ref(X, m["W"], m["P"]))
    e = rel(y["S"], m["T"])
    print(f"[xdiag-missing] {name}: S of the training X vs the fit's T {e:.2e}")
    assert e <= 1e-13
    assert np.array_equal(y["nobs"], (~np.isnan(X)).sum(axis=1)) and y["nobs"].dtype == np.int64


@pytest.mark.parametrize("name", list(CASES))
def test_complete_data_equals_the_direct_form(name):
    N, K, A, frac, st, _, _ = CASES[name]
    _, Xc, m = xd_case(name)
    y = xdiag_missing_ref(Xc, m["W"], m["P"])
    S = Xc @ m["R"]
    Q = np.stack([((Xc - S[:, :c] @ m["P"][:, :c].T) ** 2).sum(axis=1) for c in range(1, A + 1)], axis=1)
    sst = (S * S).sum(axis=0)
    T2 = np.cumsum(S * S / (sst / (N - 1)), axis=1)
    ssx = np.concatenate([[(Xc * Xc).sum()], Q.sum(axis=0)])
    e = dict(S=rel(y["S"], S), Q=rel(y["Q"], Q), T2=rel(y["T2"], T2), ssx=rel(y["ssx"], ssx))
    print(f"[xdiag-missing] {name} complete data vs the direct form: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-12, e
    assert (y["nobs"] == K).all()


@pytest.mark.parametrize("name", list(CASES))
def test_float64_against_longdouble(name):
    X, _, m = xd_case(name)
    y = case_ref(name)
    ld = xdiag_missing_ref(X, m["W"], m["P"], dtype=np.longdouble)
    e = dict(S=rel(y["S"], ld["S"]), Q=rel(y["Q"], ld["Q"]), Qrow=worst_row(y["Q"], ld["Q"]), T2=rel(y["T2"], ld["T2"]),
             ssx=rel(y["ssx"], ld["ssx"]))
    with np.errstate(all="ignore"):
        share = np.where(y["q0"] > 0, y["Q"].min(axis=1) / np.where(y["q0"] > 0, y["q0"], 1), 1.0).min()
    print(f"[xdiag-missing] {name} float64 vs longdouble: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"  smallest Q / row sum of squares {share:.2e}")
    assert max(e.values()) <= TOL_LONGDOUBLE, (name, e)
    # the residual keeps at least four of its sixteen digits' worth of the row: no cancellation of leading digits that the
    # device bar of 1e-10 could not carry
    assert share >= 1e-4, (name, share)


def test_rules_of_the_definition():
    X, _, m = xd_case("67x19")
    Xe = np.array(X)
    Xe[5, :] = np.nan   # a row without an observed cell
    Xe[:, 7] = np.nan   # a column without one
    y = xdiag_missing_ref(Xe, m["W"], m["P"])
    assert not y["S"][5].any() and not y["Q"][5].any() and not y["T2"][5].any() and y["nobs"][5] == 0
    assert all(np.isfinite(y[k]).all() for k in ("S", "Q", "T2", "ssx", "sst"))
    tv = np.array(y["sst"] / (X.shape[0] - 1))
    assert np.array_equal(xdiag_missing_ref(Xe, m["W"], m["P"], tvar=tv)["T2"], y["T2"])
    tv[1] = 0.0
    z = xdiag_missing_ref(Xe, m["W"], m["P"], tvar=tv)
    assert np.array_equal(z["T2"][:, 0], y["T2"][:, 0]) and not np.isfinite(z["T2"][np.arange(67) != 5, 1:]).any()
    for k in ("S", "Q", "ssx", "sst"):
        assert np.array_equal(z[k], y[k])


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_python_surface_is_exported():
    import pls_amd
    assert callable(getattr(pls_amd.Handle, "x_diagnostics_missing"))
    names = [p[0] for p in pls_amd._lib.PROTOTYPES]
    assert "pls_hip_x_diagnostics_missing" in names


def test_entry_point_rejects_the_null_handle():
    import pls_amd
    from pls_amd import _lib as L
    z = np.zeros(16)
    p = z.ctypes.data
    rc = pls_amd.lib().pls_hip_x_diagnostics_missing(None, p, 2, 2, 2, 1, p, p, None, L.F64, L.MEM_HOST, p, 2, p, 2, p, 2, p, p, p)
    assert rc == L.ERR_INVALID and not z.any()
