"""Cross-validation folds of X with missing values (pls_hip_cv_folds_missing): the parts that need no GPU.

cv_missing_ref is the DEFINITION of include/pls_hip.h: per fold, fit_missing_ref on the training rows, scores_missing_ref on the
held-out rows, E_c = Y_test - S[:, :c] Q[:, :c]^T.  cv_missing_masked restates what the device does instead -- the algorithm on
all rows with the 0/1 training mask entering through N-sized vectors -- and must equal the definition to 1e-13 (relative
Frobenius on E).  tests/test_gpu_missing_cv.py takes its cases, its yardstick and its bars from here.

Cases: those of tests/test_missing_ref.py (data, A, storage), folds idx = default_rng(7).permutation(N)[:6 ts].reshape(6, ts) with
ts = min(N // 6, 9); "5x12" is leave-one-out.  Per case the yardstick E must be finite and every column must keep at least two
observed training cells in every fold.  M > 1: E at tol = 1e-10 against tol = 1e-14 (max_iters 2000), worst component column, is
the SENSITIVITY (<= 1e-9) that the GPU bar max(1e-10, 10 x sensitivity) rests on, as gpu_bar of test_missing_ref does for the fit.
The slab of a round (pls_amd/csrc/miss_layout.hpp) is laid out by tests/cpp/missing_cv_layout.cpp under ASan + UBSan."""
import functools
import os
import subprocess

import numpy as np
import pytest

from test_missing_ref import CASES, TOL_F32, TOL_F64, TOL_SENSITIVITY, _quot, case_data, fit_missing_ref, rel, scores_missing_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_MASKED = 1e-13
CV_CASES = ("67x19", "130x70", "257x33-m3", "40x300", "40x300-m2", "5x12", "512x24", "513x24", "1031x130-f32", "5000x40", "33x20011")
CV_MULTI = tuple(n for n in CV_CASES if CASES[n][2] > 1)


def case_folds(name):
    """(num_folds, test_size) int64 indices of the held-out rows of a case"""
    N = CASES[name][0]
    if name == "5x12":
        return np.arange(N, dtype=np.int64)[:, None]
    ts = min(N // 6, 9)
    return np.random.default_rng(7).permutation(N)[:6 * ts].reshape(6, ts).astype(np.int64)


def cv_missing_ref(X, Y, A, idx, tol=1e-10, max_iters=500):
    """the definition: (E (M, nobs, A), iters (num_folds, A)) from one fit_missing_ref + scores_missing_ref per fold"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    nf, ts = idx.shape
    M = Y.shape[1]
    E = np.zeros((M, nf * ts, A))
    iters = np.zeros((nf, A), dtype=np.int64)
    for f in range(nf):
        train = np.ones(X.shape[0], dtype=bool)
        train[idx[f]] = False
        fit = fit_missing_ref(X[train], Y[train], A, tol=tol, max_iters=max_iters)
        S = scores_missing_ref(X[idx[f]], fit["W"], fit["P"])
        for c in range(1, A + 1):
            E[:, f * ts:(f + 1) * ts, c - 1] = (Y[idx[f]] - S[:, :c] @ fit["Q"][:, :c].T).T
        iters[f] = fit["iters"]
    return E, iters


def cv_missing_masked(X, Y, A, idx, tol=1e-10, max_iters=500):
    """the masked form: no rows gathered, m enters through u~ = m o u and t~ = m o t; every row is deflated with its own t"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    N, K = X.shape
    nf, ts = idx.shape
    M = Y.shape[1]
    obs = ~np.isnan(X)
    O = obs.astype(np.float64)
    E = np.zeros((M, nf * ts, A))
    iters = np.zeros((nf, A), dtype=np.int64)
    for f in range(nf):
        m = np.ones(N)
        m[idx[f]] = 0.0
        Xa = np.where(obs, X, 0.0)
        Ya = Y.copy()
        for a in range(A):
            j = int(np.argmax((m[:, None] * Ya * Ya).sum(axis=0))) if M > 1 else 0
            u = m * Ya[:, j]
            t_prev = None
            it = 0
            while True:
                it += 1
                w = _quot(Xa.T @ u, O.T @ (u * u))
                w = _quot(w, np.sqrt(w @ w))
                t = _quot(Xa @ w, O @ (w * w))
                tm = m * t
                tt = tm @ tm
                q = _quot(Ya.T @ tm, tt)
                if M == 1 or (it >= 2 and (tm - t_prev) @ (tm - t_prev) <= tol * tol * tt) or it >= max_iters:
                    break
                t_prev = tm
                u = m * _quot(Ya @ q, q @ q)
            p = _quot(Xa.T @ tm, O.T @ (tm * tm))
            Xa = Xa - np.outer(t, p) * O
            Ya = Ya - np.outer(t, q)
            E[:, f * ts:(f + 1) * ts, a] = Ya[idx[f]].T
            iters[f, a] = it
    return E, iters


def column_err(got, ref):
    """worst relative Frobenius error over the component columns E[:, :, a]"""
    return max(rel(got[:, :, a], ref[:, :, a]) for a in range(ref.shape[2]))


@functools.lru_cache(maxsize=None)
def cv_yardstick(name):
    """(E, iters) of the definition on the case's data and folds, computed once, read-only"""
    X, Y, _ = case_data(name)
    E, iters = cv_missing_ref(X, Y, CASES[name][3], case_folds(name))
    E.setflags(write=False); iters.setflags(write=False)
    return E, iters


@functools.lru_cache(maxsize=None)
def cv_sensitivity(name):
    """M > 1: E stopped at tol = 1e-10 against tol = 1e-14 (max_iters 2000), the worst component column"""
    if CASES[name][2] == 1:
        return 0.0
    X, Y, _ = case_data(name)
    tight, _ = cv_missing_ref(X, Y, CASES[name][3], case_folds(name), tol=1e-14, max_iters=2000)
    return column_err(cv_yardstick(name)[0], tight)


def cv_gpu_bar(name):
    N, K, M, A, frac, dt = CASES[name]
    if dt == "f32":
        return TOL_F32
    return TOL_F64 if M == 1 else max(TOL_F64, 10.0 * cv_sensitivity(name))


# ---- the yardstick and the masked form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CV_CASES)
def test_conditions_of_a_case(name):
    X, _, _ = case_data(name)
    idx = case_folds(name)
    E, iters = cv_yardstick(name)
    assert np.isfinite(E).all()
    obs = ~np.isnan(X)
    least = min(int((obs.sum(axis=0) - obs[idx[f]].sum(axis=0)).min()) for f in range(idx.shape[0]))
    print(f"[missing-cv] {name}: folds {idx.shape}, fewest observed training cells of a column {least}, iters up to {iters.max()}")
    assert least >= 2
    assert all(len(set(idx[f])) == idx.shape[1] for f in range(idx.shape[0]))
    if CASES[name][2] == 1:
        assert (iters == 1).all()


@pytest.mark.parametrize("name", CV_CASES)
def test_masked_form_equals_the_definition(name):
    X, Y, _ = case_data(name)
    E, iters = cv_yardstick(name)
    Em, im = cv_missing_masked(X, Y, CASES[name][3], case_folds(name))
    e = rel(Em, E)
    print(f"[missing-cv] {name}: masked form vs per-fold refit {e:.2e}  iters {im.max()} / {iters.max()}")
    assert e <= TOL_MASKED, (name, e)
    assert (np.abs(im - iters) <= 1).all()


@pytest.mark.parametrize("name", CV_MULTI)
def test_sensitivity_to_the_stopping_rule(name):
    s = cv_sensitivity(name)
    print(f"[missing-cv] {name} sensitivity of E (tol 1e-10 vs 1e-14): {s:.2e}  gpu bar {cv_gpu_bar(name):.2e}")
    assert s <= TOL_SENSITIVITY, (name, s)


# ---- the slab of a round ----------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(5, 12, 1, 2, 1, 5), (257, 33, 3, 4, 9, 6), (33, 20011, 1, 3, 5, 2)]  # (N, K, M, A, ts, nround)
NUM_CU = 256
FIELDS = ("work", "Ya", "mask", "u", "t", "tm", "tprev", "w", "p", "q", "colpart", "sspart", "tpart", "ypart", "yss", "qq", "words")


def _geom(N, K, es, cu):
    """miss_geom restated: (ldw, G, nbK, S, GY)"""
    FV, WG, KC = 16 // es, 256, 8
    cdiv = lambda a, b: -(-a // b)
    ldw = cdiv(N, FV) * FV
    nch = cdiv(N, WG)
    G = min(max(1, (5 * cu) // cdiv(K, KC)), nch, 65535)
    nv = cdiv(N, FV)
    lrl = 0
    while (1 << lrl) < WG and (1 << lrl) < nv:
        lrl += 1
    RL, CL = 1 << lrl, WG >> lrl
    S = min(max(1, (4 * cu) // cdiv(nv, RL)), max(1, K // (8 * CL)), 65535)
    kper = cdiv(cdiv(K, S), CL) * CL
    return ldw, G, cdiv(K, WG), cdiv(K, kper), min(nch, 2 * cu)


def field_bytes(N, K, M, A, es, cu):
    """the closed form: bytes of every field of a fold, each rounded up to 16"""
    ldw, G, nbK, S, GY = _geom(N, K, es, cu)
    raw = dict(work=ldw * K * es, Ya=N * M * 8, mask=N * 8, u=N * 8, t=N * 8, tm=N * 8, tprev=N * 8, w=K * 8, p=K * 8, q=M * A * 8,
               colpart=G * K * 16, sspart=nbK * 8, tpart=S * N * 16 if S > 1 else 0, ypart=GY * (M + 2) * 8, yss=GY * M * 8, qq=16,
               words=16)
    return [(n, -(-raw[n] // 16) * 16) for n in FIELDS]


@pytest.fixture(scope="module")
def slabs(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("missing_cv_layout") / "missing_cv_layout")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "missing_cv_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = [c + (es, NUM_CU) for c in LAYOUT_CASES for es in (8, 4)]
    p = subprocess.run([exe], input="".join(" ".join(map(str, c)) + "\n" for c in runs), capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = [l.split() for l in p.stdout.splitlines()]
    assert len(lines) == len(runs)
    return {c: (int(l[0]), [(f.split(":")[0], int(f.split(":")[1]), int(f.split(":")[2])) for f in l[1:]]) for c, l in zip(runs, lines)}


@pytest.mark.parametrize("es", [8, 4])
@pytest.mark.parametrize("case", LAYOUT_CASES)
def test_slab_of_a_fold_is_the_closed_form(slabs, case, es):
    N, K, M, A, ts, nround = case
    per_fold, got = slabs[case + (es, NUM_CU)]
    want = field_bytes(N, K, M, A, es, NUM_CU)
    assert [n for n, _, _ in got] == [n for n, _ in want]
    at = 0  # every field begins where the one before it ends, on a 16-byte boundary: no two overlap
    for (name, off, size), (_, closed) in zip(got, want):
        assert off == at and off % 16 == 0 and size == closed, (name, off, at, size, closed)
        at += size
    assert at == per_fold == sum(b for _, b in want)
    if (N, K) == (33, 20011):
        assert dict(want)["tpart"] > 0   # the K-split row sweep has partials ...
    if (N, K) == (5, 12):
        assert dict(want)["tpart"] == 0  # ... a single K range has none


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
def test_python_surface_is_exported():
    import pls_amd
    from pls_amd import _lib as L
    assert callable(pls_amd.Handle.cv_folds_missing)
    assert any(n == "pls_hip_cv_folds_missing" for n, _, _ in L.PROTOTYPES)
    for n in ("cv_LOO", "cv_LSO", "cv_NEW_DATA", "plsr_missing"):
        assert callable(getattr(pls_amd.Model, n))


def test_entry_point_rejects_the_null_handle():
    """a NULL handle is rejected without being dereferenced, and nothing is written"""
    import pls_amd
    from pls_amd import _lib as L
    z = np.zeros(16)
    idx = np.zeros(1, dtype=np.int64)
    p = z.ctypes.data
    rc = pls_amd.lib().pls_hip_cv_folds_missing(None, p, 2, p, 2, 2, 2, 1, 1, idx.ctypes.data, 1, 1, L.F64, L.MEM_HOST, p, p)
    assert rc == L.ERR_INVALID
    assert not z.any()
