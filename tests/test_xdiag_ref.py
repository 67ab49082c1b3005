"""X-space diagnostics (pls_hip_x_diagnostics): the yardstick and what can be checked without a GPU.

The yardstick evaluates the definitions literally -- S = X R, F updated component by component, row sums of squares --
in numpy, once in fp64 and once in np.longdouble; nothing in it calls the library.  Every device result (tests/
test_gpu_xdiag.py) is measured against the longdouble evaluation with the worst-case bars below (u = 2^-52,
e[i,a] = sum_k |x_ik||r_ka|, g_c[i,k] = |x_ik| + sum_{a<c} e[i,a]|p_ka|):

    S[i,a]        (K + 2) u e[i,a]
    Qres[i,c-1]   (3K + 2A + 8) u ENVQ,  ENVQ = sum_k g_c[i,k]^2
    T2[i,c-1]     (2K + 2A + 8) u ENVT,  ENVT = sum_{a<c} e[i,a]^2 / tvar[a]
    ssx[c], c>=1  sum_i bar(Qres[i,c-1]) + N u ssx[c]
    ssx[0]        (K + N) u ssx[0]
    sst[a]        sum_i 2 (K + 2) u e[i,a]^2 + N u sst[a]

They hold for ANY summation order, so no correct kernel can exceed them; a wrong column, a missing component or a dropped
row misses them by ten orders of magnitude.  The models come from the oracle's restatement of the reference's fit.
"""
import os

import numpy as np
import pytest

from conftest import DATA

U = 2.0 ** -52


def xdiag_yardstick(X, R, P, tvar=None, n_total=None, dtype=np.float64):
    """dict(S, Q, T2, ssx, sst, tvar) by the definitions, in `dtype` arithmetic (np.float64 or np.longdouble)"""
    X = np.asarray(X, dtype=dtype); R = np.asarray(R, dtype=dtype); P = np.asarray(P, dtype=dtype)
    N, K = X.shape
    A = R.shape[1]
    S = np.zeros((N, A), dtype=dtype)
    for k in range(K):                      # (longdouble has no BLAS: an explicit column loop, any K)
        S += X[:, k:k + 1] * R[k:k + 1, :]
    sst = (S * S).sum(0)
    if tvar is None:
        tvar = sst / dtype((n_total or N) - 1)
    tvar = np.asarray(tvar, dtype=dtype)
    F = X.copy()
    Q = np.zeros((N, A), dtype=dtype)
    ssx = np.zeros(A + 1, dtype=dtype)
    ssx[0] = (F * F).sum()
    for c in range(A):
        F -= S[:, c:c + 1] * P[:, c][None, :]
        Q[:, c] = (F * F).sum(1)
        ssx[c + 1] = Q[:, c].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        T2 = np.cumsum(S * S / tvar[None, :], axis=1)
    return dict(S=S, Q=Q, T2=T2, ssx=ssx, sst=sst, tvar=tvar)


def xdiag_bars(X, R, P, tvar, u=U):
    """the bars of the module docstring, plus the envelopes they are made of (for figures in units of u * envelope)"""
    X = np.abs(np.asarray(X, dtype=np.float64)); aR = np.abs(np.asarray(R, dtype=np.float64))
    aP = np.abs(np.asarray(P, dtype=np.float64))
    tvar = np.asarray(tvar, dtype=np.float64)
    N, K = X.shape
    A = aR.shape[1]
    e = X @ aR                                         # N x A
    g = X.copy()
    envq = np.zeros((N, A))
    for c in range(A):
        g = g + e[:, c:c + 1] * aP[:, c][None, :]
        envq[:, c] = (g * g).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        envt = np.cumsum(e * e / np.abs(tvar)[None, :], axis=1)
    return dict(e=e, envq=envq, envt=envt,
                S=(K + 2) * u * e,
                Q=(3 * K + 2 * A + 8) * u * envq,
                T2=(2 * K + 2 * A + 8) * u * envt)


def total_bars(bars, ref, N, K, u=U):
    """bars of ssx (A + 1) and sst (A) from the rows' bars and the longdouble totals `ref`"""
    ssx = np.asarray(ref["ssx"], dtype=np.float64); sst = np.asarray(ref["sst"], dtype=np.float64)
    bx = np.empty_like(ssx)
    bx[0] = (K + N) * U * ssx[0]
    bx[1:] = bars["Q"].sum(0) + N * u * ssx[1:]
    bt = (2 * (K + 2) * U * bars["e"] ** 2).sum(0) + N * U * sst
    return bx, bt


def nir_z(po):
    X = po.colwise_z_scores(po.read_csv(os.path.join(DATA, "nir.csv")))
    Y = po.colwise_z_scores(po.read_csv(os.path.join(DATA, "octane.csv")))
    return np.asfortranarray(X), np.asfortranarray(Y)


CPU_CASES = [("nir", None, None, None, 10), ("synth", 4097, 513, 1, 12), ("synth", 3000, 64, 4, 20),
             ("synth", 1000, 7, 4, 7), ("synth", 9, 7, 1, 3)]


def _case(po, oracle, kind, N, K, M, A):
    if kind == "nir":
        X, Y = nir_z(po)
    else:
        X, Y = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    return X, Y, oracle.plsr(X, Y, A)


@pytest.mark.parametrize("kind,N,K,M,A", CPU_CASES)
def test_yardstick_against_the_oracle(po, oracle, kind, N, K, M, A):
    """Q residuals of the training data = squared row norms of the matrix the NIPALS form deflates to (1e-10 ||x_i||^2, the
    project's parity bar between its two fit formulations); sum_i T2[i, c-1] = c (N - 1); ssx does not increase; the fp64
    yardstick sits inside the bars of the longdouble one."""
    X, Y, ref = _case(po, oracle, kind, N, K, M, A)
    N, K = X.shape
    y64 = xdiag_yardstick(X, ref["R"], ref["P"])
    yld = xdiag_yardstick(X, ref["R"], ref["P"], dtype=np.longdouble)
    # the NIPALS deflation, component by component
    Xd = np.array(X)
    x2 = (X * X).sum(1)
    for c in range(A):
        w = po.dominant_direction(Xd.T @ Y)
        t = Xd @ w
        Xd -= np.outer(t, Xd.T @ t / (t @ t))
        assert np.all(np.abs(y64["Q"][:, c] - (Xd * Xd).sum(1)) <= 1e-10 * x2), (kind, c)
        assert abs(y64["T2"][:, c].sum() - (c + 1) * (N - 1)) <= 1e-10 * (c + 1) * N
    assert np.all(np.diff(y64["ssx"]) <= 0)
    bars = xdiag_bars(X, ref["R"], ref["P"], y64["tvar"])
    for k in ("S", "Q", "T2"):
        err = np.abs(y64[k] - yld[k]).astype(np.float64)
        assert np.all(err <= bars[k]), (kind, k, float((err / bars[k]).max()))
    bx, bt = total_bars(bars, yld, N, K)
    assert np.all(np.abs(y64["ssx"] - yld["ssx"]).astype(np.float64) <= bx)
    assert np.all(np.abs(y64["sst"] - yld["sst"]).astype(np.float64) <= bt)


def test_r2x_of_the_nir_model(po, oracle):
    """the figures the feature request quotes for the 10-component model of the NIR data"""
    X, Y = nir_z(po)
    ref = oracle.plsr(X, Y, 10)
    y = xdiag_yardstick(X, ref["R"], ref["P"])
    r2x = 1.0 - y["ssx"][1:] / y["ssx"][0]
    assert np.allclose(r2x, [0.650, 0.835, 0.937, 0.963, 0.982, 0.986, 0.988, 0.989, 0.990, 0.992], atol=6e-4)


def test_entry_point_has_no_cpu_path():
    """without a device no handle can be made (PLS_HIP_ERR_DEVICE); the entry points themselves reject the NULL handle
    instead of dereferencing it, and write nothing"""
    import torch
    import pls_amd
    X = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(8, 3))
    R = np.asfortranarray(np.eye(3)[:, :2]); P = R.copy()
    if not torch.cuda.is_available():
        with pytest.raises(pls_amd.PlsHipError) as e:
            pls_amd.Handle().x_diagnostics(X, R, P)
        assert e.value.code == 2  # PLS_HIP_ERR_DEVICE
    Q = np.zeros((8, 2), order="F"); T2 = np.zeros((8, 2), order="F"); S = np.zeros((8, 2), order="F")
    ssx = np.zeros(3); sst = np.zeros(2)
    rc = pls_amd.lib().pls_hip_x_diagnostics(None, X.ctypes.data, 8, 8, 8, 3, 2, R.ctypes.data, P.ctypes.data, None, 0, 0,
                                             Q.ctypes.data, 8, T2.ctypes.data, 8, S.ctypes.data, 8, ssx.ctypes.data,
                                             sst.ctypes.data)
    assert rc == 1
    assert not (Q.any() or T2.any() or S.any() or ssx.any() or sst.any())
    rc = pls_amd.lib().pls_hip_group_x_diagnostics(None, None, 2, R.ctypes.data, P.ctypes.data, None, None, None, None,
                                                   ssx.ctypes.data, sst.ctypes.data)
    assert rc == 1 and not (ssx.any() or sst.any())


def test_python_surface_is_exported():
    import pls_amd
    for cls in (pls_amd.Handle, pls_amd.Model, pls_amd.Group):
        assert callable(getattr(cls, "x_diagnostics"))


def test_cpp_program_is_built():
    """tests/cpp/x_diagnostics (PLS::Model::x_diagnostics against its own definition) is built by the host Makefile"""
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "x_diagnostics")
    assert os.path.exists(exe) and os.access(exe, os.X_OK), "run the build first (pls_amd/host/Makefile)"
