"""Variable-space diagnostics (pls_hip_var_diagnostics): the yardstick and what can be checked without a GPU.

The yardstick evaluates the definitions literally -- S = X R, F updated component by component, COLUMN sums of squares, VIP from
ssy_a = tau_a sum_m Q[m,a]^2 -- in numpy, once in fp64 and once in np.longdouble; nothing in it calls the library.  Every device
result (tests/test_gpu_vardiag.py) is measured against the longdouble evaluation with the worst-case bars below (u = 2^-52,
e[i,a] = sum_k |x_ik||r_ka| and g_c[i,k] = |x_ik| + sum_{a<c} e[i,a]|p_ka| as in tests/test_xdiag_ref.py, g_0 = |X|):

    ssxk[k,c]     (2K + 2A + N + 8) u sum_i g_c[i,k]^2
    sst[a]        total_bars of tests/test_xdiag_ref.py as it stands
    VIP[k,c-1]    relative: max_{a<c} bar(sst_a) / sst_a + (K + M + 2A + 16) u; with tt given the first term is 0

They hold for ANY summation order, so no correct kernel can exceed them; an off-by-one component or a dropped row misses them by
eight orders of magnitude.  The models come from the oracle's restatement of the reference's fit.
"""
import numpy as np
import pytest

from test_xdiag_ref import CPU_CASES, U, _case, total_bars, xdiag_bars, xdiag_yardstick


def vardiag_yardstick(X, W, R, P, Q, tt=None, dtype=np.float64):
    """dict(ssxk: K x (A+1), sst: A, VIP: K x A) by the definitions, in `dtype` arithmetic (np.float64 or np.longdouble);
    tt None: tau = this evaluation's sst.  X None (with tt): VIP alone."""
    W = np.asarray(W, dtype=dtype); Q = np.asarray(Q, dtype=dtype)
    K, A = W.shape
    out = {}
    if X is not None:
        X = np.asarray(X, dtype=dtype); R = np.asarray(R, dtype=dtype); P = np.asarray(P, dtype=dtype)
        N = X.shape[0]
        S = np.zeros((N, A), dtype=dtype)
        for k in range(K):                      # (longdouble has no BLAS: an explicit column loop, any K)
            S += X[:, k:k + 1] * R[k:k + 1, :]
        out["sst"] = (S * S).sum(0)
        F = X.copy()
        ssxk = np.zeros((K, A + 1), dtype=dtype)
        ssxk[:, 0] = (F * F).sum(0)
        for c in range(A):
            F -= S[:, c:c + 1] * P[:, c][None, :]
            ssxk[:, c + 1] = (F * F).sum(0)
        out["ssxk"] = ssxk
    tau = out["sst"] if tt is None else np.asarray(tt, dtype=dtype)
    ssy = tau * (Q * Q).sum(0)
    wn = (W * W).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["VIP"] = np.sqrt(dtype(K) * np.cumsum(ssy[None, :] * (W * W) / wn[None, :], axis=1) / np.cumsum(ssy)[None, :])
    return out


def vardiag_bars(X, R, P, ref, M, tt_given=False, u=U):
    """dict(ssxk: K x (A+1), sst: A, VIP: K x A, the last RELATIVE) of the module docstring; ref: the longdouble yardstick"""
    aX = np.abs(np.asarray(X, dtype=np.float64)); aR = np.abs(np.asarray(R, dtype=np.float64))
    aP = np.abs(np.asarray(P, dtype=np.float64))
    N, K = aX.shape
    A = aR.shape[1]
    xb = xdiag_bars(X, R, P, np.ones(A))
    e = xb["e"]
    g = aX.copy()
    env = np.zeros((K, A + 1))
    env[:, 0] = (g * g).sum(0)
    for c in range(A):
        g = g + e[:, c:c + 1] * aP[:, c][None, :]
        env[:, c + 1] = (g * g).sum(0)
    sst = np.asarray(ref["sst"], dtype=np.float64)
    _, bt = total_bars(xb, dict(ssx=np.zeros(A + 1), sst=sst), N, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.zeros(A) if tt_given else np.maximum.accumulate(bt / sst)
    vip = first[None, :] + (K + M + 2 * A + 16) * u + np.zeros((K, A))
    return dict(ssxk=(2 * K + 2 * A + N + 8) * u * env, sst=bt, VIP=vip, env=env)


def inside(got, ref, bars, what):
    """every entry of ssxk / sst (absolute) and VIP (relative) that `got` has within the bars of the longdouble `ref`;
    -> {name: worst error / bar}"""
    worst = {}
    for k in ("ssxk", "sst", "VIP"):
        if k not in got:
            continue
        g = np.asarray(got[k]); r = ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        err = np.abs(g.astype(np.longdouble) - r).astype(np.float64)
        bar = bars[k] * np.abs(np.asarray(r, dtype=np.float64)) if k == "VIP" else bars[k]
        fin = np.isfinite(np.asarray(r, dtype=np.float64))
        assert np.array_equal(np.isfinite(g), fin), (what, k, "finite where the definition is not, or the reverse")
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err[fin] == 0, 0.0, err[fin] / bar[fin])
        worst[k] = float(ratio.max()) if ratio.size else 0.0
        print(f"{what}: worst {k} error / bar {worst[k]:.3g}")
        assert np.all(err[fin] <= bar[fin]), (what, k, worst[k])
    return worst


@pytest.fixture(scope="module")
def evaluated(po, oracle):
    """the yardsticks of CPU_CASES, computed once"""
    out = {}
    for kind, N, K, M, A in CPU_CASES:
        X, Y, ref = _case(po, oracle, kind, N, K, M, A)
        y64 = vardiag_yardstick(X, ref["W"], ref["R"], ref["P"], ref["Q"])
        yld = vardiag_yardstick(X, ref["W"], ref["R"], ref["P"], ref["Q"], dtype=np.longdouble)
        out[(kind, N, K, M, A)] = (X, Y, ref, y64, yld)
    return out


@pytest.mark.parametrize("kind,N,K,M,A", CPU_CASES)
def test_fp64_yardstick_inside_the_bars_of_the_longdouble_one(evaluated, kind, N, K, M, A):
    X, Y, ref, y64, yld = evaluated[(kind, N, K, M, A)]
    bars = vardiag_bars(X, ref["R"], ref["P"], yld, Y.shape[1])
    inside(y64, yld, bars, f"{kind} {X.shape}")
    tt = (ref["T"] ** 2).sum(0)
    v64 = vardiag_yardstick(None, ref["W"], None, None, ref["Q"], tt=tt)
    vld = vardiag_yardstick(None, ref["W"], None, None, ref["Q"], tt=tt, dtype=np.longdouble)
    tb = vardiag_bars(X, ref["R"], ref["P"], yld, Y.shape[1], tt_given=True)
    inside(v64, vld, dict(VIP=tb["VIP"]), f"{kind} {X.shape} [tt given]")


@pytest.mark.parametrize("kind,N,K,M,A", CPU_CASES)
def test_columns_add_up_to_the_rows_and_match_the_nipals_deflation(po, evaluated, kind, N, K, M, A):
    """sum_k ssxk[k,c] = ssx[c] of xdiag_yardstick within its bar; ssxk[:, c] = the squared column norms of the matrix the NIPALS
    form deflates to, to 1e-10 ssxk[:, 0] (the project's parity bar between its two fit formulations)"""
    X, Y, ref, y64, yld = evaluated[(kind, N, K, M, A)]
    N, K = X.shape
    x64 = xdiag_yardstick(X, ref["R"], ref["P"])
    bx, _ = total_bars(xdiag_bars(X, ref["R"], ref["P"], x64["tvar"]), x64, N, K)
    assert np.all(np.abs(y64["ssxk"].sum(0) - x64["ssx"]) <= bx), kind
    Xd = np.array(X)
    for c in range(A):
        w = po.dominant_direction(Xd.T @ Y)
        t = Xd @ w
        Xd -= np.outer(t, Xd.T @ t / (t @ t))
        assert np.all(np.abs(y64["ssxk"][:, c + 1] - (Xd * Xd).sum(0)) <= 1e-10 * y64["ssxk"][:, 0]), (kind, c)


@pytest.mark.parametrize("kind,N,K,M,A", CPU_CASES)
def test_vip_squares_add_up_to_k(evaluated, kind, N, K, M, A):
    X, Y, ref, y64, yld = evaluated[(kind, N, K, M, A)]
    K = X.shape[1]
    assert np.all(np.abs((y64["VIP"] ** 2).sum(0) - K) <= (K + 16) * U * K), kind


def test_python_surface_is_exported():
    import pls_amd
    assert callable(getattr(pls_amd.Handle, "var_diagnostics"))
    assert callable(getattr(pls_amd.Model, "vip")) and callable(getattr(pls_amd.Model, "r2x_by_variable"))
    assert hasattr(pls_amd.lib(), "pls_hip_var_diagnostics")


def test_entry_point_refuses_the_null_handle():
    """the entry point rejects the NULL handle instead of dereferencing it, and writes nothing"""
    import pls_amd
    X = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(8, 3))
    R = np.asfortranarray(np.eye(3)[:, :2]); Q = np.ones((1, 2), order="F"); tt = np.ones(2)
    ssxk = np.zeros((3, 3), order="F"); VIP = np.zeros((3, 2), order="F"); sst = np.zeros(2)
    rc = pls_amd.lib().pls_hip_var_diagnostics(None, X.ctypes.data, 8, 8, 3, 1, 2, R.ctypes.data, R.ctypes.data, R.ctypes.data, Q.ctypes.data,
                                               tt.ctypes.data, 0, ssxk.ctypes.data, 3, VIP.ctypes.data, 3, sst.ctypes.data)
    assert rc == 1
    assert not (ssxk.any() or VIP.any() or sst.any())
