"""Batched fits of many response sets on one X (pls_hip_fit_batch) and the response-permutation test: the parts that need
no GPU.

The yardstick of tests/test_gpu_fit_batch.py lives here: per problem the oracle's KERNEL_TYPE2 fit, tt[a] = r_a^T (X^T X) r_a
of the oracle's R, ssy = column sums of squares of Y_b, and from those the cumulative R^2 Y

    R2Y[m, c] = sum_{a <= c} Q[m, a]^2 tt[a] / ssy[m]

which equals 1 - SSE_c / ssy on column-centred data (the scores t_a = X r_a are orthogonal, tt[a] = t_a^T t_a).
"""
import os

import numpy as np
import pytest

from conftest import DATA, ROOT

NIR_SEED = 20261016
NIR_R2Y = (0.305427, 0.797936, 0.977319)  # cumulative explained variance of the octane model


def nir_z(po):
    X = po.colwise_z_scores(po.read_csv(os.path.join(DATA, "nir.csv")))
    Y = po.colwise_z_scores(po.read_csv(os.path.join(DATA, "octane.csv")))
    return np.asfortranarray(X), np.asfortranarray(Y)


def make_perms(n, nperm, seed):
    """the permutations Handle.permutation_test draws when none are given"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(nperm)]) if nperm else np.zeros((0, n), dtype=np.int64)


def stack_problems(Y, perms):
    """Ys (N x nprob*M): problem 0 is Y, problem b is Y[perms[b - 1]]"""
    return np.asfortranarray(np.concatenate([Y] + [Y[p] for p in perms], axis=1))


def batch_yardstick(oracle, X, Ys, M, A):
    """dict(R (nprob, K, A), Q (nprob, M, A), tt (nprob, A), B (nprob, K, M), ssy (nprob, M)) from one oracle fit per problem"""
    X = np.asfortranarray(X, dtype=np.float64); Ys = np.asfortranarray(Ys, dtype=np.float64)
    nprob = Ys.shape[1] // M
    XX = X.T @ X
    out = {k: [] for k in ("R", "Q", "tt", "B", "ssy", "W")}
    for b in range(nprob):
        Yb = np.asfortranarray(Ys[:, b * M:(b + 1) * M])
        ref = oracle.plsr(X, Yb, A, method=1)
        R, Q = np.asarray(ref["R"]), np.asarray(ref["Q"])
        out["R"].append(R); out["Q"].append(Q); out["W"].append(np.asarray(ref["W"]))
        out["tt"].append(np.einsum("ka,kj,ja->a", R, XX, R))
        out["B"].append(R @ Q.T)
        out["ssy"].append((Yb * Yb).sum(axis=0))
    return {k: np.stack(v) for k, v in out.items()}


def r2y_yardstick(Q, tt, ssy):
    Q, tt, ssy = (np.asarray(a, dtype=np.float64) for a in (Q, tt, ssy))
    out = np.zeros(Q.shape)
    for b in range(Q.shape[0]):
        for m in range(Q.shape[1]):
            ess = 0.0
            for a in range(Q.shape[2]):
                ess += Q[b, m, a] ** 2 * tt[b, a]
                out[b, m, a] = ess / ssy[b, m]
    return out


def test_r2y_by_components_against_the_loop():
    import pls_amd
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((5, 3, 7)); tt = rng.random((5, 7)) + 0.1; ssy = rng.random((5, 3)) + 1.0
    got = pls_amd.r2y_by_components(Q, tt, ssy)
    assert got.shape == (5, 3, 7)
    assert np.allclose(got, r2y_yardstick(Q, tt, ssy), rtol=1e-14, atol=0)
    torch = pytest.importorskip("torch")
    gt = pls_amd.r2y_by_components(torch.from_numpy(Q), torch.from_numpy(tt), torch.from_numpy(ssy))
    assert np.allclose(gt.numpy(), got, rtol=1e-14, atol=0)


def test_permutation_pvalues_counts():
    import pls_amd
    real = np.array([[0.5, 0.9]])
    perm = np.array([[[0.1, 0.95]], [[0.5, 0.2]], [[0.7, 0.9]]])   # >= counts ties
    p = pls_amd.permutation_pvalues(real, perm)
    assert p.shape == (1, 2)
    assert np.array_equal(p, np.array([[(1 + 2) / 4, (1 + 2) / 4]]))
    assert np.array_equal(pls_amd.permutation_pvalues(real, perm[:0]), np.ones((1, 2)))


@pytest.mark.parametrize("N,K,M,A", [(1000, 64, 1, 10), (2048, 128, 4, 6), (1000, 7, 2, 3)])
def test_r2y_identity_against_sse(po, oracle, N, K, M, A):
    """ESS / ssy from (Q, tt, ssy) equals 1 - SSE / ssy on column-centred data"""
    import pls_amd
    X = po.synth_x(0, N, K); X = np.asfortranarray(X - X.mean(axis=0))
    Y = po.synth_y(0, N, M); Y = np.asfortranarray(Y - Y.mean(axis=0))
    y = batch_yardstick(oracle, X, stack_problems(Y, make_perms(N, 2, 1)), M, A)
    r2 = pls_amd.r2y_by_components(y["Q"], y["tt"], y["ssy"])
    for b in range(3):
        Yb = Y if b == 0 else Y[make_perms(N, 2, 1)[b - 1]]
        for c in range(A):
            sse = ((Yb - X @ (y["R"][b][:, :c + 1] @ y["Q"][b][:, :c + 1].T)) ** 2).sum(axis=0)
            assert np.allclose(r2[b, :, c], 1.0 - sse / y["ssy"][b], rtol=0, atol=1e-12)


def nir_figures(po, oracle, nperm=199):
    X, Y = nir_z(po)
    perms = make_perms(X.shape[0], nperm, NIR_SEED)
    y = batch_yardstick(oracle, X, stack_problems(Y, perms), 1, 3)
    return X, Y, perms, y


def test_nir_permutation_figures(po, oracle):
    """the octane model, z-scored, A = 3, 199 permutations: R^2 Y as SURVEY.md Appendix B lists it, p = 1/200 everywhere,
    and a gap between the real model and the best permutation far beyond any rounding"""
    import pls_amd
    X, Y, perms, y = nir_figures(po, oracle)
    r2 = pls_amd.r2y_by_components(y["Q"], y["tt"], y["ssy"])
    assert np.allclose(r2[0, 0], NIR_R2Y, rtol=0, atol=5e-7)
    p = pls_amd.permutation_pvalues(r2[0], r2[1:])
    assert np.array_equal(p, np.full((1, 3), 1.0 / 200.0))
    gap = np.abs(r2[1:] - r2[0][None]).min()
    print(f"smallest |r2_perm - r2_real| = {gap:.4f}")
    assert abs(gap - 0.161) < 1e-3  # (p does not depend on rounding)


def test_python_surface_is_exported():
    import pls_amd
    for cls in (pls_amd.Handle, pls_amd.Group):
        assert callable(getattr(cls, "fit_batch"))
    assert callable(pls_amd.Handle.permutation_test) and callable(pls_amd.Model.permutation_test)
    assert callable(pls_amd.r2y_by_components) and callable(pls_amd.permutation_pvalues)
    assert "r2y_by_components" in pls_amd.__all__ and "permutation_pvalues" in pls_amd.__all__


def test_entry_points_reject_the_null_handle():
    """both new entry points return PLS_HIP_ERR_INVALID for a NULL handle without dereferencing it, and write nothing"""
    import pls_amd
    X = np.asfortranarray(np.arange(24, dtype=np.float64).reshape(8, 3))
    Ys = np.asfortranarray(np.arange(16, dtype=np.float64).reshape(8, 2))
    R = np.zeros((2, 2, 3)); Q = np.zeros((2, 2, 1)); tt = np.zeros((2, 2)); B = np.zeros((2, 1, 3)); ssy = np.zeros((2, 1))
    p = lambda a: a.ctypes.data
    rc = pls_amd.lib().pls_hip_fit_batch(None, p(X), 8, p(Ys), 8, 8, 3, 1, 2, 2, 0, 0, p(R), p(Q), p(tt), p(B), p(ssy))
    assert rc == 1
    assert not (R.any() or Q.any() or tt.any() or B.any() or ssy.any())
    rc = pls_amd.lib().pls_hip_group_fit_batch(None, None, None, 1, 2, p(R), p(Q), p(tt), p(B), p(ssy))
    assert rc == 1
    assert not (R.any() or Q.any() or tt.any() or B.any() or ssy.any())


def test_cpp_program_is_built():
    """tests/cpp/fit_batch (PLS::Model::permutation_test against one Model per problem) is built by the host Makefile"""
    exe = os.path.join(ROOT, "tests", "cpp", "fit_batch")
    assert os.path.exists(exe) and os.access(exe, os.X_OK), "run the build first (pls_amd/host/Makefile)"
