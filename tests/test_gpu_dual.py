"""The sample-space fit plan (PLS_HIP_ALGO_DUAL, pls_amd/csrc/plan_dual.hpp) on the GPU: the fit of a short, wide X from
G = X X^T in two sweeps over X.  Same outputs as every other plan, at the bars of tests/test_gpu_parity.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN, handle_with_env
from test_gpu_bounds import Guarded, Inputs, _fit_buffers, _fit_out, _place
from test_gpu_parity import check_against, oracle_ref, to_dev

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture
def dual(handle):
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    yield handle
    handle.set_option(pls_amd.OPT_ALGO, 0)


def _synth(handle, N, K, M, dt, seed=7):
    """device X, Y of the library's generator and their fp64 host images"""
    torch = _torch()
    tdt = torch.float64 if dt == "f64" else torch.float32
    X = handle.synth_x(0, N, K, seed, dtype=tdt); Y = handle.synth_y(0, N, M, seed, dtype=tdt)
    return X, Y, np.asfortranarray(X.cpu().numpy().astype(np.float64)), np.asfortranarray(Y.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("name,fx,fy", [("toy_A2", "toyX.csv", "toyY.csv"), ("nir_A10", "nir.csv", "octane.csv")])
def test_dual_reference_csv_golden(dual, oracle, po, name, fx, fy):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    A = int(g["A"])
    X = oracle.z_scores(po.read_csv(os.path.join(DATA, fx)))
    Y = oracle.z_scores(po.read_csv(os.path.join(DATA, fy)))
    out = dual.fit_device(to_dev(X), to_dev(Y), A)
    dual.synchronize()
    check_against(po, out, g, g["B"], g["T"], col_err=g["col_err"])
    assert np.allclose((out["T"].cpu().numpy() ** 2).sum(0), g["tt"], rtol=1e-9)


PARITY = [
    (1, 40, 1, 1, "f64"),          # a single row
    (17, 1003, 1, 5, "f64"),       # one ragged MFMA tile plus one row; K % 4 = 3
    (97, 1500, 1, 12, "f64"),
    (200, 5000, 3, 10, "f64"),
    (513, 4100, 2, 20, "f64"),     # one row past a block edge; 2A = 40
    (129, 70001, 1, 6, "f64"),     # many K splits, ragged last one
    (1031, 9000, 8, 8, "f32"),
    (2049, 3001, 4, 6, "f32"),
    (300, 2000, 32, 4, "f64"),     # the largest M
    (64, 300, 1, 40, "f64"),       # 2A = 80: more than one back-projection sweep
]


@pytest.mark.parametrize("N,K,M,A,dt", PARITY)
def test_dual_oracle_parity(dual, oracle, po, N, K, M, A, dt):
    X, Y, Xh, Yh = _synth(dual, N, K, M, dt)
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    out = dual.fit_device(X, Y, A); dual.synchronize()
    if dt == "f32":  # (the bars of test_wide_matrix_fp32)
        check_against(po, out, ref, Bref, ref["T"], tol_b=2e-5, tol_col=2e-5, col_err=cerr, tol_inv=1e-4)
    else:
        check_against(po, out, ref, Bref, ref["T"], col_err=cerr)


@pytest.mark.parametrize("N,K,M,A,dt", [(17, 1003, 1, 5, "f64"), (513, 4100, 2, 20, "f64"), (1031, 9000, 8, 8, "f32")])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
def test_dual_writes_exactly_its_outputs(dual, oracle, po, N, K, M, A, dt, layout):
    torch = _torch()
    tdt = torch.float64 if dt == "f64" else torch.float32
    _, _, Xh, Yh = _synth(dual, N, K, M, dt)
    gx, X = _place(Xh, tdt, layout)
    gy, Y = _place(Yh, tdt, layout)
    ins = Inputs(X=X, Y=Y)
    gt, gw = _fit_buffers(N, K, M, A, tdt, layout)
    dual.fit_device(X, Y, A, out=_fit_out(gt, gw)); dual.synchronize()
    gt.check(); gw.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    tol = dict(tol_b=2e-5, tol_col=2e-5, tol_inv=1e-4) if dt == "f32" else {}
    check_against(po, _fit_out(gt, gw), ref, Bref, ref["T"], col_err=cerr, **tol)


def test_dual_is_deterministic(dual):
    """the same fit twice on one handle and once on a fresh handle: equal bits in every output"""
    import pls_amd
    torch = _torch()
    X, Y, _, _ = _synth(dual, 513, 4100, 2, "f64")
    first = {k: v.clone() for k, v in dual.fit_device(X, Y, 20).items()}; dual.synchronize()
    again = dual.fit_device(X, Y, 20); dual.synchronize()
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        fresh = h.fit_device(X, Y, 20); h.synchronize()
        for k in "WPQRTB":
            assert torch.equal(first[k], again[k]), k
            assert torch.equal(first[k], fresh[k]), k


def test_dual_is_not_captured_by_opt_graph(dual):
    """OPT_GRAPH = 1 on a stream of its own: a DUAL fit simply runs, three times the same bits"""
    import pls_amd
    torch = _torch()
    X, Y, _, _ = _synth(dual, 200, 5000, 3, "f64")
    want = {k: v.clone() for k, v in dual.fit_device(X, Y, 10).items()}; dual.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side), handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        h.set_option(pls_amd.OPT_GRAPH, 1)
        for rep in range(3):
            out = h.fit_device(X, Y, 10); side.synchronize()
            for k in "WPQRTB":
                assert torch.equal(out[k], want[k]), (rep, k)


def test_dual_two_sweeps_over_x(oracle):
    """what the plan exists for: the traffic over X does not grow with A"""
    import pls_amd
    N, K = 200, 20000
    nk8 = N * K * 8
    with handle_with_env() as h:
        X = h.synth_x(0, N, K, 5); Y = h.synth_y(0, N, 1, 5)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        got = {}
        for A in (4, 16):
            h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
            h.timing()
            h.fit_device(X, Y, A)
            t = h.timing()
            assert t["launches"]["xb"] == 0 and t["launches"]["deflate"] == 0 and t["launches"]["fused"] == 0, t
            # the two sweeps and G: what does not depend on A.  (The operand term itself is (N + K) 2A 8 = 0.16 N K 8 at A = 16.)
            got[A] = t["bytes"]["xty"] - (N + K) * 2 * A * 8
            assert got[A] < 2.1 * nk8, (A, got[A])
            h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
            h.fit_device(X, Y, A)
            t = h.timing()
            assert sum(t["bytes"].values()) >= (1 + A) * nk8, (A, t)
        assert got[16] == got[4] == 2 * nk8 + N * N * 8, got
        h.set_option(pls_amd.OPT_PROFILE, 0)


def _refused(h, X, Y, A, K, M, N):
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    gt, gw = _fit_buffers(N, K, M, A, torch.float64, "aligned")
    with pytest.raises(pls_amd.PlsHipError) as e:
        h.fit_device(X, Y, A, out=_fit_out(gt, gw))
    assert e.value.code == L.ERR_UNSUPPORTED, e.value
    h.synchronize()
    gt.assert_untouched(); gw.assert_untouched()
    for i in range(len(gw)):
        gw.assert_prefilled(i)
    gt.assert_prefilled(0)


def test_dual_refusals(oracle, po):
    """N > 8192, M > 32 and a handle with a reducer: UNSUPPORTED, outputs untouched, the handle usable afterwards"""
    import pls_amd
    from pls_amd import _lib as L
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        X = h.synth_x(0, 8193, 16, 3); Y = h.synth_y(0, 8193, 1, 3)
        _refused(h, X, Y, 1, 16, 1, 8193)
        X = h.synth_x(0, 50, 60, 3); Y33 = h.synth_y(0, 50, 33, 3); Y = h.synth_y(0, 50, 2, 3)
        _refused(h, X, Y33, 2, 60, 33, 50)
        cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
        L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
        _refused(h, X, Y, 2, 60, 2, 50)
        h.clear_reducer()
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        ref, Bref, cerr = oracle_ref(oracle, po, np.asfortranarray(Xh), np.asfortranarray(Yh), 3)
        out = h.fit_device(X, Y, 3); h.synchronize()
        check_against(po, out, ref, Bref, ref["T"], col_err=cerr)


def test_dual_kernel_type2_ignores_the_option(handle):
    import pls_amd
    torch = _torch()
    X, Y, _, _ = _synth(handle, 300, 130, 2, "f64")
    handle.set_option(pls_amd.OPT_ALGO, 0)
    want = {k: v.clone() for k, v in handle.fit_device(X, Y, 6, method=pls_amd.KERNEL_TYPE2).items() if v is not None}
    handle.synchronize()
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    try:
        got = handle.fit_device(X, Y, 6, method=pls_amd.KERNEL_TYPE2); handle.synchronize()
    finally:
        handle.set_option(pls_amd.OPT_ALGO, 0)
    assert got["T"] is None
    for k in "WPQRB":
        assert torch.equal(got[k], want[k]), k


def test_dual_host_route(dual, oracle, po):
    torch = _torch()
    g = np.load(os.path.join(GOLDEN, "nir_A10.npz"))
    X = oracle.z_scores(po.read_csv(os.path.join(DATA, "nir.csv")))
    Y = oracle.z_scores(po.read_csv(os.path.join(DATA, "octane.csv")))
    out = dual.fit_host(X, Y, int(g["A"]))
    check_against(po, {k: torch.from_numpy(v) for k, v in out.items()}, g, g["B"], g["T"], col_err=g["col_err"])


def test_dual_group_route(oracle, po):
    """pls_hip_group_set_option + the group fit on a one-member group (a group of several members is row-sharded: refused)"""
    import pls_amd
    torch = _torch()
    gd = np.load(os.path.join(GOLDEN, "toy_A2.npz"))
    X = oracle.z_scores(po.read_csv(os.path.join(DATA, "toyX.csv")))
    Y = oracle.z_scores(po.read_csv(os.path.join(DATA, "toyY.csv")))
    g = pls_amd.Group([0])
    try:
        g.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        mx, my = g.upload(X), g.upload(Y)
        out = g.fit(mx, my, 2)
        res = {k: torch.from_numpy(out[k]) for k in "WPQRB"}
        res["T"] = torch.from_numpy(g.download(out["T"]))
        check_against(po, res, gd, gd["B"], gd["T"], col_err=gd["col_err"])
        g.set_option(pls_amd.OPT_ALGO, 0)
    finally:
        g.close()
    g2 = pls_amd.Group([0, 0])
    try:
        g2.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        mx, my = g2.upload(X), g2.upload(Y)
        with pytest.raises(pls_amd.PlsHipError) as e:
            g2.fit(mx, my, 2)
        assert e.value.code == 4, e.value
        g2.set_option(pls_amd.OPT_ALGO, 0)
        assert po.rel_fro(g2.fit(mx, my, 2)["B"], gd["B"]) < 1e-10
    finally:
        g2.close()
