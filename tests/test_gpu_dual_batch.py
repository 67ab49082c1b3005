"""pls_hip_fit_batch under the sample-space plan (PLS_HIP_ALGO_DUAL, pls_amd/csrc/plan_dual_batch.hpp) on the GPU: every problem
from one G = X X^T, one sweep over X for Q, tt and ssy whatever A and the number of problems are, R and B as one wide product
X^T [...] per round.  Cases, yardstick (one oracle fit per problem) and bars are those of tests/test_dual_batch_ref.py."""
import contextlib
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT, handle_with_env
from test_dual_batch_ref import CASES, case_data, case_yardstick, check
from test_fit_batch_ref import NIR_R2Y, NIR_SEED, nir_z
from test_gpu_bounds import Guarded, Inputs, _place

pytestmark = pytest.mark.gpu

NAMES = ("R", "Q", "tt", "B", "ssy")


def _torch():
    import torch
    return torch


@pytest.fixture
def dual(handle):
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    yield handle
    handle.set_option(pls_amd.OPT_ALGO, 0)


@contextlib.contextmanager
def dual_handle(**env):
    """a fresh handle under the environment switches given, with the option set"""
    import pls_amd
    with handle_with_env(**env) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
        yield h


def _dev(a, dt="f64"):
    import pls_amd
    torch = _torch()
    t = torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases are read-only)
    return pls_amd.as_colmajor(t.to(torch.float32) if dt == "f32" else t)


def _as_np(out):
    torch = _torch()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64) for k, v in out.items()}


def run(h, name, mem="device", want=NAMES):
    N, K, M, A, nprob, dt, _ = CASES[name]
    X, Ys = case_data(name)
    if mem == "device":
        out = h.fit_batch(_dev(X, dt), _dev(Ys, dt), M, A, want=want)
        h.synchronize()
    else:
        ndt = np.float32 if dt == "f32" else np.float64
        out = h.fit_batch(np.asfortranarray(X.astype(ndt)), np.asfortranarray(Ys.astype(ndt)), M, A, want=want)
    return _as_np(out)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a) and set(a) == set(b)


# ---- 1. the table, both memory kinds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_dual_batch_parity(dual, name):
    """device call and host-memory call against one oracle fit per problem; the host call within 1e-12 of the device call"""
    N, K, M, A, nprob, dt, columns = CASES[name]
    y = case_yardstick(name)
    got = run(dual, name)
    assert got["R"].shape == (nprob, K, A) and got["Q"].shape == (nprob, M, A) and got["B"].shape == (nprob, K, M)
    assert got["tt"].shape == (nprob, A) and got["ssy"].shape == (nprob, M)
    host = run(dual, name, "host")
    check(got, y, name + " device", columns)
    check(host, y, name + " host", columns)
    for k in NAMES:
        assert np.abs(host[k] - got[k]).max() <= 1e-12 * max(np.abs(got[k]).max(), 1.0), k


# ---- 2. K beyond the other routes -----------------------------------------------------------------------------------------------
def test_dual_batch_k_beyond_the_other_routes(dual, handle):
    """129 x 40001: PLS_HIP_OK under the option (without it: PLS_HIP_ERR_UNSUPPORTED, K > 32768), at the bars"""
    import pls_amd
    from pls_amd import _lib as L
    from pls_amd.model import _ld
    torch = _torch()
    name = "129x40001"
    N, K, M, A, nprob, dt, _ = CASES[name]
    X, Ys = case_data(name)
    Xd, Yd = _dev(X), _dev(Ys)
    out = {k: torch.zeros(n, dtype=torch.float64, device="cuda") for k, n in
           dict(R=nprob * K * A, Q=nprob * M * A, tt=nprob * A, B=nprob * K * M, ssy=nprob * M).items()}
    call = lambda: L.lib().pls_hip_fit_batch(dual.h, Xd.data_ptr(), _ld(Xd), Yd.data_ptr(), _ld(Yd), N, K, M, A, nprob, L.F64, L.MEM_DEVICE,
                                             *[out[k].data_ptr() for k in NAMES])
    assert call() == L.OK
    dual.synchronize()
    got = dict(R=out["R"].view(nprob, A, K).transpose(1, 2), Q=out["Q"].view(nprob, A, M).transpose(1, 2), tt=out["tt"].view(nprob, A),
               B=out["B"].view(nprob, M, K).transpose(1, 2), ssy=out["ssy"].view(nprob, M))
    check(_as_np(got), case_yardstick(name), name + " raw call")
    dual.set_option(pls_amd.OPT_ALGO, 0)
    assert call() == L.ERR_UNSUPPORTED  # (the route, not a wider limit elsewhere, took the call above)


# ---- 3. one sweep over X --------------------------------------------------------------------------------------------------------
def _profiled(h, X, Ys, A, want):
    h.timing()
    h.fit_batch(X, Ys, 1, A, want=want)
    h.synchronize()
    return h.timing()


def _assert_one_sweep(t, N, K, extra, what):
    assert t["launches"]["xty"] == 1 + extra, (what, t)
    assert t["launches"]["xb"] == 0 and t["launches"]["deflate"] == 0 and t["launches"]["fused"] == 0, (what, t)
    if extra == 0:
        assert t["bytes"]["xty"] == N * K * 8 + N * N * 8, (what, t)


def test_dual_batch_one_sweep_over_x():
    """Q, tt, ssy: one sweep over X and G, for 3 problems as for 40.  With B added: one launch of the back-projection per
    round beyond it -- dual_xtv_kernel up to 64 columns, dual_xtvb_kernel beyond; under
    PLS_HIP_DUALBATCH_SWEEPS=1 one sweep per 64 columns"""
    import pls_amd
    N, K, A = 60, 20000, 4
    with dual_handle() as h:
        X = h.synth_x(0, N, K, 5)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        for nprob in (3, 40):
            Ys = h.synth_y(0, N, nprob, 5)
            _assert_one_sweep(_profiled(h, X, Ys, A, ("Q", "tt", "ssy")), N, K, 0, nprob)
            _assert_one_sweep(_profiled(h, X, Ys, A, ("Q", "tt", "ssy", "B")), N, K, 1, (nprob, "B"))
        Ys = h.synth_y(0, N, 150, 5)
        _assert_one_sweep(_profiled(h, X, Ys, A, ("B",)), N, K, 1, "150 problems, B")
        _assert_one_sweep(_profiled(h, X, Ys, A, ("R", "B")), N, K, 2, "150 problems, R and B")
        h.set_option(pls_amd.OPT_PROFILE, 0)
    with dual_handle(PLS_HIP_DUALBATCH_SWEEPS=1) as h:
        h.set_option(pls_amd.OPT_PROFILE, 1)
        _assert_one_sweep(_profiled(h, X, Ys, A, ("B",)), N, K, 3, "150 problems, B in sweeps of 64 columns")
        h.set_option(pls_amd.OPT_PROFILE, 0)
    with handle_with_env() as h:  # without the option the profile is another: X^T X and X^T Ys
        h.set_option(pls_amd.OPT_PROFILE, 1)
        t = _profiled(h, X, h.synth_y(0, N, 3, 5), A, ("Q", "tt", "ssy"))
        h.set_option(pls_amd.OPT_PROFILE, 0)
    assert not (t["launches"]["xty"] == 1 and t["bytes"]["xty"] == N * K * 8 + N * N * 8), t


# ---- 4. rounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["97x1500", "130x600-p21"])
@pytest.mark.parametrize("cap", [5, 1])
def test_dual_batch_rounds(name, cap):
    """several rounds (21 problems in rounds of 5: a ragged last one; one problem per round) against the same yardstick"""
    with dual_handle(PLS_HIP_DUALBATCH_ROUND=cap) as h:
        check(run(h, name), case_yardstick(name), f"{name} rounds of {cap}")


def test_dual_batch_sweeps_of_64_columns_agree():
    """the other form of the back-projection beyond 64 columns (PLS_HIP_DUALBATCH_SWEEPS=1) meets the same bars"""
    name = "130x600-p140"
    with dual_handle(PLS_HIP_DUALBATCH_SWEEPS=1) as h:
        check(run(h, name), case_yardstick(name), name + " sweeps of 64 columns")


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------
def test_dual_batch_is_deterministic(dual):
    """the same bits twice on one handle and once on a fresh one"""
    name = "130x600-p140"
    first = run(dual, name)
    assert _same_bits(first, run(dual, name))
    with dual_handle() as h:
        assert _same_bits(first, run(h, name))


# ---- 6. every subset of outputs -------------------------------------------------------------------------------------------------
def test_dual_batch_every_subset_of_outputs(dual):
    name = "17x1003"
    full = run(dual, name)
    for r in range(len(NAMES) + 1):
        for want in itertools.combinations(NAMES, r):
            for mem in ("device", "host"):
                got = run(dual, name, mem, want)
                assert set(got) == set(want)
                for k in want:
                    if mem == "device":
                        assert np.array_equal(got[k].view(np.int64), full[k].view(np.int64)), (want, mem, k)
                    else:
                        assert np.abs(got[k] - full[k]).max() <= 1e-12 * max(np.abs(full[k]).max(), 1.0), (want, mem, k)


# ---- 7. guarded buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [NAMES, ("B",), ("R", "ssy"), ()], ids=["all", "B", "R-ssy", "none"])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("name", ["17x1003", "130x600-p140"])
def test_dual_batch_writes_exactly_its_outputs(name, layout, want):
    """each requested output fully written, the others, the guards and the inputs untouched ("eigen": odd leading dimension,
    pointers aligned to 8 bytes only; 130 x 600 with 140 problems: ragged K, 140 and 420 columns of the back-projection)"""
    from pls_amd import _lib as L
    torch = _torch()
    N, K, M, A, nprob, dt, _ = CASES[name]
    Xh, Ysh = case_data(name)
    gx, X = _place(Xh, torch.float64, layout)
    gy, Ys = _place(Ysh, torch.float64, layout)
    snap = Inputs(X=X, Ys=Ys)
    go = Guarded([(K * A, nprob, K * A), (M * A, nprob, M * A), (A, nprob, A), (K * M, nprob, K * M), (M, nprob, M)], torch.float64,
                 layout)
    with dual_handle() as h:
        rc = L.lib().pls_hip_fit_batch(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A, nprob, L.F64, L.MEM_DEVICE,
                                       *[go.ptr(i) if k in want else None for i, k in enumerate(NAMES)])
        L.check(rc, h.h)
        h.synchronize()
    go.assert_untouched()
    gx.assert_untouched(); gy.assert_untouched()
    snap.check()
    for i, k in enumerate(NAMES):
        if k in want:
            go.assert_written(i)
        else:
            go.assert_prefilled(i)
    arr = lambda i: go[i].cpu().numpy().astype(np.float64).T
    got = dict(R=arr(0).reshape(nprob, A, K).transpose(0, 2, 1), Q=arr(1).reshape(nprob, A, M).transpose(0, 2, 1), tt=arr(2),
               B=arr(3).reshape(nprob, M, K).transpose(0, 2, 1), ssy=arr(4))
    check({k: got[k] for k in want}, case_yardstick(name), f"guarded {name} {layout} {want}")


# ---- 8. the cross-check ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["97x1500", "130x600-p21", "1031x3000-f32"])
def test_dual_batch_refit_switch_is_the_cross_check(dual, name):
    """PLS_HIP_BATCH_REFIT=1 under the option keeps the per-problem route; the two agree within the bars"""
    got = run(dual, name)
    with dual_handle(PLS_HIP_BATCH_REFIT=1) as h:
        refit = run(h, name)
    check(refit, case_yardstick(name), name + " refit under ALGO_DUAL")
    check(refit, got, name + " refit vs the sample-space route")
    assert not _same_bits(refit, got)  # (two routes)


# ---- 9. declined calls route as before ------------------------------------------------------------------------------------------
def _synth_problem(N, K, M, nprob):
    from test_dual_batch_ref import _oracle
    from test_fit_batch_ref import make_perms, stack_problems
    o = _oracle()
    X = o.synth_x(0, N, K); X = np.asfortranarray(X - X.mean(axis=0))
    Y = o.synth_y(0, N, M); Y = Y - Y.mean(axis=0)
    return X, stack_problems(Y, make_perms(N, nprob - 1, 1))


def test_dual_batch_declined_calls_route_as_before(handle):
    """M = 40 under the option, a one-rank reducer under the option, a handle without the option: bit-equal to a plain handle"""
    import pls_amd
    from pls_amd import _lib as L
    handle.set_option(pls_amd.OPT_ALGO, 0)
    for what, (N, K, M, A, nprob) in dict(m40=(200, 48, 40, 3, 2), reducer=(97, 300, 2, 4, 5)).items():
        X, Ys = _synth_problem(N, K, M, nprob)
        Xd, Yd = _dev(X), _dev(Ys)
        plain = _as_np(handle.fit_batch(Xd, Yd, M, A, want=NAMES))
        with dual_handle() as h:
            if what == "reducer":
                cb = L.ALLREDUCE_FN(lambda user, buf, count, stream: 0)  # (one rank: the sum is the identity)
                L.check(L.lib().pls_hip_set_reducer(h.h, cb, None, 0, 1), h.h)
            got = _as_np(h.fit_batch(Xd, Yd, M, A, want=NAMES))
            h.synchronize()
            if what == "reducer":
                h.clear_reducer()
                taken = _as_np(h.fit_batch(Xd, Yd, M, A, want=NAMES))  # (... and without the reducer the route is taken)
                assert not _same_bits(taken, plain)
        assert _same_bits(got, plain), what
    with handle_with_env() as h:  # a fresh handle without the option
        assert _same_bits(_as_np(h.fit_batch(Xd, Yd, M, A, want=NAMES)), plain)


# ---- 10. groups -----------------------------------------------------------------------------------------------------------------
def test_dual_batch_one_member_group():
    """pls_hip_group_fit_batch on a one-member group reaches the route through the member's handle: values at the bars, and the
    K = 40001 of the case is beyond every other route"""
    import pls_amd
    for name in ("nir", "129x40001"):
        N, K, M, A, nprob, dt, _ = CASES[name]
        Xh, Ysh = case_data(name)
        g = pls_amd.Group([0])
        try:
            g.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
            X, Ys = g.upload(np.asfortranarray(Xh)), g.upload(np.asfortranarray(Ysh))
            got = _as_np(g.fit_batch(X, Ys, M, A, want=NAMES))
            g.free(X); g.free(Ys)
        finally:
            g.close()
        check(got, case_yardstick(name), name + " one-member group")


def test_dual_batch_larger_group_routes_as_before():
    """two members on one device: the same results with and without the option"""
    import pls_amd
    name = "97x1500"
    N, K, M, A, nprob, dt, _ = CASES[name]
    Xh, Ysh = case_data(name)
    res = []
    for algo in (0, pls_amd.ALGO_DUAL):
        g = pls_amd.Group([0, 0])
        try:
            g.set_option(pls_amd.OPT_ALGO, algo)
            X, Ys = g.upload(np.asfortranarray(Xh)), g.upload(np.asfortranarray(Ysh))
            res.append(_as_np(g.fit_batch(X, Ys, M, A, want=NAMES)))
            g.free(X); g.free(Ys)
        finally:
            g.close()
    assert _same_bits(res[0], res[1])
    check(res[1], case_yardstick(name), name + " group [0, 0] under the option")


# ---- 11. the permutation test ---------------------------------------------------------------------------------------------------
def test_dual_batch_permutation_test_nir(dual, po):
    import pls_amd
    X, Y = nir_z(po)
    nperm = 199
    with handle_with_env() as h:
        base = h.permutation_test(_dev(X), _dev(Y), 3, nperm, seed=NIR_SEED)
    for where in ("device", "host"):
        Xi, Yi = (_dev(X), _dev(Y)) if where == "device" else (X, Y)
        t = dual.permutation_test(Xi, Yi, 3, nperm, seed=NIR_SEED)
        assert np.array_equal(t["perms"], base["perms"])
        assert np.abs(t["r2y"][0] - np.array(NIR_R2Y)).max() <= 5e-7
        assert np.array_equal(t["p"], np.full((1, 3), 1.0 / 200.0))
        assert np.abs(t["r2y_perm"] - base["r2y_perm"]).max() <= 1e-10 and np.abs(t["r2y"] - base["r2y"]).max() <= 1e-10
    m = pls_amd.Model(_dev(X), _dev(Y), pls_amd.KERNEL_TYPE1, 3, handle=dual)
    tm = m.permutation_test(nperm, seed=NIR_SEED)
    assert np.abs(tm["r2y_perm"] - base["r2y_perm"]).max() <= 1e-10 and np.array_equal(tm["p"], base["p"])


def test_dual_batch_permutation_test_wide(dual):
    """Handle.permutation_test on a matrix beyond the other routes (K = 40001): runs, and agrees with the yardstick's R^2 Y"""
    import pls_amd
    from test_fit_batch_ref import make_perms
    name = "129x40001"
    N, K, M, A, nprob, dt, _ = CASES[name]
    X, Ys = case_data(name)
    y = case_yardstick(name)
    t = dual.permutation_test(_dev(X), _dev(np.asfortranarray(Ys[:, :M])), A, 0, perms=make_perms(N, nprob - 1, 1))
    r2 = pls_amd.r2y_by_components(y["Q"], y["tt"], y["ssy"])
    assert np.abs(t["r2y"] - r2[0]).max() <= 1e-12 and np.abs(t["r2y_perm"] - r2[1:]).max() <= 1e-12


# ---- 12. the C++ member ---------------------------------------------------------------------------------------------------------
def test_dual_batch_cpp_program():
    """tests/cpp/fit_batch (PLS::Model::permutation_test against one Model per problem) under PLS_HIP_ALGO=dual"""
    exe = os.path.join(ROOT, "tests", "cpp", "fit_batch")
    assert os.path.exists(exe), "tests/cpp/fit_batch not built (build() makes it through pls_amd/host/Makefile)"
    env = dict(os.environ, PLS_HIP_DEVICES="0", PLS_HIP_ALGO="dual")
    r = subprocess.run([exe, os.path.join(DATA, "nir.csv"), os.path.join(DATA, "octane.csv"), "3", "25"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and "fit_batch: ok" in r.stdout, r.stdout + r.stderr
