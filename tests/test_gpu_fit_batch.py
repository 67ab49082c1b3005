"""pls_hip_fit_batch on the GPU: many response sets against one X, and the response-permutation test on top of it.

Yardstick (tests/test_fit_batch_ref.py): one oracle KERNEL_TYPE2 fit per problem, on the fp32-rounded inputs for fp32 storage.
Bars, the project's own: B by po.rel_fro below TOL_B, the R and Q columns (sign-aligned on R) below TOL_COL of
tests/test_gpu_parity.py for A < 20; the Gram-route bars of test_resident_gram_single_launch_fit (1e-8 / 1e-7) for A >= 20;
ssy to 1e-13 relative.  tt = r^T (X^T X) r is quadratic in r, so given the column bar e on r its bar follows:
|r^T G r - s^T G s| <= |G|_2 (|r| + |s|) |r - s| <= 2.1 e |G|_2 |s|^2.
Inputs: po.synth_x / po.synth_y, column-centred; problem 0 is Y, the others are row permutations of it from a fixed seed.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT, handle_with_env
from test_fit_batch_ref import NIR_R2Y, NIR_SEED, batch_yardstick, make_perms, nir_z, stack_problems
from test_gpu_bounds import Guarded, Inputs, _place
from test_gpu_parity import TOL_B, TOL_COL, to_dev

pytestmark = pytest.mark.gpu

PERM_SEED = 20261016
#        N     K    M   A  nprob
CASES = [(1000, 64, 1, 10, 37), (4097, 513, 1, 8, 9), (2048, 128, 4, 6, 17), (1000, 7, 2, 3, 5), (600, 200, 1, 20, 6),
         (2048, 512, 8, 12, 5)]
CASE_IDS = [f"{n}x{k}-m{m}-a{a}-p{p}" for n, k, m, a, p in CASES]


def _torch():
    import torch
    return torch


def bars(A):
    return (1e-8, 1e-7) if A >= 20 else (TOL_B, TOL_COL)


_CACHE = {}


def problem_set(po, oracle, N, K, M, A, nprob, dt="f64", seed=PERM_SEED):
    """(Xh, Ysh, yardstick) in the storage precision dt (as float64 arrays holding the rounded values)"""
    key = (N, K, M, A, nprob, dt, seed)
    if key not in _CACHE:
        X = po.synth_x(0, N, K); X = X - X.mean(axis=0)
        Y = po.synth_y(0, N, M); Y = Y - Y.mean(axis=0)
        Ys = stack_problems(Y, make_perms(N, nprob - 1, seed))
        if dt == "f32":
            X = X.astype(np.float32).astype(np.float64); Ys = Ys.astype(np.float32).astype(np.float64)
        X = np.asfortranarray(X); Ys = np.asfortranarray(Ys)
        _CACHE[key] = (X, Ys, batch_yardstick(oracle, X, Ys, M, A))
    return _CACHE[key]


def as_np(out):
    torch = _torch()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64) for k, v in out.items()}


def run(handle, Xh, Ysh, M, A, dt="f64", mem="device", want=("R", "Q", "tt", "B", "ssy")):
    torch = _torch()
    if mem == "device":
        tdt = torch.float64 if dt == "f64" else torch.float32
        out = handle.fit_batch(to_dev(Xh, tdt), to_dev(Ysh, tdt), M, A, want=want)
        handle.synchronize()
    else:
        ndt = np.float64 if dt == "f64" else np.float32
        out = handle.fit_batch(Xh.astype(ndt), Ysh.astype(ndt), M, A, want=want)
    return as_np(out)


def column_err(Rg, Qg, Rr, Qr):
    """per component: the larger relative error of the R and the Q column, sign-aligned on R"""
    s = np.sign(np.einsum("ka,ka->a", Rr, Rg)); s[s == 0] = 1.0
    er = np.linalg.norm(Rg * s - Rr, axis=0) / np.linalg.norm(Rr, axis=0)
    eq = np.linalg.norm(Qg * s - Qr, axis=0) / np.linalg.norm(Qr, axis=0)
    return np.maximum(er, eq)


def check_batch(po, got, y, Xh, A, what):
    """every requested output of every problem against the yardstick y (or another GPU result) within the bars"""
    tol_b, tol_col = bars(A)
    nprob = y["ssy"].shape[0]
    g2 = np.linalg.norm(Xh, 2) ** 2 if "tt" in got else 0.0
    worst = dict(B=0.0, col=0.0, tt=0.0, ssy=0.0)
    for b in range(nprob):
        if "B" in got:
            assert np.isfinite(got["B"][b]).all(), (what, b)
            worst["B"] = max(worst["B"], po.rel_fro(got["B"][b], y["B"][b]))
        if "R" in got and "Q" in got:
            worst["col"] = max(worst["col"], float(column_err(got["R"][b], got["Q"][b], y["R"][b], y["Q"][b]).max()))
        if "tt" in got:
            bar = 2.1 * tol_col * g2 * (np.linalg.norm(y["R"][b], axis=0) ** 2)
            worst["tt"] = max(worst["tt"], float((np.abs(got["tt"][b] - y["tt"][b]) / bar).max()))
        if "ssy" in got:
            worst["ssy"] = max(worst["ssy"], float((np.abs(got["ssy"][b] - y["ssy"][b]) / y["ssy"][b]).max()))
    print(f"[fit-batch] {what}: B {worst['B']:.2e} (bar {tol_b:.0e})  columns {worst['col']:.2e} (bar {tol_col:.0e})  "
          f"tt {worst['tt']:.2e} of its bar  ssy {worst['ssy']:.2e} (bar 1e-13)")
    assert worst["B"] < tol_b, what
    assert worst["col"] <= tol_col, what
    assert worst["tt"] <= 1.0, what
    assert worst["ssy"] <= 1e-13, what


# ---- 1. the table, both storage types, both memory kinds --------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("N,K,M,A,nprob", CASES, ids=CASE_IDS)
def test_table_against_the_oracle(handle, po, oracle, N, K, M, A, nprob, dt, mem):
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob, dt)
    got = run(handle, Xh, Ysh, M, A, dt, mem)
    assert got["R"].shape == (nprob, K, A) and got["Q"].shape == (nprob, M, A) and got["B"].shape == (nprob, K, M)
    assert got["tt"].shape == (nprob, A) and got["ssy"].shape == (nprob, M)
    check_batch(po, got, y, Xh, A, f"{N}x{K} m{M} a{A} p{nprob} {dt} {mem}")


# ---- 2. every problem against pls_hip_fit(KERNEL_TYPE2) -----------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,A,nprob", CASES, ids=CASE_IDS)
def test_each_problem_against_single_fits(handle, po, oracle, N, K, M, A, nprob):
    import pls_amd
    Xh, Ysh, _ = problem_set(po, oracle, N, K, M, A, nprob)
    got = run(handle, Xh, Ysh, M, A)
    Xd = to_dev(Xh)
    single = {k: [] for k in ("R", "Q", "B")}
    for b in range(nprob):
        o = handle.fit_device(Xd, to_dev(np.asfortranarray(Ysh[:, b * M:(b + 1) * M])), A, pls_amd.KERNEL_TYPE2)
        handle.synchronize()
        for k in single:
            single[k].append(o[k].cpu().numpy().copy())
    y = {k: np.stack(v) for k, v in single.items()}
    y["ssy"] = got["ssy"]
    check_batch(po, {k: got[k] for k in ("R", "Q", "B")}, y, Xh, A, f"{N}x{K} m{M} vs pls_hip_fit")


# ---- 3. the per-problem route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,A,nprob", [CASES[0], CASES[2], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[2], CASE_IDS[3]])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_refit_switch_equals_batched_route(handle, po, oracle, N, K, M, A, nprob, dt):
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob, dt)
    batched = run(handle, Xh, Ysh, M, A, dt)
    with handle_with_env(PLS_HIP_BATCH_REFIT=1) as h2:
        refit = run(h2, Xh, Ysh, M, A, dt)
        refit_host = run(h2, Xh, Ysh, M, A, dt, "host")
    check_batch(po, refit, y, Xh, A, f"refit route {N}x{K} m{M} {dt}")
    check_batch(po, refit_host, y, Xh, A, f"refit route, host memory {N}x{K} m{M} {dt}")
    check_batch(po, refit, batched, Xh, A, f"refit vs batched {N}x{K} m{M} {dt}")


def test_forty_responses_take_the_per_problem_route(handle, po, oracle):
    N, K, M, A, nprob = 1000, 64, 40, 5, 3
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob)
    check_batch(po, run(handle, Xh, Ysh, M, A), y, Xh, A, "M = 40, device")
    check_batch(po, run(handle, Xh, Ysh, M, A, mem="host"), y, Xh, A, "M = 40, host")


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,A,nprob", [CASES[0], CASES[1], CASES[5]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[5]])
def test_repeated_call_is_bit_identical(handle, po, oracle, N, K, M, A, nprob):
    Xh, Ysh, _ = problem_set(po, oracle, N, K, M, A, nprob)
    first = run(handle, Xh, Ysh, M, A)
    for _ in range(3):
        again = run(handle, Xh, Ysh, M, A)
        for k in first:
            assert np.array_equal(first[k].view(np.int64), again[k].view(np.int64)), k


# ---- 5. one problem, many problems, several rounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,A", [(1000, 64, 1, 10), (2048, 512, 8, 12)])
def test_single_problem(handle, po, oracle, N, K, M, A):
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, 1)
    check_batch(po, run(handle, Xh, Ysh, M, A), y, Xh, A, f"one problem m{M}")


def test_1500_problems_and_forced_rounds(handle, po, oracle):
    """1500 single-response problems at K = 64 in one round (12 column blocks of the wide product); the same under a round
    limit of 200 problems: 8 rounds of two column blocks each"""
    N, K, M, A, nprob = 1000, 64, 1, 10, 1500
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob)
    one = run(handle, Xh, Ysh, M, A)
    check_batch(po, one, y, Xh, A, "1500 problems, one round")
    with handle_with_env(PLS_HIP_BATCH_ROUND=200) as h2:
        rounds = run(h2, Xh, Ysh, M, A)
        check_batch(po, rounds, y, Xh, A, "1500 problems, rounds of 200")
        check_batch(po, rounds, one, Xh, A, "rounds of 200 vs one round")
        rounds_host = run(h2, Xh, Ysh, M, A, mem="host")
        check_batch(po, rounds_host, y, Xh, A, "1500 problems, rounds of 200, host memory")
    with handle_with_env(PLS_HIP_BATCH_ROUND=3) as h3:  # M > 1: rounds that end inside the table's 17 problems
        Xm, Ym, ym = problem_set(po, oracle, 2048, 128, 4, 6, 17)
        check_batch(po, run(h3, Xm, Ym, 4, 6), ym, Xm, 6, "17 problems m4, rounds of 3")


# ---- 6. every subset of outputs -------------------------------------------------------------------------------------------------
def test_every_subset_of_outputs(handle, po, oracle):
    N, K, M, A, nprob = CASES[2]
    Xh, Ysh, _ = problem_set(po, oracle, N, K, M, A, nprob)
    full = run(handle, Xh, Ysh, M, A)
    names = ("R", "Q", "tt", "B", "ssy")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            for mem in ("device", "host"):
                got = run(handle, Xh, Ysh, M, A, mem=mem, want=want)
                assert set(got) == set(want)
                for k in want:
                    assert np.array_equal(got[k].view(np.int64), full[k].view(np.int64)), (want, mem, k)


# ---- 7. guarded buffers ---------------------------------------------------------------------------------------------------------
def _guarded_call(h, po, oracle, N, K, M, A, nprob, dt, layout, mem):
    """the raw entry point on guarded inputs and outputs: (outputs as arrays, yardstick, Xh, launches per kernel family)"""
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob, dt)
    dev = "cuda" if mem == "device" else "numpy"
    tdt = (torch.float64 if dt == "f64" else torch.float32) if mem == "device" else (np.float64 if dt == "f64" else np.float32)
    odt = torch.float64 if mem == "device" else np.float64
    gx, X = _place(Xh, tdt, layout, dev)
    gy, Ys = _place(Ysh, tdt, layout, dev)
    shapes = [(K * A, nprob, K * A), (M * A, nprob, M * A), (A, nprob, A), (K * M, nprob, K * M), (M, nprob, M)]
    go = Guarded(shapes, odt, layout, dev)
    snap = Inputs(X=X, Ys=Ys)
    h.set_option(pls_amd.OPT_PROFILE, 2)  # (launch counts per kernel family: which product ran)
    h.timing()
    rc = L.lib().pls_hip_fit_batch(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A, nprob, L.F64 if dt == "f64" else L.F32,
                                   L.MEM_DEVICE if mem == "device" else L.MEM_HOST, go.ptr(0), go.ptr(1), go.ptr(2), go.ptr(3),
                                   go.ptr(4))
    L.check(rc, h.h)
    h.synchronize()
    launches = h.timing()["launches"]
    go.check()
    gx.assert_untouched(); gy.assert_untouched()
    snap.check()
    arr = lambda i: (go[i].cpu().numpy() if mem == "device" else np.asarray(go[i])).astype(np.float64).T
    got = dict(R=arr(0).reshape(nprob, A, K).transpose(0, 2, 1), Q=arr(1).reshape(nprob, A, M).transpose(0, 2, 1), tt=arr(2),
               B=arr(3).reshape(nprob, M, K).transpose(0, 2, 1), ssy=arr(4))
    return got, y, Xh, launches


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("route", ["batched", "refit", "m40"])
def test_guarded_buffers(handle, po, oracle, route, dt, layout, mem):
    """each requested output fully written, guards and inputs untouched, on every route; the "eigen" layout (leading dimension
    N, pointers aligned to 8 bytes only) takes the column-block fallback of the wide product and meets the same bars"""
    shapes = dict(batched=(1001, 130, 2, 5, 70), refit=(1001, 130, 2, 5, 4), m40=(600, 48, 40, 4, 2))[route]
    env = dict(PLS_HIP_BATCH_REFIT=1) if route == "refit" else {}
    with handle_with_env(**env) as h:
        got, y, Xh, launches = _guarded_call(h, po, oracle, *shapes, dt, layout, mem)
    check_batch(po, got, y, Xh, shapes[3], f"guarded {route} {dt} {layout} {mem}")
    if route == "batched" and mem == "device":
        # aligned: one SYRK launch and ONE launch of the wide product; eigen: both decline and run in blocks of 32 columns
        # (X^T X: 5 blocks of the 130 columns, X^T Ys: 5 blocks of the 140), each block at least one launch of the xty family
        if layout == "aligned":
            assert launches["xty"] == 2, launches
        else:
            assert launches["xty"] >= 10, launches


# ---- 8. invalid arguments -------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(handle):
    from pls_amd import _lib as L
    torch = _torch()
    N, K, M, A, nprob = 64, 8, 2, 3, 4
    gx, X = _place(np.random.default_rng(1).standard_normal((N, K)), torch.float64, "aligned")
    gy, Ys = _place(np.random.default_rng(2).standard_normal((N, nprob * M)), torch.float64, "aligned")
    go = Guarded([(K * A, nprob, K * A), (M * A, nprob, M * A), (A, nprob, A), (K * M, nprob, K * M), (M, nprob, M)], torch.float64)
    good = dict(X=gx.ptr(0), ldx=gx.ld(0), Ys=gy.ptr(0), ldy=gy.ld(0), N=N, K=K, M=M, A=A, nprob=nprob, dtype=L.F64, mem=L.MEM_DEVICE)
    bad = [dict(A=0), dict(A=K + 1), dict(N=0), dict(N=-1), dict(M=0), dict(nprob=0), dict(K=0), dict(ldx=N - 1), dict(ldy=N - 1),
           dict(X=None), dict(Ys=None), dict(dtype=7), dict(mem=5)]
    for change in bad:
        a = dict(good, **change)
        rc = L.lib().pls_hip_fit_batch(handle.h, a["X"], a["ldx"], a["Ys"], a["ldy"], a["N"], a["K"], a["M"], a["A"], a["nprob"],
                                       a["dtype"], a["mem"], go.ptr(0), go.ptr(1), go.ptr(2), go.ptr(3), go.ptr(4))
        handle.synchronize()
        assert rc == L.ERR_INVALID, change
        go.assert_untouched()
        for i in range(5):
            go.assert_prefilled(i)
    # ... and the good call still works afterwards
    rc = L.lib().pls_hip_fit_batch(handle.h, *[good[k] for k in ("X", "ldx", "Ys", "ldy", "N", "K", "M", "A", "nprob", "dtype", "mem")],
                                   go.ptr(0), go.ptr(1), go.ptr(2), go.ptr(3), go.ptr(4))
    assert rc == L.OK
    handle.synchronize()
    go.check()


# ---- 9. row-sharded handles -----------------------------------------------------------------------------------------------------
TIMEOUT = 300


def _worker(rank, port, q, case):
    """one rank: its rows of X and Ys, a counting reducer, one fit_batch -> outputs and the message sizes it saw"""
    splits = case["splits"]
    world = len(splits)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.update({k: str(v) for k, v in case.get("env", {}).items()})
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from datetime import timedelta

    import torch
    import torch.distributed as dist
    import pls_amd
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=TIMEOUT - 60))
    try:
        torch.cuda.set_device(0)
        h = pls_amd.Handle()
        row0 = sum(splits[:rank]); n = splits[rank]
        K, M, A = case["K"], case["M"], case["A"]
        tdt = torch.float32 if case.get("dtype") == "f32" else torch.float64
        X = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(case["Xh"][row0:row0 + n])).cuda().to(tdt))
        Ys = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(case["Ysh"][row0:row0 + n])).cuda().to(tdt))
        sizes = []
        from pls_amd.distributed import attach_reducer
        attach_reducer(h, K, M, post=lambda view, i: sizes.append(int(view.numel())))
        if case.get("mem") == "host":
            X, Ys = X.cpu().numpy(), Ys.cpu().numpy()
        out = h.fit_batch(X, Ys, M, A, want=("R", "Q", "tt", "B", "ssy"))
        h.synchronize()
        out = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).copy() for k, v in out.items()}
        try:
            h.permutation_test(X, Ys[:, :M], A, 2)
            out["perm-raises"] = False
        except ValueError:
            out["perm-raises"] = True
        q.put((rank, dict(out=out, sizes=sizes)))
        h.close()
    except BaseException:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


def _run_ranks(case):
    import queue

    import torch.multiprocessing as mp
    from test_gpu_dist_cv import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q, case)) for r in range(len(case["splits"]))]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in procs:
            try:
                res.append(q.get(timeout=TIMEOUT))
            except queue.Empty:
                pytest.fail(f"a rank did not answer within {TIMEOUT} s (got {[r for r, _ in res]})")
        res.sort(key=lambda t: t[0])
        assert not any("error" in r[1] for r in res), [r[1].get("error") for r in res]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        return [o for _, o in res]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()


def expected_messages(K, M, nprob, round_limit=None):
    """the documented sequence of pls_hip_fit_batch on a sharded handle (include/pls_hip.h, pls_hip_allreduce_fn)"""
    per = (K + 1) * M
    piece = max(1, (1 << 20) // per)
    rnd = nprob if round_limit is None else min(nprob, round_limit)
    sizes = [8 * K * K]
    for b0 in range(0, nprob, rnd):
        nb = min(rnd, nprob - b0)
        for p0 in range(0, nb, piece):
            sizes.append(8 * per * min(piece, nb - p0))
    return sizes


@pytest.mark.parametrize("splits,variant", [([500, 500], "f64"), ([333, 400, 267], "f64"), ([600, 0, 400], "f64"), ([501, 499], "f32"),
                                            ([400, 600], "host"), ([500, 500], "rounds")],
                         ids=["2ranks", "3ranks-ragged", "3ranks-empty-shard", "2ranks-f32", "2ranks-host", "2ranks-rounds"])
def test_row_sharded(handle, po, oracle, splits, variant):
    """outputs bit-identical on every rank, within the bars of the single-rank result and of the oracle, and the messages a
    counting reducer saw are the documented sequence"""
    N, K, M, A, nprob = 1000, 64, 2, 6, 11
    dt = "f32" if variant == "f32" else "f64"
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob, dt)
    case = dict(splits=splits, K=K, M=M, A=A, Xh=Xh, Ysh=Ysh, dtype=dt)
    if variant == "host":
        case["mem"] = "host"
    if variant == "rounds":
        case["env"] = dict(PLS_HIP_BATCH_ROUND=4)
    res = _run_ranks(case)
    first = res[0]["out"]
    for r, o in enumerate(res):
        assert o["out"]["perm-raises"] is True
        for k in ("R", "Q", "tt", "B", "ssy"):
            assert np.array_equal(o["out"][k].view(np.int64), first[k].view(np.int64)), (k, "rank", r)
        assert o["sizes"] == expected_messages(K, M, nprob, 4 if variant == "rounds" else None), (r, o["sizes"])
    got = {k: first[k].astype(np.float64) for k in ("R", "Q", "tt", "B", "ssy")}
    check_batch(po, got, y, Xh, A, f"sharded {splits} {variant}")
    check_batch(po, got, run(handle, Xh, Ysh, M, A, dt), Xh, A, f"sharded {splits} {variant} vs one rank")


def test_row_sharded_message_pieces(handle, po, oracle):
    """more problems than one message holds: (K + 1) M nb is capped at 2^20 values per slice, in whole problems"""
    N, K, M, A, nprob = 300, 127, 4, 3, 2100
    X = po.synth_x(0, N, K); X = np.asfortranarray(X - X.mean(axis=0))
    Y = po.synth_y(0, N, M); Y = Y - Y.mean(axis=0)
    Ysh = stack_problems(Y, make_perms(N, nprob - 1, PERM_SEED))
    res = _run_ranks(dict(splits=[140, 160], K=K, M=M, A=A, Xh=X, Ysh=Ysh))
    want = expected_messages(K, M, nprob)
    assert len(want) == 3 and want[1] == 8 * 512 * 2048 and want[2] == 8 * 512 * 52
    for r, o in enumerate(res):
        assert o["sizes"] == want, (r, o["sizes"])
        for k in ("R", "Q", "tt", "B", "ssy"):
            assert np.array_equal(o["out"][k].view(np.int64), res[0]["out"][k].view(np.int64)), (k, "rank", r)
    one = run(handle, X, Ysh, M, A)
    got = {k: res[0]["out"][k].astype(np.float64) for k in ("R", "Q", "tt", "B", "ssy")}
    check_batch(po, got, one, X, A, "sharded, three messages, vs one rank")
    sample = [0, 1, 2047, 2048, 2099]  # either side of the piece boundary, against the oracle
    ys = batch_yardstick(oracle, X, np.asfortranarray(np.concatenate([Ysh[:, b * M:(b + 1) * M] for b in sample], axis=1)), M, A)
    check_batch(po, {k: v[sample] for k, v in got.items()}, ys, X, A, "sharded, three messages, sampled problems vs oracle")


# ---- 10. group ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,A,nprob", [CASES[0], CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_group_with_repeated_ordinals(handle, po, oracle, N, K, M, A, nprob):
    import pls_amd
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob)
    single = run(handle, Xh, Ysh, M, A)
    g = pls_amd.Group([0, 0, 0])
    try:
        X, Ys = g.upload(Xh), g.upload(Ysh)
        got = as_np(g.fit_batch(X, Ys, M, A, want=("R", "Q", "tt", "B", "ssy")))
        part = as_np(g.fit_batch(X, Ys, M, A, want=("Q", "tt")))
        g.free(X); g.free(Ys)
    finally:
        g.close()
    check_batch(po, got, y, Xh, A, f"group [0,0,0] {N}x{K} m{M}")
    check_batch(po, got, single, Xh, A, f"group [0,0,0] {N}x{K} m{M} vs one handle")
    assert set(part) == {"Q", "tt"} and np.array_equal(part["Q"], got["Q"]) and np.array_equal(part["tt"], got["tt"])


# ---- 11. the permutation test ---------------------------------------------------------------------------------------------------
def test_permutation_test_nir(handle, po, oracle):
    import pls_amd
    torch = _torch()
    X, Y = nir_z(po)
    nperm = 199
    perms = make_perms(X.shape[0], nperm, NIR_SEED)
    y = batch_yardstick(oracle, X, stack_problems(Y, perms), 1, 3)
    r2 = pls_amd.r2y_by_components(y["Q"], y["tt"], y["ssy"])
    p_ref = pls_amd.permutation_pvalues(r2[0], r2[1:])
    for where in ("device", "host"):
        Xi, Yi = (to_dev(X), to_dev(Y)) if where == "device" else (X, Y)
        t = handle.permutation_test(Xi, Yi, 3, nperm, seed=NIR_SEED)
        assert np.array_equal(t["perms"], perms)
        assert t["r2y"].shape == (1, 3) and t["r2y_perm"].shape == (nperm, 1, 3) and t["p"].shape == (1, 3)
        assert np.abs(t["r2y"] - r2[0]).max() <= 1e-9 and np.abs(t["r2y_perm"] - r2[1:]).max() <= 1e-9
        assert np.abs(t["r2y"][0] - np.array(NIR_R2Y)).max() <= 5e-7
        assert np.array_equal(t["p"], p_ref) and np.array_equal(t["p"], np.full((1, 3), 1.0 / 200.0))
        small = handle.permutation_test(Xi, Yi, 3, nperm, seed=NIR_SEED, max_bytes=17 * X.shape[0] * 8)  # chunks of 17 problems
        assert np.abs(small["r2y"] - t["r2y"]).max() <= 1e-12 and np.abs(small["r2y_perm"] - t["r2y_perm"]).max() <= 1e-12
        assert np.array_equal(small["p"], t["p"])
        given = handle.permutation_test(Xi, Yi, 3, 0, perms=perms[:5])
        assert np.array_equal(given["r2y_perm"], t["r2y_perm"][:5])
    m = pls_amd.Model(to_dev(X), to_dev(Y), pls_amd.KERNEL_TYPE2, 3, handle=handle)
    tm = m.permutation_test(nperm, seed=NIR_SEED)
    assert np.abs(tm["r2y"] - r2[0]).max() <= 1e-9 and np.array_equal(tm["p"], p_ref)


# ---- 12. the C++ member ---------------------------------------------------------------------------------------------------------
def test_cpp_program():
    exe = os.path.join(ROOT, "tests", "cpp", "fit_batch")
    assert os.path.exists(exe), "tests/cpp/fit_batch not built (build() makes it through pls_amd/host/Makefile)"
    for devices in ("1", "3"):
        env = dict(os.environ, PLS_HIP_DEVICES="0,0,0" if devices == "3" else "0")
        r = subprocess.run([exe, os.path.join(DATA, "nir.csv"), os.path.join(DATA, "octane.csv"), "3", "25"], capture_output=True,
                           text=True, timeout=300, env=env)
        assert r.returncode == 0 and "fit_batch: ok" in r.stdout, r.stdout + r.stderr
