"""Cross-validation folds on a row-sharded handle (pls_hip_cv_folds as a collective, include/pls_hip.h).

Two or three ranks share the one GPU of the test box, each holding a contiguous block of rows, the messages carried by
pls_amd.distributed's reducer over gloo (or the library's device-side exchange).  test_idx holds GLOBAL row indices.
Every rank must receive the same E bit for bit; E must match the single-process call on the whole matrix (X^T X is summed
in another order, so to 1e-9 rather than bit for bit) and one oracle refit per fold (test_batched_cv_folds's bar)."""
import ctypes
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 240  # seconds per case: every rank's result (or its error) must be back by then


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _blocks(splits):
    return [(sum(splits[:r]), splits[r]) for r in range(len(splits))]


def _worker(rank, port, q, case):
    """one rank: its block of rows, a reducer, then the calls of the case in order -> {call name: E, or ("error", code)}"""
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
    from pls_amd import _lib as L
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=TIMEOUT - 60))
    try:
        torch.cuda.set_device(0)
        h = pls_amd.Handle()
        row0, n = _blocks(splits)[rank]
        K, M, A = case["K"], case["M"], case["A"]
        tdt = torch.float32 if case.get("dtype") == "f32" else torch.float64
        if "Xh" in case:  # a data set of the parent's (the nir example)
            X = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(case["Xh"][row0:row0 + n])).cuda().to(tdt))
            Y = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(case["Yh"][row0:row0 + n])).cuda().to(tdt))
        else:             # synth_x / synth_y at this rank's row0: the rows of the whole matrix this rank owns
            X = h.synth_x(row0, n, K, pls_amd.SEED_DEFAULT, dtype=tdt)
            Y = h.synth_y(row0, n, M, pls_amd.SEED_DEFAULT, dtype=tdt)
        if case.get("reducer") == "ipc":
            from pls_amd.distributed import attach_ipc_exchange
            attach_ipc_exchange(h)
        else:
            from pls_amd.distributed import attach_reducer
            attach_reducer(h, K, M)
        if case.get("mem") == "host":
            X, Y = X.cpu().numpy(), Y.cpu().numpy()
        out = {}
        for name, idx in case["calls"]:
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            if case.get("guard"):  # E inside a guard band of sentinels (test_gpu_bounds.Guarded)
                from test_gpu_bounds import Guarded
                nf, ts = idx.shape
                nobs = nf * ts
                ge = Guarded([(nobs, M * A, nobs)], torch.float64, "aligned", "cuda")
                rc = L.lib().pls_hip_cv_folds(h.h, X.data_ptr(), pls_amd.model._ld(X), Y.data_ptr(), pls_amd.model._ld(Y), n, K,
                                              M, A, idx.ctypes.data_as(ctypes.c_void_p), ts, nf, L.F64, L.MEM_DEVICE, ge.ptr(0))
                L.check(rc, h.h)
                h.synchronize()
                ge.check()
                out[name] = ge[0].cpu().numpy().reshape(nobs, M, A).transpose(1, 0, 2).copy()
                continue
            try:
                t0 = time.perf_counter()
                E = h.cv_folds(X, Y, A, idx)
                E = E.cpu().numpy() if isinstance(E, torch.Tensor) else np.asarray(E)
                out[name + "/s"] = time.perf_counter() - t0
                out[name] = E
            except L.PlsHipError as e:
                out[name] = ("error", e.code)
        q.put((rank, out))
        h.close()
    except BaseException:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


def _run(case):
    """spawn one process per entry of case["splits"]; returns [outputs] in rank order"""
    import queue

    import torch.multiprocessing as mp
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
        return [out for _, out in res]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()


def _synth(oracle, N, K, M):
    return oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)


def _nir(oracle, po):
    from conftest import DATA
    return (oracle.z_scores(po.read_csv(os.path.join(DATA, "nir.csv"))),
            oracle.z_scores(po.read_csv(os.path.join(DATA, "octane.csv"))))


def _lso(N, ts, nf, seed, splits):
    """nf folds of ts distinct rows; fold 0 straddles every shard boundary (the rows on either side of it)"""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(N)[:ts] for _ in range(nf)])
    edges = [b for b in np.cumsum(splits)[:-1] if 0 < b < N]
    near = sorted({int(r) for b in edges for r in (b - 1, b) if 0 <= r < N})[:ts]
    rest = [int(r) for r in rng.permutation(N) if int(r) not in near][:ts - len(near)]
    idx[0] = np.array(near + rest)
    return idx


def _single(handle, Xh, Yh, A, idx, dtype=None):
    """pls_hip_cv_folds on one rank, the whole matrix on the device"""
    import torch
    import pls_amd
    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return pls_amd.as_colmajor(t if dtype is None else t.to(dtype))
    E = handle.cv_folds(dev(Xh), dev(Yh), A, idx).cpu().numpy()
    handle.synchronize()
    return E


def _check(outs, name, E1, ref, what):
    """bit-identical on every rank; within 1e-9 of the single-process call; within 1e-8 of the per-fold oracle refits"""
    E = outs[0][name]
    assert isinstance(E, np.ndarray), (what, name, E)
    for r, o in enumerate(outs):
        assert np.array_equal(o[name], E), (what, name, "rank", r)
    scale = max(np.abs(ref).max(), 1.0)
    gap = np.abs(E - E1).max()
    print(f"[dist-cv] {what} {name}: max |E_sharded - E_single| = {gap:.3e} (scale {scale:.3g}), "
          f"vs oracle {np.abs(E - ref).max():.3e}")
    assert gap < 1e-9 * scale, (what, name, gap)
    assert np.abs(E - ref).max() < 1e-8 * scale, (what, name)
    assert np.abs(E1 - ref).max() < 1e-8 * scale


SYN = dict(N=200, K=24, M=3, A=5, ts=60, nf=12)


@pytest.mark.parametrize("splits", [[100, 100], [67, 67, 66], [98, 100, 2], [100, 0, 100]],
                         ids=["2ranks-even", "3ranks-even", "3ranks-2row-shard", "3ranks-empty-shard"])
def test_sharded_cv_batched_synth(handle, oracle, splits):
    """the batched route (X^T X downdates) with each rank's share of the folds; N = 200, K = 24, M = 3, A = 5"""
    N, K, M, A, ts, nf = (SYN[k] for k in ("N", "K", "M", "A", "ts", "nf"))
    idx = _lso(N, ts, nf, 11, splits)
    outs = _run(dict(splits=splits, K=K, M=M, A=A, calls=[("lso", idx)]))
    Xh, Yh = _synth(oracle, N, K, M)
    from test_gpu_parity import _fold_reference
    _check(outs, "lso", _single(handle, Xh, Yh, A, idx), _fold_reference(oracle, Xh, Yh, A, idx), f"synth {splits}")


@pytest.mark.parametrize("splits", [[30, 30], [29, 1, 30]], ids=["2ranks", "3ranks-1row-shard"])
def test_sharded_cv_nir(handle, oracle, po, splits):
    """z-scored nir / octane (60 x 401, M = 1, A = 10): leave-one-out and 25 folds of 18 rows.  One rank would take the
    single-launch fold kernels on the whole X; a sharded handle never does (they read every row)."""
    Xh, Yh = _nir(oracle, po)
    N, K, A = Xh.shape[0], Xh.shape[1], 10
    loo = np.arange(N)[:, None]
    lso = _lso(N, 18, 25, 5, splits)
    calls = [("loo", loo), ("loo-again", loo), ("lso", lso)]
    outs = _run(dict(splits=splits, K=K, M=1, A=A, Xh=Xh, Yh=Yh, calls=calls))
    from test_gpu_parity import _fold_reference
    t0 = time.perf_counter()
    E1 = _single(handle, Xh, Yh, A, loo)
    t1 = time.perf_counter()
    E1 = _single(handle, Xh, Yh, A, loo)
    t_single = time.perf_counter() - t1
    _check(outs, "loo", E1, _fold_reference(oracle, Xh, Yh, A, loo), f"nir {splits}")
    assert np.array_equal(outs[0]["loo-again"], outs[0]["loo"])
    _check(outs, "lso", _single(handle, Xh, Yh, A, lso), _fold_reference(oracle, Xh, Yh, A, lso), f"nir {splits}")
    print(f"[dist-cv] nir LOO wall time: {len(splits)} ranks on one GPU {max(o['loo-again/s'] for o in outs) * 1e3:.1f} ms "
          f"(slowest rank, second call), one rank {t_single * 1e3:.1f} ms (second call; first {(t1 - t0) * 1e3:.1f} ms)")


@pytest.mark.parametrize("M,env", [(40, {}), (3, {"PLS_HIP_CV_REFIT": 1})], ids=["m40", "refit-switch"])
def test_sharded_cv_refit(oracle, M, env):
    """the refit route: per fold, every rank gathers its own training rows and takes part in one sharded fit"""
    from conftest import handle_with_env
    from test_gpu_parity import _fold_reference
    N, K, A, ts, nf = 200, 24, 5, 60, 6
    splits = [98, 102]
    idx = _lso(N, ts, nf, 13, splits)
    outs = _run(dict(splits=splits, K=K, M=M, A=A, env=env, calls=[("lso", idx)]))
    Xh, Yh = _synth(oracle, N, K, M)
    with handle_with_env(**env) as h1:
        E1 = _single(h1, Xh, Yh, A, idx)
    _check(outs, "lso", E1, _fold_reference(oracle, Xh, Yh, A, idx), f"refit M={M} {env}")


@pytest.mark.parametrize("variant", ["ipc", "f32", "host"])
def test_sharded_cv_reducers_dtype_memory(handle, oracle, variant):
    """the device-side exchange as the reducer; fp32 storage; host-memory (numpy) inputs"""
    import torch
    from test_gpu_parity import _fold_reference
    N, K, M, A, ts, nf = (SYN[k] for k in ("N", "K", "M", "A", "ts", "nf"))
    splits = [101, 99]
    idx = _lso(N, ts, nf, 17, splits)
    case = dict(splits=splits, K=K, M=M, A=A, calls=[("lso", idx)])
    if variant == "ipc":
        case["reducer"] = "ipc"
    elif variant == "f32":
        case["dtype"] = "f32"
    else:
        case["mem"] = "host"
    outs = _run(case)
    Xh, Yh = _synth(oracle, N, K, M)
    if variant == "f32":  # the reference sees the fp32 values the ranks generated
        import pls_amd
        Xh = np.asfortranarray(handle.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=torch.float32).cpu().numpy().astype(np.float64))
        Yh = np.asfortranarray(handle.synth_y(0, N, M, pls_amd.SEED_DEFAULT, dtype=torch.float32).cpu().numpy().astype(np.float64))
    E1 = _single(handle, Xh, Yh, A, idx, torch.float32 if variant == "f32" else None)
    _check(outs, "lso", E1, _fold_reference(oracle, Xh, Yh, A, idx), variant)


def test_sharded_cv_invalid_arguments_on_every_rank(handle, oracle):
    """an index >= n_total and a fold that covers every row: PLS_HIP_ERR_INVALID on EVERY rank (no rank left waiting in a
    collective), and each rank's next valid call succeeds"""
    from pls_amd import _lib as L
    from test_gpu_parity import _fold_reference
    N, K, M, A, ts, nf = 200, 24, 3, 5, 20, 4
    splits = [120, 80]
    good = _lso(N, ts, nf, 19, splits)
    bad_index = good.copy()
    bad_index[2, 5] = N
    all_rows = np.arange(N)[None, :]
    calls = [("bad-index", bad_index), ("after-bad-index", good), ("all-rows", all_rows), ("after-all-rows", good)]
    outs = _run(dict(splits=splits, K=K, M=M, A=A, calls=calls))
    for o in outs:
        assert o["bad-index"] == ("error", L.ERR_INVALID)
        assert o["all-rows"] == ("error", L.ERR_INVALID)
    Xh, Yh = _synth(oracle, N, K, M)
    ref = _fold_reference(oracle, Xh, Yh, A, good)
    E1 = _single(handle, Xh, Yh, A, good)
    _check(outs, "after-bad-index", E1, ref, "errors")
    _check(outs, "after-all-rows", E1, ref, "errors")


@pytest.mark.parametrize("splits", [[100, 100], [100, 0, 100]], ids=["2ranks", "3ranks-empty-shard"])
def test_sharded_cv_writes_exactly_e(handle, oracle, splits):
    """E inside a guard band of sentinel NaNs on every rank: every element written, no guard cell touched"""
    from test_gpu_parity import _fold_reference
    N, K, M, A, ts, nf = (SYN[k] for k in ("N", "K", "M", "A", "ts", "nf"))
    idx = _lso(N, ts, nf, 23, splits)
    outs = _run(dict(splits=splits, K=K, M=M, A=A, guard=True, calls=[("lso", idx)]))
    Xh, Yh = _synth(oracle, N, K, M)
    _check(outs, "lso", _single(handle, Xh, Yh, A, idx), _fold_reference(oracle, Xh, Yh, A, idx), f"guarded {splits}")
