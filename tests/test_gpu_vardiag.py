"""pls_hip_var_diagnostics on the MI355X: ssxk, sst and VIP against the longdouble yardstick of tests/test_vardiag_ref.py with the
worst-case bars derived there (u = 2^-52 for fp64 AND fp32 storage: the scores stay fp64 inside the library).  Every case prints
the device's worst distance in units of its bar.

The shapes straddle the edges of the column sweep's tile (128 rows x 64 columns, ranges of 24 component counts): a single row, less
than a tile, one row and one column past a tile, tails on both axes, a shape whose rows the planner splits (tests/
test_vardiag_layout.py holds 40,000 x 64 to RS > 1 and every shape here to its geometry), short and wide, real data."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, handle_with_env
from test_gpu_parity import to_dev
from test_vardiag_ref import inside, vardiag_bars, vardiag_yardstick
from test_xdiag_ref import nir_z

pytestmark = pytest.mark.gpu

ALL = ("ssxk", "VIP", "sst")
_REF = {}


def _torch():
    import torch
    return torch


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in d.items()}


def problem(oracle, N, K, M, A, f32=False):
    """(X, Y, the oracle's model, the longdouble yardstick, its bars), computed once per shape"""
    key = (N, K, M, A, f32)
    if key not in _REF:
        X, Y = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
        if f32:
            X = np.asfortranarray(X.astype(np.float32).astype(np.float64))
        ref = oracle.plsr(X, Y, A)
        yld = vardiag_yardstick(X, ref["W"], ref["R"], ref["P"], ref["Q"], dtype=np.longdouble)
        _REF[key] = (X, Y, ref, yld, vardiag_bars(X, ref["R"], ref["P"], yld, M))
    return _REF[key]


def dev_model(ref):
    return {k: to_dev(ref[k]) for k in "WRPQ"}


def full_call(handle, X, m, tt=None, want=ALL):
    out = handle.var_diagnostics(X, W=m["W"], R=m["R"], P=m["P"], Q=m["Q"], tt=tt, want=want)
    handle.synchronize()
    return _np(out)


def run_case(handle, label, Xh, ref, yld, bars, dtype=None):
    """all outputs, twice (same bits), each output alone -- all inside the bars"""
    X = to_dev(Xh, dtype)
    m = dev_model(ref)
    a = full_call(handle, X, m)
    b = full_call(handle, X, m)
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), (label, k, "two calls with the same arguments differ")
    inside(a, yld, bars, label)
    for k in ALL:
        one = full_call(handle, X, m, want=(k,))
        assert set(one) == {k}
        assert one[k].tobytes() == a[k].tobytes(), (label, k, "alone it has other bits than with the others")
    return a


# ---- the shapes of the feature request --------------------------------------------------------------------------------------------
SHAPES = [("1x7 a3: a single row", 1, 7, 1, 3), ("9x7 a3: less than a tile", 9, 7, 1, 3),
          ("129x65 a13: one past a tile on both axes", 129, 65, 2, 13), ("1031x513 a12: tails on both axes", 1031, 513, 1, 12),
          ("40000x64 a13: the planner splits the rows", 40000, 64, 2, 13), ("60x4000 a6: short and wide", 60, 4000, 1, 6),
          ("1000x7 a7: A = K", 1000, 7, 4, 7), ("300x64 a30: two ranges", 300, 64, 2, 30)]


@pytest.mark.parametrize("label,N,K,M,A", SHAPES, ids=[s[0].split()[0] for s in SHAPES])
def test_synthetic(handle, oracle, label, N, K, M, A):
    if N == 1:   # (a model needs rows: fitted on 64, the diagnostics of its first row)
        Xf, Yf = oracle.synth_x(0, 64, K), oracle.synth_y(0, 64, M)
        ref = oracle.plsr(Xf, Yf, A)
        X = np.asfortranarray(Xf[:1])
        yld = vardiag_yardstick(X, ref["W"], ref["R"], ref["P"], ref["Q"], dtype=np.longdouble)
        run_case(handle, label, X, ref, yld, vardiag_bars(X, ref["R"], ref["P"], yld, M))
        return
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A)
    run_case(handle, label, X, ref, yld, bars)


def test_nir(handle, oracle, po):
    """real data, z-scored; R^2 X of the whole matrix (the figures of tests/test_xdiag_ref.py) from the columns' sums"""
    X, Y = nir_z(po)
    ref = oracle.plsr(X, Y, 10)
    yld = vardiag_yardstick(X, ref["W"], ref["R"], ref["P"], ref["Q"], dtype=np.longdouble)
    a = run_case(handle, "nir a10", X, ref, yld, vardiag_bars(X, ref["R"], ref["P"], yld, Y.shape[1]))
    r2x = 1.0 - a["ssxk"][:, 1:].sum(0) / a["ssxk"][:, 0].sum()
    assert np.allclose(r2x, [0.650, 0.835, 0.937, 0.963, 0.982, 0.986, 0.988, 0.989, 0.990, 0.992], atol=6e-4)
    assert np.all(np.abs((a["VIP"] ** 2).sum(0) - X.shape[1]) <= 1e-9 * X.shape[1])


def test_fp32_storage(handle, oracle):
    """X in fp32 storage is exact in fp64 and the scores stay fp64 inside the library: the fp64 bars hold.  Aligned (four rows per
    load) and with an odd leading dimension (one row per load)."""
    torch = _torch()
    N, K, M, A = 1031, 64, 2, 10
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A, f32=True)
    run_case(handle, "1031x64 a10 fp32 storage", X, ref, yld, bars, dtype=torch.float32)
    Xd = torch.empty((K, N + 1), dtype=torch.float32, device="cuda")[:, :N].t()
    Xd.copy_(torch.from_numpy(X))
    inside(full_call(handle, Xd, dev_model(ref)), yld, bars, "fp32 storage, odd ld")


def test_tt_given_and_tt_null(handle, oracle):
    """VIP from tt: with the call's own sst passed back the bits of the tt = NULL call; with t^T t of the fit inside the bars
    without the sst term; and X = NULL, N ignored"""
    N, K, M, A = 1031, 513, 1, 12
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A)
    Xd, m = to_dev(X), dev_model(ref)
    a = full_call(handle, Xd, m)
    back = full_call(handle, Xd, m, tt=a["sst"], want=("VIP",))
    assert back["VIP"].tobytes() == a["VIP"].tobytes()
    tt = (ref["T"] ** 2).sum(0)
    vld = vardiag_yardstick(None, ref["W"], None, None, ref["Q"], tt=tt, dtype=np.longdouble)
    tb = vardiag_bars(X, ref["R"], ref["P"], yld, M, tt_given=True)
    out = handle.var_diagnostics(None, W=m["W"], Q=m["Q"], tt=tt, want=("VIP",)); handle.synchronize()
    inside(_np(out), vld, dict(VIP=tb["VIP"]), "VIP alone, tt given, X = NULL")
    # numpy in, numpy out
    hst = handle.var_diagnostics(X, W=ref["W"], R=ref["R"], P=ref["P"], Q=ref["Q"], want=ALL)
    assert all(isinstance(v, np.ndarray) for v in hst.values())
    inside(hst, yld, bars, "numpy inputs")


# ---- layouts and guarded buffers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("N,K,M,A,dt", [(9, 7, 1, 3, "f64"), (129, 65, 2, 13, "f64"), (1031, 64, 2, 10, "f32")])
def test_writes_exactly_its_outputs(handle, oracle, N, K, M, A, dt, layout):
    """exactly K x (A + 1) of ssxk, K x A of VIP and A of sst are written -- padded leading dimensions ("aligned") or ld == rows
    with every pointer one element past a 16-byte boundary ("eigen") -- nothing in the padding, no input changed; every
    combination of NULL outputs, with tt and without, leaves the outputs not asked for untouched and the others with the bits of
    the full call"""
    import pls_amd
    from test_gpu_bounds import Guarded
    torch = _torch()
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A, f32=dt == "f32")
    tdt = torch.float32 if dt == "f32" else torch.float64
    f8 = torch.float64
    gx = Guarded([(N, K)], tdt, layout, "cuda")
    gm = Guarded([(K, A, K), (K, A, K), (K, A, K), (M, A, M), (A, 1)], f8, layout, "cuda")
    go = Guarded([(K, A + 1), (K, A), (A, 1)], f8, layout, "cuda")
    tt = (ref["T"] ** 2).sum(0)

    def put(dst, a):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.dtype))
    put(gx[0], X)
    for i, k in enumerate("WRPQ"):
        put(gm[i], ref[k])
    put(gm[4], tt[:, None])
    keep = [g.raw.clone() for g in (gx, gm)]
    vld = vardiag_yardstick(None, ref["W"], None, None, ref["Q"], tt=tt, dtype=np.longdouble)
    tbar = vardiag_bars(X, ref["R"], ref["P"], yld, M, tt_given=True)["VIP"]
    full = {}
    for use_tt in (False, True):
        for mask in (7, 1, 2, 4, 3, 5, 6):
            go.refill()
            asked = [i for i in range(3) if mask >> i & 1]
            rc = pls_amd.lib().pls_hip_var_diagnostics(handle.h, gx.ptr(0), gx.ld(0), N, K, M, A, gm.ptr(0), gm.ptr(1), gm.ptr(2), gm.ptr(3),
                                                       gm.ptr(4) if use_tt else None, 1 if dt == "f32" else 0,
                                                       go.ptr(0) if 0 in asked else None, go.ld(0), go.ptr(1) if 1 in asked else None,
                                                       go.ld(1), go.ptr(2) if 2 in asked else None)
            assert rc == 0, pls_amd._lib.last_error(handle.h)
            handle.synchronize()
            for g in (gx, gm, go):
                g.assert_untouched()
            for g, k in zip((gx, gm), keep):
                assert (g.raw == k).all(), "an input was written"
            got = {}
            for i, name in enumerate(ALL):
                if i in asked:
                    go.assert_written(i)
                    got[name] = go[i].cpu().numpy() if name != "sst" else go[i][:, 0].cpu().numpy()
                else:
                    go.assert_prefilled(i)
            if mask == 7:
                full[use_tt] = got
                what = f"guarded {N}x{K} a{A} {dt} {layout} tt={'given' if use_tt else 'NULL'}"
                inside({k: v for k, v in got.items() if k != "VIP"}, yld, bars, what)
                inside({"VIP": got["VIP"]}, vld if use_tt else yld, dict(VIP=tbar) if use_tt else bars, what)
            for name, v in got.items():
                assert v.tobytes() == full[use_tt][name].tobytes(), (mask, use_tt, name, "the bits depend on what else was asked for")


def test_bad_arguments(handle):
    """argument errors are PLS_HIP_ERR_INVALID before anything is touched"""
    import pls_amd
    torch = _torch()
    L = pls_amd.lib()
    N, K, M, A = 64, 6, 2, 3
    X = torch.ones(N * K, dtype=torch.float64, device="cuda"); Mt = torch.ones(K * A, dtype=torch.float64, device="cuda")
    out = torch.full((K * (A + 1) + K * A + A,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 8 * off)
    ssxk, VIP, sst = p(out), p(out, K * (A + 1)), p(out, K * (A + 1) + K * A)

    def call(X_=p(X), ldx=N, N_=N, K_=K, M_=M, A_=A, W_=p(Mt), R_=p(Mt), P_=p(Mt), Q_=p(Mt), tt=None, dt=0, s=ssxk, ldk=K, v=VIP, ldv=K,
             t=sst):
        return L.pls_hip_var_diagnostics(handle.h, X_, ldx, N_, K_, M_, A_, W_, R_, P_, Q_, tt, dt, s, ldk, v, ldv, t)
    assert call() == 0
    handle.synchronize()
    out.fill_(7.0)
    assert call(X_=None) == 1 and call(ldx=N - 1) == 1 and call(N_=0) == 1 and call(N_=-1) == 1
    assert call(A_=K + 1) == 1 and call(A_=0) == 1 and call(dt=2) == 1
    assert call(R_=None) == 1 and call(P_=None) == 1 and call(W_=None) == 1 and call(Q_=None) == 1 and call(M_=0) == 1
    assert call(ldk=K - 1) == 1 and call(ldv=K - 1) == 1
    assert call(R_=None, s=None, v=None) == 1           # sst needs the scores
    assert call(X_=None, s=None, t=None) == 1           # VIP without tt needs them too
    handle.synchronize()
    assert bool(out.eq(7.0).all()), "a rejected call wrote"
    # what is not needed may be missing: VIP from tt reads nothing N-sized; ssxk alone needs neither W nor Q
    assert call(X_=None, N_=0, R_=None, P_=None, tt=p(Mt), s=None, t=None) == 0
    assert call(W_=None, Q_=None, M_=0, v=None) == 0
    assert call(s=None, v=None, t=None) == 0            # nothing asked for: nothing done
    handle.synchronize()


def test_fresh_handle_and_used_handle_return_the_same_bits(handle, oracle):
    """a fresh handle, and one that has just run another shape and another entry point"""
    N, K, M, A = 1031, 513, 1, 12
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A)
    Xd, m = to_dev(X), dev_model(ref)
    with handle_with_env() as h:
        a = full_call(h, Xd, m)
    X2, Y2, ref2, _, _ = problem(oracle, 129, 65, 2, 13)
    with handle_with_env() as h:
        full_call(h, to_dev(X2), dev_model(ref2))
        h.x_diagnostics(Xd, m["R"], m["P"], want=("Q", "T2", "ssx", "sst"))
        h.fit_device(to_dev(X2), to_dev(Y2), 5)
        b = full_call(h, Xd, m)
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), k
    inside(a, yld, bars, "fresh handle")


# ---- sharded handle -----------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, N, K, M, A, splits, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import pls_amd
    from oracle import pls_oracle as po
    from pls_amd.distributed import attach_reducer
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        h = pls_amd.Handle()
        ora = po.OracleLib()
        ref = ora.plsr(ora.synth_x(0, N, K), ora.synth_y(0, N, M), A)
        row0, nrows = sum(splits[:rank]), splits[rank]
        X = h.synth_x(row0, nrows, K, pls_amd.SEED_DEFAULT)
        msgs = []
        attach_reducer(h, K, M, post=lambda view, i: msgs.append(int(view.numel())))
        m = {k: torch.from_numpy(ref[k]).cuda() for k in "WRPQ"}
        tt = (ref["T"] ** 2).sum(0)
        res = {}
        for name, want, t in (("all", ("ssxk", "VIP", "sst"), None), ("vip_sst", ("VIP",), None), ("vip_tt", ("VIP",), tt)):
            del msgs[:]
            out = h.var_diagnostics(X, W=m["W"], R=m["R"], P=m["P"], Q=m["Q"], tt=t, want=want)
            h.synchronize()
            res[name] = {k: v.cpu().numpy() for k, v in out.items()}
            res[name + "_msgs"] = list(msgs)
        q.put((rank, res))
        h.close()
    except BaseException:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("splits", [[2050, 2047], [2049, 0, 2048]], ids=["2ranks-uneven", "3ranks-one-empty"])
def test_sharded_handle(oracle, splits):
    """a collective on a row-sharded handle: every output bit-identical on all ranks and inside the bars of the whole matrix;
    exactly ONE message when X is needed -- 8 (A + K (A + 1)) values with ssxk, 8 A without -- and none for VIP from tt"""
    import torch.multiprocessing as mp
    N, K, M, A = sum(splits), 96, 1, 9
    world = len(splits)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, N, K, M, A, splits, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
    assert not any("error" in r[1] for r in res), [r[1].get("error") for r in res]
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    X, Y, ref, yld, bars = problem(oracle, N, K, M, A)
    tt = (ref["T"] ** 2).sum(0)
    vld = vardiag_yardstick(None, ref["W"], None, None, ref["Q"], tt=tt, dtype=np.longdouble)
    tbar = vardiag_bars(X, ref["R"], ref["P"], yld, M, tt_given=True)["VIP"]
    for rank, out in res:
        assert out["all_msgs"] == [8 * (A + K * (A + 1))] and out["vip_sst_msgs"] == [8 * A] and out["vip_tt_msgs"] == [], (rank, out["all_msgs"])
        for name in ("all", "vip_sst", "vip_tt"):
            for k, v in out[name].items():
                assert v.tobytes() == res[0][1][name][k].tobytes(), (rank, name, k)
        inside(out["all"], yld, bars, f"sharded rank {rank}")
        inside(out["vip_sst"], yld, bars, f"sharded rank {rank} [VIP alone]")
        inside(out["vip_tt"], vld, dict(VIP=tbar), f"sharded rank {rank} [VIP from tt]")


# ---- long leading dimensions ------------------------------------------------------------------------------------------------------------
from test_gpu_long_ld import arena  # noqa: E402,F401  (the module-scoped arena fixture)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_long_leading_dimension(arena, oracle, dt):   # noqa: F811
    """X with its last column beginning beyond 2^31 elements, built as XDIAG_CASES of tests/test_gpu_long_ld.py are: inside the
    bars, the arena untouched around it, and its compact twin inside the bars as well"""
    from pls_amd import _lib as L
    from test_gpu_long_ld import _both, _cached, _code, _ldv, _ptr, _round, _tdt, case_ld
    import pls_amd
    torch = _torch()
    f64 = torch.float64
    N, K, M, A = 300, 2050, 1, 8
    ld = case_ld("total", dt, K)
    assert (K - 1) * ld > 1 << 31
    Xh = _round(oracle.synth_x(0, N, K), dt)
    fit = _cached(("vd", N, K, A), lambda: oracle.plsr(oracle.synth_x(0, N, K), oracle.synth_y(0, N, M), A))
    m = {}
    for k in "WRP":
        m[k] = pls_amd.colmajor_empty(K, A, f64, "cuda", ld=K); m[k].copy_(torch.from_numpy(np.asfortranarray(fit[k])))
    m["Q"] = pls_amd.colmajor_empty(M, A, f64, "cuda", ld=M); m["Q"].copy_(torch.from_numpy(np.asfortranarray(fit["Q"])))

    def call(h, lay):
        X = lay.inp("X", Xh, dtype=_tdt(dt))
        o = dict(ssxk=pls_amd.colmajor_empty(K, A + 1, f64, "cuda"), VIP=pls_amd.colmajor_empty(K, A, f64, "cuda"),
                 sst=torch.empty(A, dtype=f64, device="cuda"))
        L.check(L.lib().pls_hip_var_diagnostics(h.h, _ptr(X), _ldv(X), N, K, M, A, _ptr(m["W"]), _ptr(m["R"]), _ptr(m["P"]), _ptr(m["Q"]), None,
                                                _code(dt), _ptr(o["ssxk"]), _ldv(o["ssxk"]), _ptr(o["VIP"]), _ldv(o["VIP"]), _ptr(o["sst"])), h.h)
        h.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, "X", lambda lay: call(h, lay))
    yld = vardiag_yardstick(Xh, fit["W"], fit["R"], fit["P"], fit["Q"], dtype=np.longdouble)
    bars = vardiag_bars(Xh, fit["R"], fit["P"], yld, M)
    inside(got, yld, bars, f"long ld {N}x{K} {dt}")
    inside(twin, yld, bars, "its compact twin")


# ---- Model ----------------------------------------------------------------------------------------------------------------------------
def test_model_vip_and_r2x_by_variable(handle, oracle):
    """Model.vip() and Model.r2x_by_variable() against the yardstick of the device's own model: after KERNEL_TYPE1 tt comes from T
    (no pass over X), after KERNEL_TYPE2 from the call's scores; a missing=True model gives vip from its T and refuses
    r2x_by_variable"""
    import pls_amd
    N, K, M, A = 3000, 64, 4, 8
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    Xn = oracle.synth_x(N, 500, K)
    for method in (pls_amd.KERNEL_TYPE1, pls_amd.KERNEL_TYPE2):
        mdl = pls_amd.Model(to_dev(Xh), to_dev(Yh), method, A, handle=handle)
        own = {k: getattr(mdl, k).cpu().numpy() for k in "WRPQ"}
        tt = None if method == pls_amd.KERNEL_TYPE2 else (mdl.T.cpu().numpy().astype(np.float64) ** 2).sum(0)
        yld = vardiag_yardstick(Xh, own["W"], own["R"], own["P"], own["Q"], tt=tt, dtype=np.longdouble)
        bars = vardiag_bars(Xh, own["R"], own["P"], yld, M, tt_given=tt is not None)
        vip = mdl.vip(); r2 = mdl.r2x_by_variable(); handle.synchronize()
        assert tuple(vip.shape) == (K, A) and tuple(r2.shape) == (K, A)
        inside({"VIP": vip.cpu().numpy()}, yld, bars, f"Model.vip method {method}")
        ss = np.asarray(yld["ssxk"], dtype=np.float64)
        tol = (bars["ssxk"][:, 1:] + bars["ssxk"][:, :1] * ss[:, 1:] / ss[:, :1]) / ss[:, :1] + 4 * 2.0 ** -52
        assert np.all(np.abs(r2.cpu().numpy() - (1 - ss[:, 1:] / ss[:, :1])) <= tol), method
        ynew = vardiag_yardstick(Xn, own["W"], own["R"], own["P"], own["Q"], dtype=np.longdouble)
        bnew = vardiag_bars(Xn, own["R"], own["P"], ynew, M)
        sn = np.asarray(ynew["ssxk"], dtype=np.float64)
        tol = (bnew["ssxk"][:, 1:] + bnew["ssxk"][:, :1] * sn[:, 1:] / sn[:, :1]) / sn[:, :1] + 4 * 2.0 ** -52
        assert np.all(np.abs(mdl.r2x_by_variable(to_dev(Xn)).cpu().numpy() - (1 - sn[:, 1:] / sn[:, :1])) <= tol), method
    # numpy in, numpy out
    mh = pls_amd.Model(Xh, Yh, pls_amd.KERNEL_TYPE1, A, handle=handle)
    assert isinstance(mh.vip(), np.ndarray) and mh.r2x_by_variable(Xn).shape == (K, A)
    # a missing-value model: vip from its own T, no per-variable R^2 X
    Xm = np.array(Xh[:500]); Xm[::7, 3] = np.nan; Xm[5::11, 40] = np.nan
    mm = pls_amd.Model(to_dev(Xm), to_dev(Yh[:500]), pls_amd.KERNEL_TYPE1, 4, handle=handle, missing=True)
    own = {k: getattr(mm, k).cpu().numpy() for k in "WQ"}
    tt = (mm.T.cpu().numpy().astype(np.float64) ** 2).sum(0)
    vld = vardiag_yardstick(None, own["W"], None, None, own["Q"], tt=tt, dtype=np.longdouble)
    v = mm.vip(); handle.synchronize()
    inside({"VIP": v.cpu().numpy()}, vld, dict(VIP=np.full((K, 4), (K + M + 2 * 4 + 16) * 2.0 ** -52)), "Model.vip missing=True")
    with pytest.raises(pls_amd.PlsHipError) as e:
        mm.r2x_by_variable()
    assert e.value.code == 4   # PLS_HIP_ERR_UNSUPPORTED
