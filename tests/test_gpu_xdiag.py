"""pls_hip_x_diagnostics on the MI355X: Q residuals, Hotelling T^2, scores, ssx, sst against the longdouble yardstick of
tests/test_xdiag_ref.py with the worst-case bars derived there (u = 2^-52 for fp64 AND fp32 storage: the scores stay fp64
inside the library).  Every case prints the device's worst distance in units of u * envelope; the table of a whole run
is printed and, when PLS_XDIAG_ACCURACY_FILE names a file, written there (the source of profiles/xdiag/accuracy.txt).

The general two-sweep route is the only route this library has (no fused one-sweep route was built), so there is no
second route to compare.
"""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT
from test_gpu_parity import to_dev
from test_xdiag_ref import U, nir_z, total_bars, xdiag_bars, xdiag_yardstick

pytestmark = pytest.mark.gpu

ACCURACY = []   # (case, N, K, A, worst Q / (u ENVQ), worst T2 / (u ENVT), worst S / (u e))


def _torch():
    import torch
    return torch


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _units(err, env):
    """worst err / (u * env) over the entries with a non-zero envelope"""
    env = np.asarray(env, dtype=np.float64)
    ok = env > 0
    return float((np.asarray(err, dtype=np.float64)[ok] / (U * env[ok])).max()) if ok.any() else 0.0


def check_outputs(label, got, X, R, P, tvar=None, n_total=None, rows=None, record=True, pre=None):
    """every output in `got` (dict of device tensors / numpy arrays) against the longdouble yardstick of X (the rows of this
    call), inside the bars; `rows`: the totals ssx / sst belong to this larger matrix (sharded calls), given as its yardstick
    (ref, bars, N).  pre: the (yardstick, bars) an earlier call on the same inputs returned.  Returns that pair."""
    X = np.asarray(X, dtype=np.float64)
    N, K = X.shape
    A = R.shape[1]
    if pre is None:
        ref = xdiag_yardstick(X, R, P, tvar=tvar, n_total=n_total, dtype=np.longdouble)
        bars = xdiag_bars(X, R, P, np.asarray(ref["tvar"], dtype=np.float64))
    else:
        ref, bars = pre
    fig = {}
    for k, env in (("S", "e"), ("Q", "envq"), ("T2", "envt")):
        if k not in got:
            continue
        g = _np(got[k])
        assert g.shape == (N, A), (label, k, g.shape)
        if k == "S" and g.dtype == np.float32:   # an fp32 OUTPUT: the yardstick rounded to fp32, +- 1 ulp
            want = np.asarray(ref["S"], dtype=np.float64).astype(np.float32)
            ulp = np.spacing(np.abs(want))
            bad = np.abs(g.astype(np.float64) - want.astype(np.float64)) > ulp
            assert not bad.any(), (label, "S fp32", int(bad.sum()))
            continue
        finite = np.isfinite(bars[k])
        err = np.abs(g.astype(np.longdouble) - ref[k]).astype(np.float64)
        fig[k] = _units(err[finite], bars[env][finite])
        print(f"{label}: worst {k} error {fig[k]:.2f} u*{env} (bar {bars[k][finite].max() / (U * bars[env][finite].max()):.0f})")
        assert np.all(err[finite] <= bars[k][finite]), (label, k, fig[k])
    if rows is None:
        tref, tbars, tn = ref, bars, N
    else:
        tref, tbars, tn = rows
    bx, bt = total_bars(tbars, tref, tn, K)
    if "ssx" in got:
        err = np.abs(_np(got["ssx"]).astype(np.longdouble) - tref["ssx"]).astype(np.float64)
        print(f"{label}: ssx error / bar {np.max(err / bx):.3g}")
        assert np.all(err <= bx), (label, "ssx", err, bx)
    if "sst" in got:
        err = np.abs(_np(got["sst"]).astype(np.longdouble) - tref["sst"]).astype(np.float64)
        print(f"{label}: sst error / bar {np.max(err / bt):.3g}")
        assert np.all(err <= bt), (label, "sst", err, bt)
    if record and fig:
        ACCURACY.append((label, N, K, A, fig.get("Q", float("nan")), fig.get("T2", float("nan")), fig.get("S", float("nan"))))
    return ref, bars


ALL = ("Q", "T2", "S", "ssx", "sst")


def run_case(handle, label, Xh, R, P, tvar=None, dtype=None):
    """device memory: all outputs, twice (same bits); host memory; each output alone -- all inside the bars"""
    torch = _torch()
    X = to_dev(Xh, dtype)
    Rd, Pd = to_dev(R), to_dev(P)
    a = handle.x_diagnostics(X, Rd, Pd, tvar=tvar, want=ALL); handle.synchronize()
    a = {k: v.clone() for k, v in a.items()}
    b = handle.x_diagnostics(X, Rd, Pd, tvar=tvar, want=ALL); handle.synchronize()
    for k in ALL:
        assert torch.equal(a[k], b[k]), (label, k, "two calls with the same arguments differ")
    ref, bars = check_outputs(label, a, Xh, R, P, tvar=tvar)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    hst = handle.x_diagnostics(np.asfortranarray(Xh, dtype=npdt), R, P, tvar=tvar, want=ALL)
    check_outputs(label + " [host memory]", hst, Xh, R, P, tvar=tvar, record=False, pre=(ref, bars))
    for k in ALL:
        one = handle.x_diagnostics(X, Rd, Pd, tvar=tvar, want=(k,)); handle.synchronize()
        assert set(one) == {k}
        check_outputs(label + f" [{k} alone]", one, Xh, R, P, tvar=tvar, record=False, pre=(ref, bars))
    return a, (ref, bars)


# ---- the cases of the feature request ------------------------------------------------------------------------------

def test_nir_training_and_new_rows(handle, oracle, po):
    X, Y = nir_z(po)
    ref = oracle.plsr(X, Y, 10)
    a, pre = run_case(handle, "nir train", X, ref["R"], ref["P"])
    r2x = 1.0 - _np(a["ssx"])[1:] / _np(a["ssx"])[0]
    assert np.allclose(r2x, [0.650, 0.835, 0.937, 0.963, 0.982, 0.986, 0.988, 0.989, 0.990, 0.992], atol=6e-4)
    # tvar = None on training data against passing sst / (N - 1) back in
    tv = _np(a["sst"]) / (X.shape[0] - 1)
    back = handle.x_diagnostics(to_dev(X), to_dev(ref["R"]), to_dev(ref["P"]), tvar=tv, want=ALL); handle.synchronize()
    check_outputs("nir train [tvar passed back]", back, X, ref["R"], ref["P"], record=False, pre=pre)
    # fit on rows 0-44, diagnostics of rows 45-59 with the tvar of the fit
    fit = oracle.plsr(X[:45], Y[:45], 10)
    tvar = (fit["T"] ** 2).sum(0) / 44
    run_case(handle, "nir new rows 45-59", X[45:], fit["R"], fit["P"], tvar=tvar)


SYNTH = [("synth 4097x513 m1 train", 4097, 513, 1, 12), ("synth 3000x64 m4", 3000, 64, 4, 20),
         ("synth 1000x7 m4 A=K", 1000, 7, 4, 7), ("synth 9x7 m1", 9, 7, 1, 3), ("synth 2048x200 m2 A=100", 2048, 200, 2, 100),
         ("synth 65537x512 m1", 65537, 512, 1, 20), ("synth 300x4096 m1 (short, wide)", 300, 4096, 1, 8)]


@pytest.mark.parametrize("label,N,K,M,A", SYNTH, ids=[s[0].split()[1] for s in SYNTH])
def test_synthetic_training(handle, oracle, label, N, K, M, A):
    X, Y = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    ref = oracle.plsr(X, Y, A)
    run_case(handle, label, X, ref["R"], ref["P"])


def test_synthetic_new_rows(handle, oracle):
    N, K, A = 4097, 513, 12
    X, Y = oracle.synth_x(0, N, K), oracle.synth_y(0, N, 1)
    ref = oracle.plsr(X, Y, A)
    tvar = (ref["T"] ** 2).sum(0) / (N - 1)
    run_case(handle, "synth 4097x513 new rows", oracle.synth_x(4097, 1001, K), ref["R"], ref["P"], tvar=tvar)


def test_fp32_storage(handle, oracle):
    """X in fp32 storage is exact in fp64; the scores stay fp64 inside the library, so the fp64 bars hold; the S OUTPUT is
    fp32: the yardstick rounded, +- 1 ulp"""
    torch = _torch()
    N, K, A = 4097, 64, 10
    X = np.asfortranarray(oracle.synth_x(0, N, K).astype(np.float32).astype(np.float64))
    Y = oracle.synth_y(0, N, 2)
    ref = oracle.plsr(X, Y, A)
    a, _ = run_case(handle, "synth 4097x64 m2 (fp32 storage)", X, ref["R"], ref["P"], dtype=torch.float32)
    assert a["S"].dtype == torch.float32
    # an unaligned fp32 matrix (odd ld): the one-row-per-lane forms
    Xd = torch.empty((K, N + 1), dtype=torch.float32, device="cuda")[:, :N].t()
    Xd.copy_(torch.from_numpy(X))
    b = handle.x_diagnostics(Xd, to_dev(ref["R"]), to_dev(ref["P"]), want=ALL); handle.synchronize()
    check_outputs("fp32 storage, odd ld", b, X, ref["R"], ref["P"], record=False)


def test_config3_shape(handle, oracle, po):
    """1,048,576 x 512, A = 20, the matrix made on the device: Q / T2 / S of four row blocks of 4,096 rows against the
    longdouble yardstick; ssx and sst of all rows against the yardstick evaluated block by block on the host -- its rows in
    fp64 (numpy), the totals accumulated in longdouble (the longdouble evaluation of 10^10 residual elements takes about an
    hour on a CPU; the fp64 rows sit within 8.1 u ENVQ of it on every case measured, the bar is 1584 u ENVQ)."""
    import pls_amd
    N, K, A = 1 << 20, 512, 20
    omp = po.OracleLib(omp=True)
    X = handle.synth_x(0, N, K, pls_amd.SEED_DEFAULT)
    Xh = omp.synth_x(0, N, K); Yh = omp.synth_y(0, N, 1)
    for r0 in (0, 777777, N - 100):
        assert np.array_equal(X[r0:r0 + 100].cpu().numpy(), Xh[r0:r0 + 100])
    ref = omp.plsr(Xh, Yh, A)
    R, P = ref["R"], ref["P"]
    a = handle.x_diagnostics(X, to_dev(R), to_dev(P), want=ALL); handle.synchronize()
    b = handle.x_diagnostics(X, to_dev(R), to_dev(P), want=ALL); handle.synchronize()
    for k in ALL:
        assert _torch().equal(a[k], b[k]), k
    ssx = np.zeros(A + 1, dtype=np.longdouble); sst = np.zeros(A, dtype=np.longdouble)
    bq = np.zeros(A); be = np.zeros(A)
    BL = 65536
    for r0 in range(0, N, BL):
        y = xdiag_yardstick_blas(Xh[r0:r0 + BL], R, P)
        ssx += y["ssx"].astype(np.longdouble); sst += y["sst"].astype(np.longdouble)
        bb = xdiag_bars(Xh[r0:r0 + BL], R, P, np.ones(A))
        bq += bb["Q"].sum(0); be += (2 * (K + 2) * U * bb["e"] ** 2).sum(0)
    tvar = np.asarray(sst / (N - 1), dtype=np.float64)
    bx = np.concatenate([[(K + N) * U * float(ssx[0])], bq + N * U * ssx[1:].astype(np.float64)])
    bt = be + N * U * sst.astype(np.float64)
    ex = np.abs(_np(a["ssx"]).astype(np.longdouble) - ssx).astype(np.float64)
    et = np.abs(_np(a["sst"]).astype(np.longdouble) - sst).astype(np.float64)
    print(f"config 3: ssx error / bar {np.max(ex / bx):.3g}, sst error / bar {np.max(et / bt):.3g}")
    assert np.all(ex <= bx) and np.all(et <= bt)
    for r0 in (0, 123456, 600000, N - 4096):
        got = {k: a[k][r0:r0 + 4096] for k in ("Q", "T2", "S")}
        check_outputs(f"config 3 rows {r0}..", got, Xh[r0:r0 + 4096], R, P, tvar=tvar)


def xdiag_yardstick_blas(X, R, P):
    """the fp64 yardstick with the scores from numpy's matrix product (rows of a large block)"""
    S = X @ R
    F = np.array(X)
    A = R.shape[1]
    ssx = np.zeros(A + 1)
    ssx[0] = (F * F).sum()
    for c in range(A):
        F -= np.outer(S[:, c], P[:, c])
        ssx[c + 1] = np.einsum("ij,ij->i", F, F).sum()
    return dict(ssx=ssx, sst=(S * S).sum(0))


# ---- layouts and guarded buffers -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("N,K,A,dt", [(1, 7, 3, "f64"), (9, 7, 3, "f64"), (1031, 64, 10, "f64"), (1031, 64, 10, "f32"),
                                      (4097, 130, 30, "f64"), (301, 1024, 5, "f64")])
def test_writes_exactly_its_outputs(handle, oracle, N, K, A, dt, layout, mem):
    """exactly N x A of Qres, T2, S, A + 1 of ssx and A of sst are written -- padded leading dimensions ("aligned") or
    ld == rows with every pointer 8 (4) bytes past a 16-byte boundary ("eigen"), one row, odd row counts, a component list
    in two ranges, the column split -- nothing in the padding, no input changed, values inside the bars"""
    import pls_amd
    from test_gpu_bounds import Guarded
    torch = _torch()
    Xh = oracle.synth_x(0, max(N, 64), K)
    ref = oracle.plsr(Xh, oracle.synth_y(0, max(N, 64), 1), A)
    Xh = np.asfortranarray(Xh[:N])
    if dt == "f32":
        Xh = np.asfortranarray(Xh.astype(np.float32).astype(np.float64))
    tvar = (ref["T"] ** 2).sum(0) / (ref["T"].shape[0] - 1)
    dev = "cuda" if mem == "device" else "numpy"
    tdt = (torch.float32 if dt == "f32" else torch.float64) if mem == "device" else (np.float32 if dt == "f32" else np.float64)
    f8 = torch.float64 if mem == "device" else np.float64
    gx = Guarded([(N, K)], tdt, layout, dev)
    gs = Guarded([(N, A)], tdt, layout, dev)
    gm = Guarded([(K, A, K), (K, A, K), (A, 1)], f8, layout, dev)
    go = Guarded([(N, A), (N, A), (A + 1, 1), (A, 1)], f8, layout, dev)

    def put(dst, a):
        if mem == "device":
            dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.dtype))
        else:
            dst[...] = a
    put(gx[0], Xh); put(gm[0], ref["R"]); put(gm[1], ref["P"]); put(gm[2], tvar[:, None])
    keep = [g.raw.clone() if mem == "device" else g.raw.copy() for g in (gx, gm)]
    for use_tvar in (True, False) if N >= 2 else (True,):
        go.refill(); gs.refill()
        rc = pls_amd.lib().pls_hip_x_diagnostics(handle.h, gx.ptr(0), gx.ld(0), N, N, K, A, gm.ptr(0), gm.ptr(1),
                                                 gm.ptr(2) if use_tvar else None, 1 if dt == "f32" else 0,
                                                 1 if mem == "device" else 0, go.ptr(0), go.ld(0), go.ptr(1), go.ld(1),
                                                 gs.ptr(0), gs.ld(0), go.ptr(2), go.ptr(3))
        assert rc == 0, pls_amd._lib.last_error(handle.h)
        handle.synchronize()
        for g in (gx, gs, gm, go):
            g.assert_untouched()
        go.assert_written(); gs.assert_written()
        for g, k in zip((gx, gm), keep):
            assert (g.raw == k).all(), "an input was written"
        got = {"Q": go[0], "T2": go[1], "S": gs[0], "ssx": go[2][:, 0], "sst": go[3][:, 0]}
        got = {k: (v.cpu().numpy() if mem == "device" else np.array(v)) for k, v in got.items()}
        check_outputs(f"guarded {N}x{K} A{A} {dt} {layout} {mem}", got, Xh, ref["R"], ref["P"],
                      tvar=tvar if use_tvar else None, record=False)


def test_bad_arguments(handle):
    """argument errors are PLS_HIP_ERR_INVALID before anything is touched"""
    import pls_amd
    torch = _torch()
    L = pls_amd.lib()
    N, K, A = 64, 6, 3
    X = torch.zeros(N * K, dtype=torch.float64, device="cuda"); R = torch.zeros(K * A, dtype=torch.float64, device="cuda")
    out = torch.full((2 * N * A + 3 * A + 1,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 8 * off)
    Q, T2, ssx, sst = p(out), p(out, N * A), p(out, 2 * N * A), p(out, 2 * N * A + A + 1)

    def call(X_=p(X), ldx=N, N_=N, nt=N, K_=K, A_=A, R_=p(R), P_=p(R), tv=None, dt=0, mem=1, ldq=N):
        return L.pls_hip_x_diagnostics(handle.h, X_, ldx, N_, nt, K_, A_, R_, P_, tv, dt, mem, Q, ldq, T2, N, None, N, ssx, sst)
    assert call() == 0
    handle.synchronize()
    out.fill_(7.0)
    assert call(X_=None) == 1 and call(ldx=N - 1) == 1 and call(A_=K + 1) == 1 and call(A_=0) == 1
    assert call(dt=2) == 1 and call(mem=7) == 1 and call(R_=None) == 1 and call(P_=None) == 1 and call(ldq=N - 1) == 1
    assert call(N_=1, nt=1) == 1                 # T2 from the call's own scores needs two rows
    assert call(N_=1, nt=1, tv=p(R)) == 0        # ... with a tvar it does not
    assert call(nt=N - 1) == 1 and call(N_=0) == 1
    handle.synchronize()
    assert bool((out[N * A + 1:N * A + N].eq(7.0)).all()), "a rejected call wrote"


# ---- sharded handle, group, Model, the C++ layer -----------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, world, port, N, K, A, splits, q):
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
        ref = ora.plsr(ora.synth_x(0, N, K), ora.synth_y(0, N, 1), A)
        row0, nrows = sum(splits[:rank]), splits[rank]
        X = h.synth_x(row0, nrows, K, pls_amd.SEED_DEFAULT)
        msgs = []
        attach_reducer(h, K, 1, post=lambda view, i: msgs.append(int(view.numel())))
        R = torch.from_numpy(ref["R"]).cuda(); P = torch.from_numpy(ref["P"]).cuda()
        res = {}
        for name, want in (("all", ("Q", "T2", "S", "ssx", "sst")), ("q_only", ("Q",))):
            del msgs[:]
            out = h.x_diagnostics(X, R, P, want=want, n_total=N)
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
    """a collective on a row-sharded handle: the rank's own rows of Q / T2 / S inside the bars of the yardstick's rows, ssx
    and sst bit-identical on all ranks and inside the bars, exactly ONE message of 8 (2A + 1) values per call -- also when
    only Q is asked for"""
    import torch.multiprocessing as mp
    N, K, A = sum(splits), 96, 9
    world = len(splits)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, N, K, A, splits, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
    assert not any("error" in r[1] for r in res), [r[1].get("error") for r in res]
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    Xh = oracle.synth_x(0, N, K)
    ref = oracle.plsr(Xh, oracle.synth_y(0, N, 1), A)
    full = xdiag_yardstick(Xh, ref["R"], ref["P"], dtype=np.longdouble)
    fbars = xdiag_bars(Xh, ref["R"], ref["P"], np.asarray(full["tvar"], dtype=np.float64))
    for rank, out in res:
        assert out["all_msgs"] == [8 * (2 * A + 1)] and out["q_only_msgs"] == [8 * (2 * A + 1)], (rank, out["all_msgs"])
        for k in ("ssx", "sst"):
            assert np.array_equal(out["all"][k], res[0][1]["all"][k]), (rank, k)
        r0 = sum(splits[:rank])
        rows = Xh[r0:r0 + splits[rank]]
        assert out["all"]["Q"].shape == (splits[rank], A)
        if splits[rank] == 0:
            check_outputs(f"sharded rank {rank} (empty)", {k: out["all"][k] for k in ("ssx", "sst")}, Xh, ref["R"], ref["P"],
                          record=False)
            continue
        tv = np.asarray(full["tvar"], dtype=np.float64)
        check_outputs(f"sharded rank {rank}", out["all"], rows, ref["R"], ref["P"], tvar=tv, rows=(full, fbars, N), record=False)
        check_outputs(f"sharded rank {rank} [Q alone]", out["q_only"], rows, ref["R"], ref["P"], tvar=tv, record=False)


@pytest.mark.parametrize("n", [1, 3])
def test_group(oracle, n):
    """pls_hip_group_x_diagnostics on resident matrices, 1 and 3 virtual members: downloads inside the bars"""
    import pls_amd
    N, K, A = 3001, 130, 11
    Xh = oracle.synth_x(0, N, K)
    ref = oracle.plsr(Xh, oracle.synth_y(0, N, 2), A)
    g = pls_amd.Group([0] * n)
    try:
        X = g.upload(Xh)
        for tvar in (None, (ref["T"] ** 2).sum(0) / (N - 1)):
            out = g.x_diagnostics(X, ref["R"], ref["P"], tvar=tvar, want=ALL)
            got = {k: (g.download(out[k]) if k in ("Q", "T2", "S") else out[k]) for k in ALL}
            check_outputs(f"group of {n}", got, Xh, ref["R"], ref["P"], tvar=tvar, record=False)
            for k in ("Q", "T2", "S"):
                g.free(out[k])
        only = g.x_diagnostics(X, ref["R"], ref["P"], want=("ssx",))
        check_outputs(f"group of {n} [ssx alone]", only, Xh, ref["R"], ref["P"], record=False)
        g.free(X)
    finally:
        g.close()


def test_model_kernel_type1_and_type2_agree(handle, oracle):
    """Model.x_diagnostics(): after KERNEL_TYPE1 tvar comes from T, after KERNEL_TYPE2 (no T) from one call on the training
    data; both inside the bars of the yardstick of the oracle's model, on the training data and on new rows"""
    import pls_amd
    N, K, A = 3000, 64, 8
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, 4)
    Xn = oracle.synth_x(N, 500, K)
    ref = oracle.plsr(Xh, Yh, A)
    tvar = (ref["T"] ** 2).sum(0) / (N - 1)
    for method in (pls_amd.KERNEL_TYPE1, pls_amd.KERNEL_TYPE2):
        m = pls_amd.Model(to_dev(Xh), to_dev(Yh), method, A, handle=handle)
        assert (m.T is None) == (method == pls_amd.KERNEL_TYPE2)
        for X, tv in ((None, None), (to_dev(Xn), tvar)):
            d = m.x_diagnostics(X); handle.synchronize()
            Xc = Xh if X is None else Xn
            y = xdiag_yardstick(Xc, ref["R"], ref["P"], tvar=tv, dtype=np.longdouble)
            # (the model is the DEVICE's fit: its R, P differ from the oracle's by the fit's own rounding, 1e-10 by the
            # project's parity bar; what is compared at the bars is the diagnostics of the device's own model)
            R, P = m.R.cpu().numpy(), m.P.cpu().numpy()
            own_tv = _np(m._tvar())
            check_outputs(f"Model method {method}", {"Q": d["Q"], "T2": d["T2"]}, Xc, R, P, tvar=own_tv, record=False)
            assert np.allclose(_np(d["R2X"]), np.asarray(1 - y["ssx"][1:] / y["ssx"][0], dtype=np.float64), atol=1e-9)
            assert np.allclose(_np(d["Q"]), np.asarray(y["Q"], dtype=np.float64), rtol=0, atol=1e-8 * float(np.max(y["Q"][:, 0])))
    # numpy in, numpy out
    mh = pls_amd.Model(Xh, Yh, pls_amd.KERNEL_TYPE1, A, handle=handle)
    d = mh.x_diagnostics(Xn)
    assert isinstance(d["Q"], np.ndarray) and d["Q"].shape == (500, A)
    check_outputs("Model host", {"Q": d["Q"], "T2": d["T2"]}, Xn, mh.R, mh.P, tvar=mh._tvar(), record=False)


def test_cpp_program():
    exe = os.path.join(ROOT, "tests", "cpp", "x_diagnostics")
    assert os.path.exists(exe), "tests/cpp/x_diagnostics not built (build() makes it through pls_amd/host/Makefile)"
    for devices in ("1", "3"):
        env = dict(os.environ, PLS_HIP_DEVICES="0,0,0" if devices == "3" else "0")
        r = subprocess.run([exe, os.path.join(DATA, "nir.csv"), os.path.join(DATA, "octane.csv"), "10"], capture_output=True,
                           text=True, timeout=300, env=env)
        assert r.returncode == 0 and "x_diagnostics: ok" in r.stdout, r.stdout + r.stderr


def test_zz_write_accuracy_table():
    """the figures of this run, in units of u * envelope, for profiles/xdiag/accuracy.txt"""
    if not ACCURACY:   # (run on its own: nothing to tabulate)
        return
    lines = [f"{'case':44s} {'N':>8s} {'K':>5s} {'A':>4s}  Q err/(u ENVQ) | bar   T2 err/(u ENVT) | bar   S err/(u e) | bar"]
    for label, N, K, A, fq, ft, fs in ACCURACY:
        lines.append(f"{label:44s} {N:8d} {K:5d} {A:4d}  {fq:8.2f} {3 * K + 2 * A + 8:10d}   {ft:8.2f} {2 * K + 2 * A + 8:11d}   "
                     f"{fs:6.2f} {K + 2:8d}")
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("PLS_XDIAG_ACCURACY_FILE")
    if out:
        with open(out, "w") as f:
            f.write(text)
