"""pls_hip_validation on the device against the numpy yardstick of tests/test_validation_ref.py.

D (the Wilcoxon signed-rank sums) must equal the yardstick EXACTLY on both routes -- one workgroup per pair sorting in LDS,
and the streaming radix sort -- for every shape, with and without ties; PRESS within nobs * 2^-52 relative of the exact sum
(the a-priori bound of any summation order of non-negative terms plus the rounding of each square); the reference column and
the picks equal; probw within 1e-14 absolute (D is exact, what follows is a dozen fp64 operations on values in [0, 1]).
Every comparison is preceded by the preconditions on the yardstick alone (no ties unless the case is about ties, separated
PRESS minimum, no probw within 1e-6 of alpha): a failed precondition fails the test.
"""
import ctypes
import io
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT
from test_gpu_bounds import Guarded
from test_validation_ref import EPS, check_preconditions, probw_from_d, summary_ref, synth_residuals

pytestmark = pytest.mark.gpu
ALPHA = 0.1
PROBW_TOL = 1e-14

_cache = {}


def _torch():
    import torch
    return torch


def _case(M, nobs, A, seed):
    """(E, yardstick summary) of the generator, preconditions asserted; computed once per shape"""
    key = (M, nobs, A, seed)
    if key not in _cache:
        E = synth_residuals(M, nobs, A, seed)
        s = summary_ref(E, ALPHA)
        check_preconditions(E, s, ALPHA)
        _cache[key] = (E, s)
    return _cache[key]


def _to_device(E):
    """numpy (M, nobs, A) -> the view Handle.cv_folds returns: (M, nobs, A) over (M, A, nobs) contiguous storage"""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(E.transpose(0, 2, 1))).cuda().permute(0, 2, 1)


def _to_host(E):
    return np.ascontiguousarray(E.transpose(0, 2, 1)).transpose(0, 2, 1)


def _np(out):
    return tuple(o.cpu().numpy() if not isinstance(o, np.ndarray) else o for o in out)


def _route(h, rows):
    import pls_amd
    h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, rows)


@pytest.fixture()
def vh(handle):
    """the session handle with the route switch back at the device's default afterwards"""
    import pls_amd
    default = _lds_default(handle)
    yield handle
    handle.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, default)
    handle.set_option(pls_amd.OPT_PROFILE, 0)


_default = {}


def _lds_default(handle):
    import pls_amd
    if "v" not in _default:  # read once, before any test lowers it
        _default["v"] = handle.get_option(pls_amd.OPT_VALIDATION_LDS_ROWS)
    return _default["v"]


def _compare(out, E, s, what):
    from pls_amd.model import pick_components
    press, D, probw, ref = _np(out)
    ps, rs, Ds, ws, bs = s
    M, nobs, A = E.shape
    rel = np.abs(press - ps) / ps
    below = np.array([[alt < rs[m] for alt in range(A)] for m in range(M)])
    perr = np.abs(probw - ws)[below].max() if below.any() else 0.0
    print(f"[validation] {what}: max PRESS rel err {np.nanmax(rel):.3e} (bound {nobs * EPS:.3e}), max |probw - ref| {perr:.3e}, "
          f"ref {ref.tolist()}, pairs {int(below.sum())}")
    assert np.array_equal(ref, rs), (what, ref, rs)
    assert (rel <= nobs * EPS).all(), (what, float(rel.max()))
    for m in range(M):
        for alt in range(A):
            if alt < rs[m]:
                assert D[m, alt] == float(Ds[m, alt]) and int(D[m, alt]) == Ds[m, alt], (what, m, alt, D[m, alt], Ds[m, alt])
            else:
                assert D[m, alt] == 0.0 and np.isnan(probw[m, alt]), (what, m, alt)
    assert perr <= PROBW_TOL, (what, perr)
    assert np.array_equal(pick_components(probw, ref, ALPHA), bs), what
    return press, D, probw, ref


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


SMALL = [(1, 1, 4, 1), (2, 2, 5, 1), (2, 63, 6, 1), (2, 64, 6, 1), (2, 65, 6, 2), (1, 60, 10, 1), (3, 1000, 12, 2),
         (2, 4096, 20, 3), (2, 4097, 20, 4)]
LARGE = [(4, 65537, 6, 5), (1, 300000, 8, 6), (1, 3000000, 6, 7)]


@pytest.mark.parametrize("route", ["default", "stream"])
@pytest.mark.parametrize("M,nobs,A,seed", SMALL, ids=[f"{m}x{n}x{a}" for m, n, a, _ in SMALL])
def test_small_shapes_on_both_routes(vh, M, nobs, A, seed, route):
    """assertions 1, 3, 4, 5: exact D, PRESS bound, ref, probw, picks; repeatable bits; host memory against device memory"""
    E, s = _case(M, nobs, A, seed)
    _route(vh, _lds_default(vh) if route == "default" else 0)
    Ed = _to_device(E)
    first = _compare(vh.validation(Ed), E, s, f"{M}x{nobs}x{A} {route} device")
    again = _np(vh.validation(Ed))
    assert _same_bits(first, again), "two device calls differ"
    host = _compare(vh.validation(_to_host(E)), E, s, f"{M}x{nobs}x{A} {route} host")
    assert _same_bits(host, _np(vh.validation(_to_host(E)))), "two host calls differ"
    assert _same_bits(first[1:], host[1:]), "D / probw / ref differ between host and device memory"
    assert (np.abs(first[0] - host[0]) <= nobs * EPS * first[0]).all()


@pytest.mark.parametrize("M,nobs,A,seed", LARGE, ids=[f"{m}x{n}x{a}" for m, n, a, _ in LARGE])
def test_long_columns(vh, M, nobs, A, seed):
    """the streaming route at its own sizes (up to 3 M rows per column), device memory twice and host memory once"""
    E, s = _case(M, nobs, A, seed)
    assert nobs > _lds_default(vh)
    Ed = _to_device(E)
    first = _compare(vh.validation(Ed), E, s, f"{M}x{nobs}x{A} device")
    assert _same_bits(first, _np(vh.validation(Ed)))
    host = _compare(vh.validation(_to_host(E)), E, s, f"{M}x{nobs}x{A} host")
    assert _same_bits(first[1:], host[1:])


def test_route_threshold_straddled(vh):
    """nobs = T and T + 1 for the T pls_hip_get_option reports: both exact, and the launch count shows that T is the
    last length the one-workgroup route takes (PRESS finish + one sort launch) and T + 1 the first that streams"""
    import pls_amd
    T = _lds_default(vh)
    assert T >= 1024
    with pytest.raises(pls_amd.PlsHipError) as e:
        vh.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, T + 1)
    assert e.value.code == 1
    launches = {}
    for nobs in (T - 1, T, T + 1):
        E, s = _case(1, nobs, 5, 11)
        vh.set_option(pls_amd.OPT_PROFILE, 2)
        vh.timing()
        out = vh.validation(_to_device(E))
        t = vh.timing()
        vh.set_option(pls_amd.OPT_PROFILE, 0)
        _compare(out, E, s, f"threshold nobs={nobs}")
        launches[nobs] = t["launches"]["small"]
        assert t["launches"]["xty"] == 1 and t["bytes"]["xty"] == 5 * nobs * 8
    assert launches[T - 1] == 2 and launches[T] == 2 and launches[T + 1] > 2, launches
    # lowered: the same column streams
    vh.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, 100)
    assert vh.get_option(pls_amd.OPT_VALIDATION_LDS_ROWS) == 100
    E, s = _case(2, 100, 6, 12)
    _compare(vh.validation(_to_device(E)), E, s, "lowered threshold, nobs=100 (LDS)")
    E, s = _case(2, 101, 6, 12)
    _compare(vh.validation(_to_device(E)), E, s, "lowered threshold, nobs=101 (stream)")


@pytest.mark.parametrize("route", ["default", "stream"])
@pytest.mark.parametrize("nobs", [65, 1001, 4097])
def test_unaligned_odd_columns(vh, nobs, route):
    """E at an address 8 but not 16 bytes aligned, odd nobs: every second column starts off a 16-byte boundary"""
    torch = _torch()
    from pls_amd import _lib as L
    M, A = 2, 6
    E, s = _case(M, nobs, A, 21)
    _route(vh, _lds_default(vh) if route == "default" else 0)
    ge = Guarded([(nobs, M * A)], torch.float64, "eigen", "cuda")
    assert ge.ptr(0).value % 16 == 8 and ge.ld(0) == nobs
    ge[0].copy_(torch.from_numpy(np.ascontiguousarray(E.transpose(1, 0, 2).reshape(nobs, M * A))).cuda())
    before = ge.bits(0).clone()
    go = Guarded([(M, A), (M, A), (M, A), (M, 1)], torch.float64, "eigen", "cuda")
    rc = L.lib().pls_hip_validation(vh.h, ge.ptr(0), nobs, A, M, L.MEM_DEVICE, go.ptr(0), go.ptr(1), go.ptr(2), go.ptr(3))
    L.check(rc, vh.h)
    vh.synchronize()
    go.check(); ge.assert_untouched()
    assert bool((ge.bits(0) == before).all()), "E was modified"
    out = (go[0].cpu().numpy(), go[1].cpu().numpy(), go[2].cpu().numpy(), go.bits(3).cpu().numpy()[:, 0])
    _compare(out, E, s, f"unaligned nobs={nobs} {route}")


@pytest.mark.parametrize("route", ["default", "stream"])
def test_ties(vh, route):
    """assertion 2: residuals rounded to two decimals (many equal |del|, many zeros): D exact against the STABLE yardstick;
    a reference column that equals an alternative on all rows but four whose signed ranks cancel: D = 0 and probw the
    formula at D = 0"""
    _route(vh, _lds_default(vh) if route == "default" else 0)
    for (M, nobs, A, seed) in [(2, 500, 8, 31), (1, 5000, 6, 32)]:
        E = np.round(synth_residuals(M, nobs, A, seed), 2)
        s = summary_ref(E, ALPHA)
        check_preconditions(E, s, ALPHA, ties_expected=True)
        ties = sum(nobs - len(np.unique(np.abs(np.abs(E[m, :, s[1][m]]) - np.abs(E[m, :, alt]))))
                   for m in range(M) for alt in range(s[1][m]))
        assert ties > nobs // 10, "the tie case has hardly any ties"
        out = _compare(vh.validation(_to_device(E)), E, s, f"ties {M}x{nobs}x{A} {route} ({ties} tied rows)")
        host = _compare(vh.validation(_to_host(E)), E, s, f"ties host {route}")
        assert _same_bits(out[1:], host[1:])
    # Two columns that are identical row by row have the same PRESS, so the earlier one IS the reference column and the
    # pair is never formed.  The pair below is identical on all rows but four, where del = +0.1, -0.2, -0.3, +0.35: the
    # 773 zeros take the ranks 1..773, the four signed ranks cancel (774 - 775 - 776 + 777), and the alternative's PRESS
    # is larger by 0.3625.  D = 0, probw = the formula at D = 0.
    E = synth_residuals(1, 777, 7, 33)
    r = summary_ref(E, ALPHA)[1][0]
    assert r >= 2
    rows = [10, 200, 400, 700]
    E[0, :, 1] = E[0, :, r]
    E[0, rows, r] = 1.0
    E[0, rows, 1] = [0.9, -1.2, 1.3, -0.65]
    s = summary_ref(E, ALPHA)
    check_preconditions(E, s, ALPHA, ties_expected=True)
    assert s[1][0] == r and s[2][0, 1] == 0
    out = _compare(vh.validation(_to_device(E)), E, s, f"identical columns {route}")
    assert out[1][0, 1] == 0.0 and out[2][0, 1] == probw_from_d(0.0, 777) == 0.5


@pytest.mark.parametrize("route", ["default", "stream"])
def test_nan_columns(vh, route):
    """assertion 6: a NaN column above ref changes nothing below it; a NaN column at index 0 gives ref = 0 (nothing is < NaN)"""
    _route(vh, _lds_default(vh) if route == "default" else 0)
    M, nobs, A = 2, 900, 9
    E, s = _case(M, nobs, A, 41)
    clean = _compare(vh.validation(_to_device(E)), E, s, f"nan: clean {route}")
    En = E.copy()
    for m in range(M):
        assert s[1][m] + 1 < A
        En[m, :, s[1][m] + 1] = np.nan
    out = _np(vh.validation(_to_device(En)))
    assert np.array_equal(out[3], clean[3])
    for m in range(M):
        r = s[1][m]
        assert np.isnan(out[0][m, r + 1])
        assert np.array_equal(out[1][m, :r].view(np.int64), clean[1][m, :r].view(np.int64))
        assert np.array_equal(out[2][m, :r].view(np.int64), clean[2][m, :r].view(np.int64))
        assert np.array_equal(np.delete(out[0][m], r + 1).view(np.int64), np.delete(clean[0][m], r + 1).view(np.int64))
    E0 = E.copy()
    E0[:, :, 0] = np.nan
    for mem in ("device", "host"):
        out = _np(vh.validation(_to_device(E0) if mem == "device" else _to_host(E0)))
        vh.synchronize()
        assert out[3].tolist() == [0] * M and np.isnan(out[0][:, 0]).all() and np.isfinite(out[0][:, 1:]).all()
        assert (out[1] == 0).all() and np.isnan(out[2]).all()
    # one NaN row inside a pair: sign 0, ranked last -- what numpy's stable argsort does with it as well
    E1 = E.copy()
    E1[0, 17, 1] = np.nan
    s1 = summary_ref(E1, ALPHA)
    assert s1[1][0] == s[1][0] >= 2 and s1[2][0, 1] != s[2][0, 1]
    out = _np(vh.validation(_to_device(E1)))
    assert out[3][0] == s1[1][0] and all(int(out[1][0, alt]) == s1[2][0, alt] for alt in range(s1[1][0]))


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("route", ["default", "stream"])
def test_writes_exactly_its_outputs(vh, route, mem):
    """assertion 7: PRESS, D, probw, ref between guard cells: every cell written, no guard cell touched, E unchanged; NULL
    outputs accepted in every combination"""
    torch = _torch()
    from pls_amd import _lib as L
    M, nobs, A = 3, 333, 7
    E, s = _case(M, nobs, A, 51)
    _route(vh, _lds_default(vh) if route == "default" else 0)
    dev = "cuda" if mem == "device" else "numpy"
    dt = torch.float64 if mem == "device" else np.float64
    flat = np.ascontiguousarray(E.transpose(1, 0, 2).reshape(nobs, M * A))
    ge = Guarded([(nobs, M * A)], dt, "eigen", dev)
    if mem == "device":
        ge[0].copy_(torch.from_numpy(flat).cuda())
        before = ge.bits(0).clone()
    else:
        ge[0][...] = flat
        before = ge.bits(0).copy()
    code = L.MEM_DEVICE if mem == "device" else L.MEM_HOST
    for mask in (0b1111, 0b0001, 0b1000, 0b0110, 0b0100, 0b0000):
        go = Guarded([(M, A), (M, A), (M, A), (M, 1)], dt, "eigen", dev)
        ptrs = [go.ptr(i) if mask >> i & 1 else None for i in range(4)]
        rc = L.lib().pls_hip_validation(vh.h, ge.ptr(0), nobs, A, M, code, *ptrs)
        L.check(rc, vh.h)
        vh.synchronize()
        go.assert_untouched()
        for i in range(4):
            if mask >> i & 1:
                go.assert_written(i)
            else:
                go.assert_prefilled(i)
        same = (ge.bits(0) == before)
        assert bool(same.all()), "E was modified"
        ge.assert_untouched()
        if mask == 0b1111:
            get = (lambda a: a.cpu().numpy()) if mem == "device" else np.asarray
            _compare((get(go[0]), get(go[1]), get(go[2]), get(go.bits(3))[:, 0]), E, s, f"guarded {route} {mem}")


def test_invalid_arguments(vh):
    from pls_amd import _lib as L
    E = _to_device(synth_residuals(1, 16, 3, 0))
    p = E.permute(0, 2, 1).data_ptr()
    f = L.lib().pls_hip_validation
    assert f(vh.h, p, 0, 3, 1, L.MEM_DEVICE, None, None, None, None) == L.ERR_INVALID
    assert f(vh.h, p, 16, 0, 1, L.MEM_DEVICE, None, None, None, None) == L.ERR_INVALID
    assert f(vh.h, p, 16, 3, 0, L.MEM_DEVICE, None, None, None, None) == L.ERR_INVALID
    assert f(vh.h, None, 16, 3, 1, L.MEM_DEVICE, None, None, None, None) == L.ERR_INVALID
    assert f(vh.h, p, 16, 3, 1, 7, None, None, None, None) == L.ERR_INVALID
    assert f(vh.h, p, 16, 3, 1, L.MEM_DEVICE, None, None, None, None) == L.OK
    # A = 1: no alternative exists
    press, D, probw, ref = _np(vh.validation(_to_device(synth_residuals(2, 50, 1, 1))))
    assert ref.tolist() == [0, 0] and (D == 0).all() and np.isnan(probw).all() and (press > 0).all()


# ---- Python Model ---------------------------------------------------------------------------------------------------------
def _zs(a):
    return (a - a.mean(0)) / a.std(0, ddof=1)


def _csv(name):
    return np.loadtxt(os.path.join(DATA, name), delimiter=",", ndmin=2)


@pytest.mark.parametrize("data,A", [("nir", 10), ("toy", 4)])
@pytest.mark.parametrize("mem", ["device", "host"])
def test_model_selection_on_real_residuals(vh, data, A, mem):
    """assertion 8: leave-one-out residuals of the reference's example data through Model.optimal_num_components,
    validation and print_validation, against the yardstick on the same E"""
    import pls_amd
    torch = _torch()
    X, Y = (_zs(_csv("nir.csv")), _zs(_csv("octane.csv"))) if data == "nir" else (_zs(_csv("toyX.csv")), _zs(_csv("toyY.csv")))
    if mem == "device":
        Xd, Yd = (pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(a)).cuda()) for a in (X, Y))
    else:
        Xd, Yd = X, Y
    model = pls_amd.Model(Xd, Yd, pls_amd.KERNEL_TYPE1, A, handle=vh)
    E = model.cv_LOO()
    Eh = E.cpu().numpy() if mem == "device" else np.asarray(E)
    s = summary_ref(Eh, ALPHA)
    check_preconditions(Eh, s, ALPHA)
    best = model.optimal_num_components(E)
    print(f"[validation] {data} A={A} {mem}: PRESS minimum at {(s[1] + 1).tolist()} components, picks {best.tolist()}, "
          f"probw {[round(float(v), 4) for v in s[3][0][:s[1][0]]]}")
    assert np.array_equal(best, s[4])
    _compare(vh.validation(E), Eh, s, f"{data} LOO {mem}")
    if data == "nir":
        assert s[1].tolist() == [6] and best.tolist() == [3]  # minimum at 7 components, pick 3
    else:
        assert (s[1] + 1).tolist() == [3, 1] and best.tolist() == [2, 1]
    nobs = Eh.shape[1]
    ress, mse = (model.validation(E, t) for t in (pls_amd.RESS, pls_amd.MSE))
    ress, mse = _np((ress, mse))
    # (a division and a multiplication, or a reciprocal and two multiplications: at most 2 ulp)
    assert np.allclose(mse * nobs, ress, rtol=4 * EPS, atol=0)
    buf = io.StringIO()
    model.print_validation(E, "LOO", pls_amd.MSE, file=buf)
    lines = buf.getvalue().splitlines()
    M = Eh.shape[0]
    assert lines[0] == "LOO Validation:"
    assert lines[1] == "RMSE  Matrix (rows = Y variable; cols = # of components):"
    rows = np.array([[float(t) for t in ln.split()] for ln in lines[2:2 + M]])
    assert np.allclose(rows, np.sqrt(mse), rtol=1e-5)
    assert lines[2 + M] == "Optimal number of components (by Y variable):\t" + " ".join(str(b) for b in best.tolist())
    assert len(lines) == 3 + M
    buf = io.StringIO()
    model.print_validation(E, "LOO", pls_amd.RESS, file=buf)
    assert buf.getvalue().splitlines()[1].startswith("PRESS  Matrix")


# ---- a row-sharded handle: the call is local ------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_worker(rank, port, q, Xh, Yh, splits, A):
    world = len(splits)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    from datetime import timedelta

    import torch
    import torch.distributed as dist
    import pls_amd
    from pls_amd.distributed import attach_reducer
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        torch.cuda.set_device(0)
        h = pls_amd.Handle()
        row0 = sum(splits[:rank])
        n = splits[rank]
        X = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(Xh[row0:row0 + n])).cuda())
        Y = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(Yh[row0:row0 + n])).cuda())
        calls = []
        attach_reducer(h, X.shape[1], Y.shape[1], post=lambda view, i: calls.append(i))  # counts every collective
        E = h.cv_folds(X, Y, A, np.arange(Xh.shape[0])[:, None])
        h.synchronize()
        during_folds = len(calls)
        out = {}
        for route in ("default", "stream"):
            if route == "stream":
                h.set_option(pls_amd.OPT_VALIDATION_LDS_ROWS, 0)
            out[route] = tuple(o.cpu().numpy() for o in h.validation(E))
            h.synchronize()
        out["E"] = E.cpu().numpy()
        out["collectives"] = (during_folds, len(calls))
        q.put((rank, out))
        h.close()
    except BaseException:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_handle_validation_is_local():
    """assertion 8, second half: two ranks share the GPU, cv_folds as a collective hands both the same E; validation on
    it sends no message (the counting hook of the reducer sees none) and both ranks get identical bits"""
    import queue

    import torch.multiprocessing as mp
    X, Y = _zs(_csv("nir.csv")), _zs(_csv("octane.csv"))
    splits, A = [31, 29], 10
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, port, q, X, Y, splits, A)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in procs:
            try:
                res.append(q.get(timeout=240))
            except queue.Empty:
                pytest.fail("a rank did not answer within 240 s")
        res.sort(key=lambda t: t[0])
        assert not any("error" in r[1] for r in res), [r[1].get("error") for r in res]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    a, b = res[0][1], res[1][1]
    assert np.array_equal(a["E"], b["E"])
    for o in (a, b):
        assert o["collectives"][0] > 0 and o["collectives"][1] == o["collectives"][0], o["collectives"]
    s = summary_ref(a["E"], ALPHA)
    check_preconditions(a["E"], s, ALPHA)
    for route in ("default", "stream"):
        assert _same_bits(a[route], b[route]), route
        _compare(a[route], a["E"], s, f"sharded rank 0 {route}")


# ---- the C++ drop-in ------------------------------------------------------------------------------------------------------
def test_cpp_residual_summary():
    """assertion 9: tests/cpp/validation_summary.cpp -- the device summary behind PLS::validation / optimal_num_components
    against a recomputation through the public host wilcoxon() and plain loops on residual.errors(), for cv_LOO and
    cv_LSO(0.3, 200); cv_NEW_DATA against A separate residuals() calls"""
    exe = os.path.join(ROOT, "tests", "cpp", "validation_summary")
    assert os.path.exists(exe), "tests/cpp/validation_summary not built (build() makes it through pls_amd/host/Makefile)"
    r = subprocess.run([exe, os.path.join(DATA, "nir.csv"), os.path.join(DATA, "octane.csv")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    print(r.stderr, file=sys.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "validation_summary: ok" in r.stdout
