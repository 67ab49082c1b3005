"""Every entry point is held to the order of the stream it was given (include/pls_hip.h, "Stream order").

tests/stream_order.py has the sandwich and the catalogue: one case per entry point and route, fp64 and one fp32 twin per entry
point.  Here every case runs its two synchronous baselines (the route asserted from the launch counters, every output required to
differ between the two data sets), the sandwich on the warm handle (bits; for *enqueues* cases: the call came back while the
stream was still held) and once on a handle that has never run anything (bits only).  Then what a single call cannot show: the
callers' index lists, two calls back to back, set_stream and close with work pending, host-memory calls on a busy handle, two
handles on two streams in flight together, the Python wrappers under a foreign current stream -- and the trap itself, which three
misbehaving stand-ins must not get through.

Single GPU, single process: row-sharded handles, groups and the cross-process exchange are left to a later change, as in
tests/test_gpu_history.py.  Nothing here can fault: every race is a race between copies and fills of scratch tensors.
Run with -s for one line per sandwich: route, window, host-side duration, warm / fresh, "returned with the stream held"."""
import numpy as np
import pytest

import stream_order as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    b = so.Bench()
    yield b
    print(f"stream_order: largest window {so.Window.largest_ms:.1f} ms at {so.Window.rate():.0f} ticks/ms", flush=True)
    b.close()


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a device left in error by an earlier test ends the session here, before anything more is launched on it"""
    import torch
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:
            pytest.exit(f"the device is in error, nothing more is run on it: {e}", returncode=3)
    yield


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", so.GROUPS)
def test_catalogue(bench, group):
    cases = [c for c in so.CASES if c.group == group]
    print(f"{group}: {len(cases)} cases")
    bad = []
    for c in cases:
        bad += so.run_case(bench, c)
    assert not bad, "\n".join(bad)


# ---- helpers of the tests below ------------------------------------------------------------------------------------------------------
FUSED = "fit kernel-fused 1301x48 m3 a6"
WIDE = "fit nipals 515x1500 m2 a5"


def solo(rig, kind=None, tune=None, h=None):
    """the synchronous baseline of the rig's case on a handle of its own (or on h, which it leaves warm): (digest, window for the call)"""
    own = h is None
    if own:
        h = so.make_handle(kind or rig.case.kind, rig.s)
    try:
        if tune:
            tune(h)
        rig.baseline(h, "true")
        want, _, _, host_ms = rig.baseline(h, "true")
    finally:
        if own:
            h.close()
    return want, so.Window.ms_for(host_ms)


def snapshot_ok(r, want, what):
    assert r["rc"] == 0, (what, r["rc"])
    assert r["held_before"], f"{what}: the window had closed before the call was made"
    assert so.digest(r["snap"]) == want, f"{what}: the outputs snapshotted behind the call are not the solo baseline's bits"


# ---- index lists -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cv_folds 1301x48 m3 a6: batched on the shared X^T X", "cv_folds 60x400 m2 a6: DUAL: every fold from one X X^T",
                                  "cv_press_batch 60x400 m2 a4 x3: DUAL: sample space", "cv_folds_missing 120x30 m2 a3: one round"])
def test_the_index_list_may_be_reused_when_the_call_returns(bench, name):
    import torch
    case = so.by_name(name)
    with torch.cuda.stream(bench.s):
        rig = so.Rig(bench, case)
        mine, other = case.idx(6), case.idx(7)
        assert mine.shape == other.shape and not np.array_equal(mine, other)
        want, window = solo(rig, tune=None)   # (the case's own call uses the fold assignment of seed 6)
        h = so.make_handle(case.kind, bench.s)
        try:
            idx = mine.copy()
            rig.prepare()

            def call():
                rc = case.call(h, rig.live, rig.out, so.TRUE_SEED, idx=idx)
                idx[...] = other        # the line after the call returns
                return rc
            r = rig.queue(call, window)
            bench.s.synchronize()
            snapshot_ok(r, want, name)
            assert h._lib.pls_hip_synchronize(h.h) == 0
        finally:
            h.close()


# ---- two calls back to back ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["small then large", "large then small"])
def test_two_calls_back_to_back_the_second_growing_the_workspaces(bench, order):
    import torch
    import pls_amd
    a, b = so.by_name(FUSED), so.by_name(WIDE)
    with torch.cuda.stream(bench.s):
        ra, rb = so.Rig(bench, a), so.Rig(bench, b)
        nip = lambda h: h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        want_a, wa = solo(ra)
        want_b, wb = solo(rb)
        h = so.make_handle("general", bench.s)
        try:
            ra.prepare(); rb.prepare()
            first, second = ((ra, a), (rb, b)) if order == "small then large" else ((rb, b), (ra, a))

            def call(rig, case):
                (nip if case is b else (lambda h: h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)))(h)
                return case.call(h, rig.live, rig.out, so.TRUE_SEED)
            r1 = first[0].queue(lambda: call(*first), wa + wb)
            r2 = second[0].queue(lambda: call(*second), 0.0, hold=False)
            bench.s.synchronize()
            for r, (rig, case) in ((r1, first), (r2, second)):
                print(f"  {order}: {case.name}: host {r['host_ms']:.3f} ms; returned with the stream held: {'yes' if r['held_after'] else 'no'}")
            snapshot_ok(r1, want_a if first[1] is a else want_b, first[1].name)
            r2["held_before"] = True   # (its own event follows the first call: the first call's window is the one that counts)
            snapshot_ok(r2, want_a if second[1] is a else want_b, second[1].name)
            assert r1["held_after"], "the first call waited for the device"
            assert h._lib.pls_hip_synchronize(h.h) == 0
        finally:
            h.close()


# ---- set_stream and close with work pending -------------------------------------------------------------------------------------------
def test_set_stream_with_work_pending(bench):
    import torch
    case = so.by_name(FUSED)
    s1, s2 = bench.s, torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1g = so.Rig(bench, case)
        want, window = solo(r1g)
    with torch.cuda.stream(s2):
        r2g = so.Rig(bench, case, s=s2)
        want2, _ = solo(r2g)
    assert want2 == want
    with torch.cuda.stream(s1):
        h = so.make_handle(case.kind, s1)
        r1g.prepare()
        r1 = r1g.queue(lambda: case.call(h, r1g.live, r1g.out, so.TRUE_SEED), window)
    try:
        with torch.cuda.stream(s2):
            r2g.prepare()
            h.set_stream(s2.cuda_stream)
            r2 = r2g.queue(lambda: case.call(h, r2g.live, r2g.out, so.TRUE_SEED), window)
        s1.synchronize(); s2.synchronize()
        snapshot_ok(r1, want, "the call pending on the first stream")
        snapshot_ok(r2, want, "the call on the second stream")
        assert r2["held_after"], "the call on the second stream waited for the device"
        assert h._lib.pls_hip_synchronize(h.h) == 0
    finally:
        h.close()


def test_close_with_work_pending(bench):
    import torch
    case = so.by_name(FUSED)
    with torch.cuda.stream(bench.s):
        rig = so.Rig(bench, case)
        want, window = solo(rig)
        h = so.make_handle(case.kind, bench.s)
        rig.prepare()
        r = rig.queue(lambda: case.call(h, rig.live, rig.out, so.TRUE_SEED), window)
        h.close()
        bench.s.synchronize()
        snapshot_ok(r, want, "the call pending when the handle was closed")


# ---- host-memory calls on a busy handle ---------------------------------------------------------------------------------------------
def _host_calls():
    """name -> f(h) -> dict of numpy outputs: one PLS_HIP_MEM_HOST call of every entry point that takes `mem`, at one small shape"""
    import ctypes
    import pls_amd
    from pls_amd import _lib as L
    rng = np.random.default_rng(5)
    F = np.asfortranarray
    N, K, M, A = 97, 33, 2, 5
    X, Y = F(rng.standard_normal((N, K))), F(rng.standard_normal((N, M)))
    Xn = X.copy(order="F"); Xn[rng.random((N, K)) < 0.1] = np.nan; Xn[:, 0] = X[:, 0]; Xn[0, :] = X[0, :]
    R, P, Q = F(rng.standard_normal((K, A))), F(rng.standard_normal((K, A))), F(rng.standard_normal((M, A)))
    Ys = F(rng.standard_normal((N, 3 * M)))
    idx = np.arange(12, dtype=np.int64).reshape(3, 4)
    E = rng.standard_normal((M, 40, A))
    Wt = pls_amd.bootstrap_weights(N, 4, 3)
    tv = np.linspace(1.0, 2.0, A)

    def model_sse(h):
        out = np.zeros((M, A), order="F")
        q = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        L.check(L.lib().pls_hip_model_sse(h.h, q(X), N, q(Y), N, N, K, M, A, q(R), q(Q), L.F64, L.MEM_HOST, q(out)), h.h)
        return {"SSE": out}
    d = lambda v: v if isinstance(v, dict) else {"out": v}
    t = lambda names, v: dict(zip(names, v))
    return {
        "pls_hip_fit": lambda h: {k: v for k, v in h.fit_host(X, Y, A).items() if v is not None},
        "pls_hip_coefficients": lambda h: d(h.coefficients(R, Q, 4)),
        "pls_hip_xb": lambda h: d(h.xb(X, R)),
        "pls_hip_model_sse": model_sse,
        "pls_hip_cv_folds": lambda h: d(h.cv_folds(X, Y, A, idx)),
        "pls_hip_validation": lambda h: t(("press", "D", "probw", "ref"), h.validation(E)),
        "pls_hip_x_diagnostics": lambda h: h.x_diagnostics(X, R, P, tvar=tv, want=("Q", "T2", "S", "ssx", "sst")),
        "pls_hip_fit_batch": lambda h: h.fit_batch(X, Ys, M, A, want=("R", "Q", "tt", "B", "ssy")),
        "pls_hip_fit_resampled": lambda h: h.fit_resampled(X, Y, A, Wt, want=("Q", "tt", "B", "B0", "Bmean", "Bm2")),
        "pls_hip_cv_press_batch": lambda h: h.cv_press_batch(X, Ys, M, A, idx, want=("PRESS", "ssy", "E")),
        "pls_hip_fit_missing": lambda h: h.fit_missing(Xn, Y, A),
        "pls_hip_cv_folds_missing": lambda h: d(h.cv_folds_missing(Xn, Y, 3, idx)),
        "pls_hip_scores_missing": lambda h: d(h.scores_missing(Xn, R, P)),
        "pls_hip_x_diagnostics_missing": lambda h: h.x_diagnostics_missing(Xn, R, P, tvar=tv, want=("Q", "T2", "S", "ssx", "sst", "nobs")),
        "pls_hip_colwise_z_scores_missing": lambda h: t(("Z", "mean", "sd", "nobs"), h.z_scores_missing(Xn)),
    }


HOST_ENTRIES = ["pls_hip_fit", "pls_hip_coefficients", "pls_hip_xb", "pls_hip_model_sse", "pls_hip_cv_folds", "pls_hip_validation",
                "pls_hip_x_diagnostics", "pls_hip_fit_batch", "pls_hip_fit_resampled", "pls_hip_cv_press_batch", "pls_hip_fit_missing",
                "pls_hip_cv_folds_missing", "pls_hip_scores_missing", "pls_hip_x_diagnostics_missing", "pls_hip_colwise_z_scores_missing"]


def _np_digest(out):
    import hashlib
    s = hashlib.sha256()
    for k in sorted(out):
        a = np.ascontiguousarray(out[k])
        s.update(f"{k}:{a.dtype}:{a.shape}".encode()); s.update(a.tobytes())
    return s.hexdigest()


def test_host_memory_calls_on_a_busy_handle(bench):
    """a device-memory fit is left pending behind a window, then the host-memory call is made on the same handle: it returns with
    its own baseline in place, and the pending fit's snapshot is still its baseline"""
    import torch
    calls = _host_calls()
    assert list(calls) == HOST_ENTRIES
    case = so.by_name(FUSED)
    bad = []
    with torch.cuda.stream(bench.s):
        rig = so.Rig(bench, case)
        want, window = solo(rig)
        for entry, f in calls.items():
            h = so.make_handle(case.kind, bench.s)
            try:
                base = _np_digest(f(h))
                assert _np_digest(f(h)) == base, entry
                rig.prepare()
                r = rig.queue(lambda: case.call(h, rig.live, rig.out, so.TRUE_SEED), window)
                got = _np_digest(f(h))          # (no synchronisation in between; the call itself completes)
                bench.s.synchronize()
                if got != base:
                    bad.append(f"{entry}: the host-memory call behind a pending fit does not return its own baseline")
                if not (r["rc"] == 0 and r["held_before"] and so.digest(r["snap"]) == want):
                    bad.append(f"{entry}: the pending fit's snapshot is not its baseline after the host-memory call")
                if h._lib.pls_hip_synchronize(h.h) != 0:
                    bad.append(f"{entry}: pls_hip_synchronize failed")
            finally:
                h.close()
    assert not bad, "\n".join(bad)


# ---- two handles, two streams, in flight together ------------------------------------------------------------------------------------
PAIRS = {
    "resident fits": [("fit resident 1301x48 m1 a6",) * 2, ("fit resident 1301x48 m3 a6",) * 2, ("fit resident-auto 1301x48 m1 a6",) * 2,
                      ("fit resident-auto 1301x48 m3 a6",) * 2],
    "general fused against DUAL": [(FUSED, "fit dual 200x5000 m3 a5")],
    "fit_batch against validation": [("fit_batch batched 1301x48 m1 x3", "validation m2 a5 nobs1001 LDS")],
}


@pytest.mark.parametrize("what", list(PAIRS))
def test_two_handles_on_two_streams_in_flight_together(bench, what):
    """A resident fit whose bounded 50 ms wait runs out here (PLS_HIP_ERR_DEVICE from pls_hip_synchronize) is a finding about
    resident_turn / resident_done, not something to run again."""
    import torch
    streams = (bench.s, torch.cuda.Stream())
    rigs, handles = [], {}
    try:
        for names in PAIRS[what]:
            for s, name in zip(streams, names):
                case = so.by_name(name)
                with torch.cuda.stream(s):
                    rig = so.Rig(bench, case, s=s)
                    if (s, case.kind) not in handles:
                        handles[(s, case.kind)] = so.make_handle(case.kind, s)
                    fresh, _ = solo(rig)
                    want, window = solo(rig, h=handles[(s, case.kind)])   # (... which leaves the handle warm: no workspace grows below)
                    assert want == fresh, case.name
                    rig.prepare()
                rigs.append((rig, case, want, window, handles[(s, case.kind)]))
        total = sum(w for _, _, _, w, _ in rigs)
        for s in streams:
            with torch.cuda.stream(s):
                so.Window.hold(total)
        results = []
        for rig, case, want, _, h in rigs:      # alternately: stream 1, stream 2, stream 1, ...
            with torch.cuda.stream(rig.s):
                results.append(rig.queue(lambda: case.call(h, rig.live, rig.out, so.TRUE_SEED), total, hold=False))
        for s in streams:
            s.synchronize()
        for (rig, case, want, _, h), r in zip(rigs, results):
            print(f"  {what}: {case.name} on stream {streams.index(rig.s) + 1}: host {r['host_ms']:.3f} ms; returned with the stream held: "
                  f"{'yes' if r['held_after'] else 'no'}")
            r["held_before"] = True   # (the window is the one held on both streams before the first call)
            snapshot_ok(r, want, f"{case.name} on stream {streams.index(rig.s) + 1}")
        late = [case.name for (_, case, _, _, _), r in zip(rigs, results) if not r["held_after"]]
        assert not late, f"returned only after the streams had been released, so not in flight together with the others: {late}"
        for h in handles.values():
            rc = h._lib.pls_hip_synchronize(h.h)
            assert rc == 0, (rc, so._pls()._lib.last_error(h.h))
    finally:
        for s in streams:
            s.synchronize()
        for h in handles.values():
            h.close()


# ---- the Python wrappers under a foreign current stream -----------------------------------------------------------------------------
def test_the_wrappers_run_their_own_torch_work_on_the_handles_stream(bench):
    """Handle(stream=s) while torch's current stream is the default stream; arguments that make the wrapper convert: a float32
    row-major Bm, R and P of the wrong leading dimension, a strided Q"""
    import torch
    import pls_amd
    s = bench.s
    N, K, A, M = 1001, 37, 6, 2
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    h = pls_amd.Handle(stream=s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            data = {}
            for seed in (so.TRUE_SEED, so.DECOY_SEED):
                data[seed] = {"X": bench.util.synth_x(0, N, K, seed), "Y": bench.util.synth_y(0, N, M, seed),
                              "Bm": so.normal(seed, "wB", K, 3).to(torch.float32).contiguous(),            # row-major fp32
                              "R": so.cm(K, A, ld=K + 3).copy_(so.normal(seed, "wR", K, A)),               # ld != K
                              "P": so.cm(K, A, ld=K + 5).copy_(so.normal(seed, "wP", K, A)),
                              "S": so.normal(seed, "wS", N, A),
                              "Q": so.normal(seed, "wQ", M, 2 * A)[:, ::2]}                                # strided
            bench.util.synchronize(); s.synchronize()
            live = {k: so.like(v) for k, v in data[so.TRUE_SEED].items()}
            assert live["Bm"].stride() == (3, 1) and live["R"].stride(1) == K + 3 and live["Q"].stride(1) == 2 * M
        calls = {
            "xb": lambda: {"XB": h.xb(live["X"], live["Bm"])},
            "x_diagnostics": lambda: h.x_diagnostics(live["X"], live["R"], live["P"], want=("Q", "T2", "S", "ssx", "sst")),
            "sse_by_components": lambda: {"SSE": h.sse_by_components(live["S"], live["Y"], live["Q"])},
        }
        bad = []
        for name, f in calls.items():
            with torch.cuda.stream(s):
                for k, v in live.items():
                    v.copy_(data[so.TRUE_SEED][k])
                s.synchronize()
            want = f(); s.synchronize(); want = so.digest(want)
            with torch.cuda.stream(s):
                for k, v in live.items():
                    v.copy_(data[so.DECOY_SEED][k])
                s.synchronize()
            decoy = f(); s.synchronize()
            assert so.digest(decoy) != want
            with torch.cuda.stream(s):
                opened = torch.cuda.Event()
                so.Window.hold(so.MIN_WINDOW_MS); opened.record(s)
                for k, v in live.items():
                    v.copy_(data[so.TRUE_SEED][k])
            held = not opened.query()
            out = f()                                   # torch's current stream: the default stream
            with torch.cuda.stream(s):
                snap = {k: v.clone() for k, v in out.items()}
                for k, v in live.items():
                    v.copy_(data[so.DECOY_SEED][k])
            s.synchronize()
            assert held, "the window had closed before the call was made"
            if so.digest(snap) != want:
                bad.append(f"Handle.{name}: not the baseline's bits: its conversions did not run on the handle's stream")
        assert not bad, "\n".join(bad)
        h.synchronize()
    finally:
        h.close()


# ---- the trap closes ------------------------------------------------------------------------------------------------------------------
def test_the_trap_closes(bench):
    """no library call: three stand-in "entry points" written in torch must each FAIL the sandwich in their own way, a fourth passes"""
    import torch
    s, other = bench.s, torch.cuda.Stream()
    work = lambda i, o: o["y"].copy_(i["x"] * 2.0 + 1.0)
    late = []

    def good(h, i, o, seed):
        work(i, o)
        return 0

    def early_read(h, i, o, seed):
        with torch.cuda.stream(other):
            work(i, o)
        return 0

    def late_write(h, i, o, seed):
        tmp = i["x"] * 2.0 + 1.0
        late.append(lambda: o["y"].copy_(tmp))
        return 0

    def waits(h, i, o, seed):
        work(i, o)
        s.synchronize()
        return 0
    verdicts = {}
    with torch.cuda.stream(s):
        for name, fn in (("good", good), ("early read", early_read), ("late write", late_write), ("waits", waits)):
            case = so.Case("stand-in: " + name, "-", "-", "-", "default", so.ENQUEUES, False,
                           lambda u, seed: {"x": so.normal(seed, "trap", 4096, 8)}, lambda i: {"y": so.like(i["x"])}, fn, lambda l: None)
            rig = so.Rig(bench, case)
            want = so.digest({"y": rig.true["x"] * 2.0 + 1.0})
            assert want != so.digest({"y": rig.decoy["x"] * 2.0 + 1.0})
            rig.prepare()

            def after():   # behind the trailing scribble: the write that comes too late, from another stream
                if late:
                    ev = torch.cuda.Event(); ev.record(s)
                    other.wait_event(ev)
                    with torch.cuda.stream(other):
                        late.pop()()
            r = rig.queue(lambda: fn(None, rig.live, rig.out, so.TRUE_SEED), so.MIN_WINDOW_MS, after=after)
            s.synchronize(); other.synchronize()
            so.report(case, "stand-in", r)
            verdicts[name] = so.judge(r, want, name, True)
            print(f"  {name}: {verdicts[name] or 'passes'}")
    assert verdicts["good"] == [], verdicts["good"]
    for name, why in (("early read", "not the baseline's bits"), ("late write", "not the baseline's bits"), ("waits", "waited for the device")):
        assert len(verdicts[name]) == 1 and why in verdicts[name][0], (name, verdicts[name])
