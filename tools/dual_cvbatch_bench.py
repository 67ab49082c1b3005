#!/usr/bin/env python3
"""One pls_hip_cv_press_batch call on a short, wide device-resident X -- the cross-validated Q^2 of many response sets -- against
what the library offered before it: a loop over the problems of pls_hip_cv_folds plus pls_hip_validation (PRESS only).
   python tools/dual_cvbatch_bench.py {w1 | w2 | x} [--mode dual | plain] [--nprob N] [--label NAME] [--json FILE] [--reps N]
Calls:  w1 = 500 x 200,000 fp64    w2 = 2,000 x 50,000 fp64    x = 500 x 16,384 fp64;  M = 1, A = 5, 7 folds that cover all rows
(test_size = ceil(N / 7); the few rows that fill the last fold are held out twice).
--mode dual (default): the call for --nprob problems (default 101) under ALGO_DUAL, want = (PRESS, ssy): every problem and fold
    from one X X^T (plan_dual_cvbatch.hpp).  Alternating with it in the same process, the baseline: cv_folds + validation for
    each of 20 problems on the same DUAL handle, every turn its own X X^T.  The baseline runs code the new entry point leaves
    untouched, so both are measured in the same tree.  The record holds both medians, the baseline scaled to nprob problems
    and the ratio of the two.
--mode plain: the call on a handle without the option (the general route: one cross-validation per problem, whatever route
    pls_hip_cv_folds takes there); --nprob defaults to 3 on the wide shapes, where a problem costs 7 refits on all of X.
Data from the device generator, a stream of its own, one warm-up of each, then 20 repetitions (3 where a call takes more than
half a second; --reps overrides), each bracketed by HIP events on the handle's stream around the call and its synchronisation.
The medians (min - max) are printed and APPENDED to the list under "<call>/<label>" of FILE (default
profiles/dual/cvbatch_bench.json)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]


def opt(name):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return None


mode = opt("--mode") or "dual"
label = opt("--label")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "dual", "cvbatch_bench.json")
reps = opt("--reps")
nprob_arg = opt("--nprob")
args = [a for a in argv if not a.startswith("--")]
sys.path.insert(0, ROOT)

import numpy as np
import torch

import pls_amd
from pls_amd import _lib as L

CALLS = {"w1": (500, 200000), "w2": (2000, 50000), "x": (500, 16384)}
call = args[0] if args else "w1"
N, K = CALLS[call]
M, A, NF, NBASE = 1, 5, 7, 20
nprob = int(nprob_arg) if nprob_arg else (101 if mode == "dual" or call == "x" else 3)
label = label or f"{mode}-{nprob}"
ts = -(-N // NF)
rows = np.random.default_rng(7).permutation(N)
idx = np.ascontiguousarray(np.concatenate([rows, rows[:NF * ts - N]]).reshape(NF, ts), dtype=np.int64)

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    if mode == "dual":
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT)
    Ys = h.synth_y(0, N, max(nprob, NBASE) * M, pls_amd.SEED_DEFAULT)
    h.synchronize()
    Yn = pls_amd.as_colmajor(Ys[:, :nprob * M].clone())
    cols = [pls_amd.as_colmajor(Ys[:, b * M:(b + 1) * M].clone()) for b in range(NBASE)]
    press = torch.empty((A, M), dtype=torch.float64, device=X.device)

    def batch():
        return h.cv_press_batch(X, Yn, M, A, idx)["PRESS"]

    def loop():  # PRESS of NBASE problems as before the entry point existed
        for b in range(NBASE):
            E = h.cv_folds(X, cols[b], A, idx).permute(0, 2, 1)  # the library's layout, contiguous
            L.check(L.lib().pls_hip_validation(h.h, E.data_ptr(), NF * ts, A, M, L.MEM_DEVICE, press.data_ptr(), None, None, None), h.h)
        return press

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        q = f()
        h.synchronize()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), q

    runs = [batch, loop] if mode == "dual" else [batch]
    first = [timed(f)[0] for f in runs]  # warm-up: workspace, code objects
    first = [timed(f)[0] for f in runs]
    n = int(reps) if reps else (20 if max(first) < 500.0 else 3)
    t = [[] for _ in runs]
    q = None
    for _ in range(n):  # alternating
        for i, f in enumerate(runs):
            ms, out = timed(f)
            t[i].append(ms)
            q = out if i == 0 else q
    finite = bool(torch.isfinite(q).all())
    rec = {"call": call, "shape": [N, K, "f64"], "M": M, "A": A, "folds": [NF, ts], "nprob": nprob, "mode": mode, "label": label,
           "reps": n, "ms_median": statistics.median(t[0]), "ms_min": min(t[0]), "ms_max": max(t[0]), "PRESS_finite": finite}
    if mode == "dual":
        per = statistics.median(t[1]) / NBASE
        rec.update(loop_problems=NBASE, loop_ms_median=statistics.median(t[1]), loop_ms_min=min(t[1]), loop_ms_max=max(t[1]),
                   loop_ms_per_problem=per, loop_ms_for_nprob=per * nprob, ratio=per * nprob / rec["ms_median"])

print(f"{call} N={N} K={K} M={M} A={A} folds={NF}x{ts} nprob={nprob} [{label}]: {rec['ms_median']:.3f} ms "
      f"({rec['ms_min']:.3f} - {rec['ms_max']:.3f}), {n} repetitions")
if mode == "dual":
    print(f"   loop of cv_folds + validation: {rec['loop_ms_per_problem']:.3f} ms per problem, {rec['loop_ms_for_nprob']:.1f} ms for "
          f"{nprob}: ratio {rec['ratio']:.1f}")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{call}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
