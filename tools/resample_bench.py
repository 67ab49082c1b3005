#!/usr/bin/env python3
"""One pls_hip_fit_resampled call on a short, wide device-resident X with PLS_HIP_ALGO_DUAL set: every bootstrap draw from one
X X^T (plan_resample.hpp) against the only way without the call -- materialise the resampled rows X[idx], Y[idx] of every draw
and run one DUAL pls_hip_fit (with B) per draw.
   python tools/resample_bench.py {r1 | r2} [--mode resampled | fits | refit] [--want B | summary | Q] [--nrep N] [--label NAME]
                                  [--json FILE] [--reps N]
Calls:  r1 = 500 x 50,000 fp64    r2 = 2,000 x 20,000 fp64;  M = 1, A = 5, 200 bootstrap draws (bootstrap_weights, seed 0).
--mode resampled (default): one fit_resampled call under ALGO_DUAL; --want summary (default: B0, Bmean, Bm2), B (every B_b) or
               Q (Q and tt only: no back-projection).
--mode fits:   per draw X[idx], Y[idx] gathered on the device (torch indexing into a column-major buffer, inside the timed
               region: the materialisation is part of that way) and one DUAL pls_hip_fit with B; --nrep defaults to 20 there
               and the figure is for those.
--mode refit:  fit_resampled under PLS_HIP_RESAMPLE_REFIT=1 (the general route: row-scaled copies, one fit per draw).
The baseline runs no code this route changes, so it is measured in the same tree.  Data from the device generator, a stream of
its own, one warm-up call (two where a call takes less than half a second), then repeated calls each bracketed by HIP events
on the handle's stream around the call and its synchronisation: 20 of them, or 3 where a call takes more than half a second
(--reps overrides).  The median (min - max) is printed and APPENDED to the list under "<call>/<label>" of FILE (default
profiles/dual/resample_bench.json)."""
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


mode = opt("--mode") or "resampled"
wanted = opt("--want") or "summary"
label = opt("--label")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "dual", "resample_bench.json")
reps = opt("--reps")
nrep = int(opt("--nrep") or (20 if mode == "fits" else 200))
args = [a for a in argv if not a.startswith("--")]
if mode == "refit":
    os.environ["PLS_HIP_RESAMPLE_REFIT"] = "1"
label = label or (mode + ("" if mode == "fits" else "+" + wanted))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import pls_amd

CALLS = {"r1": (500, 50000), "r2": (2000, 20000)}
call = args[0] if args else "r1"
N, K = CALLS[call]
M, A = 1, 5
want = {"summary": ("B0", "Bmean", "Bm2"), "B": ("B",), "Q": ("Q", "tt")}[wanted]

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT)
    Y = h.synth_y(0, N, M, pls_amd.SEED_DEFAULT)
    Wh = pls_amd.bootstrap_weights(N, nrep, 0)
    Wt = pls_amd.as_colmajor(torch.from_numpy(np.ascontiguousarray(Wh)).cuda())
    idx = [torch.from_numpy(np.repeat(np.arange(N), Wh[:, b].astype(np.int64))).cuda() for b in range(nrep)]
    Xr, Yr = pls_amd.colmajor_empty(N, K, X.dtype, X.device), pls_amd.colmajor_empty(N, M, Y.dtype, Y.device)
    h.synchronize()
    out = None

    def once():
        global out
        if mode == "fits":
            for b in range(nrep):
                Xr.copy_(X[idx[b]]); Yr.copy_(Y[idx[b]])
                out = h.fit_device(Xr, Yr, A, pls_amd.KERNEL_TYPE1, want_B=True, out=out)
            return out["B"]
        return h.fit_resampled(X, Y, A, Wt, want=want)[want[0]]

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        q = once()
        h.synchronize()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), q

    first, q = timed()  # warm-up: workspace, code objects
    if first < 500.0:
        first, q = timed()
    n = int(reps) if reps else (20 if first < 500.0 else 3)
    t = [timed()[0] for _ in range(n)]
    finite = bool(torch.isfinite(q).all())
    rec = {"call": call, "shape": [N, K, "f64"], "M": M, "A": A, "nrep": nrep, "mode": mode, "want": list(want), "label": label,
           "reps": n, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_per_draw": statistics.median(t) / nrep,
           "finite": finite}

print(f"{call} N={N} K={K} M={M} A={A} nrep={nrep} [{label}]: {rec['ms_median']:.3f} ms "
      f"({rec['ms_min']:.3f} - {rec['ms_max']:.3f}), {n} repetitions, {rec['ms_per_draw']:.3f} ms per draw")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{call}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
