#!/usr/bin/env python3
"""One pls_hip_cv_folds call on a short, wide device-resident X with PLS_HIP_ALGO_DUAL set: every fold from one X X^T
(plan_dual_cv.hpp) against what a library without that route does with the same call (one DUAL fit per fold, or the X^T X route).
   python tools/dual_cv_bench.py {v1 | v2 | v3 | v4} [--tree DIR] [--label NAME] [--json FILE] [--reps N] [--profile]
Calls:  v1 = 512 x 262,144 fp64, M = 1, A = 20, leave-one-out        v2 = 2,048 x 8,192 fp64, M = 1, A = 20, leave-one-out
        v3 = 1,000 x 500,000 fp32, M = 1, A = 20, ten folds of 100    v4 = 2,048 x 131,072 fp64, M = 4, A = 50, 20 folds of 100
Data from the device generator, a stream of its own, one warm-up call (two where a call takes less than half a second), then
repeated calls each bracketed by HIP events around the synchronising call: 20 of them, or 3 where a call takes more than half
a second (--reps overrides).  The median (min - max) and the number of repetitions are printed and APPENDED to the list under
"<call>/<label>" of FILE (default profiles/dual/cv_bench.json), so that alternating invocations -- this tree, the parent's,
this tree, ... on one box -- leave their figures side by side.
--tree DIR: the pls_amd package of another checkout (built there), e.g. the parent commit; label it with --label parent.
--profile: 3 calls and nothing else, for one `rocprofv3 --kernel-trace --stats -- python tools/dual_cv_bench.py v1 --profile`
(no counters in the same run)."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]


def opt(name):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return None


tree = opt("--tree")
label = opt("--label") or ("tree" if tree else "this")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "dual", "cv_bench.json")
reps = opt("--reps")
flags = {a for a in argv if a.startswith("--")}
args = [a for a in argv if not a.startswith("--")]
sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)

import torch

import pls_amd

# N, K, storage, M, A, test_size, folds (0: leave-one-out)
CALLS = {"v1": (512, 262144, "f64", 1, 20, 1, 0), "v2": (2048, 8192, "f64", 1, 20, 1, 0),
         "v3": (1000, 500000, "f32", 1, 20, 100, 10), "v4": (2048, 131072, "f64", 4, 50, 100, 20)}
call = args[0] if args else "v1"
N, K, st, M, A, ts, nf = CALLS[call]
if not hasattr(pls_amd, "ALGO_DUAL"):
    print(f"{call} [{label}]: this library has no ALGO_DUAL, skipped")
    sys.exit(0)
dt = torch.float32 if st == "f32" else torch.float64
if nf == 0:
    idx = np.arange(N, dtype=np.int64)[:, None]
else:
    rng = np.random.default_rng(7)
    idx = np.stack([rng.permutation(N)[:ts] for _ in range(nf)]).astype(np.int64)

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
    Y = h.synth_y(0, N, M, pls_amd.SEED_DEFAULT, dtype=dt)
    h.synchronize()

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        E = h.cv_folds(X, Y, A, idx)  # (returns synchronised)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), E

    if "--profile" in flags:
        for _ in range(3):
            h.cv_folds(X, Y, A, idx)
        print(json.dumps({"call": call, "calls": 3}))
        sys.exit(0)
    first, E = timed()  # warm-up: workspace, code objects
    if first < 500.0:
        first, E = timed()
    n = int(reps) if reps else (20 if first < 500.0 else 3)
    t = [timed()[0] for _ in range(n)]
    finite = bool(torch.isfinite(E).all())

rec = {"call": call, "shape": [N, K, st], "M": M, "A": A, "test_size": ts, "folds": int(idx.shape[0]), "label": label, "reps": n,
       "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "E_finite": finite}
print(f"{call} N={N} K={K} {st} M={M} A={A} folds={idx.shape[0]}x{ts} [{label}]: {rec['ms_median']:.3f} ms "
      f"({rec['ms_min']:.3f} - {rec['ms_max']:.3f}), {n} repetitions")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{call}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
