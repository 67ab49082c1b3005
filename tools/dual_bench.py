#!/usr/bin/env python3
"""One pls_hip_fit on a short, wide device-resident X under one plan: the sample-space plan against the plans it replaces.
   python tools/dual_bench.py {w1 | w2 | w3 | w4} {dual | kernel | auto | nipals} [--tree DIR] [--label NAME] [--json FILE] [--profile]
Shapes:  w1 = 512 x 262,144 fp64, M = 1, A = 20      w2 = 1,000 x 500,000 fp32, M = 1, A = 20
         w3 = 2,048 x 131,072 fp64, M = 4, A = 50    w4 = 8,192 x 65,536 fp64, M = 1, A = 20
Data from the device generator, a stream of its own, 5 warm-up fits, then 20 fits each bracketed by HIP events; the median
(min - max) is printed and APPENDED to the list under "<shape>/<plan>/<label>" of FILE (default profiles/dual/bench.json), so
that alternating invocations -- this tree, the parent's, this tree, ... on one box -- leave their triples side by side.
--tree DIR: the pls_amd package of another checkout (built there), e.g. the parent commit; label it with --label parent.  A
library without ALGO_DUAL skips the plan `dual` (exit 0, nothing recorded).
--profile: 7 fits and nothing else, for one `rocprofv3 --kernel-trace --stats -- python tools/dual_bench.py w1 dual --profile`
(no counters in the same run).
Model: G = X X^T executes 2 K (128 nb)^2 (nb + 1) / (2 nb) flops in blocks of 128 rows, nb = ceil(N / 128); the fp64 matrix
pipe is 78.6 TF; a sweep over X at the 6.29 TB/s copy ceiling takes N K s / 6.29e12 seconds."""
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


tree = opt("--tree")
label = opt("--label") or ("tree" if tree else "this")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "dual", "bench.json")
flags = {a for a in argv if a.startswith("--")}
args = [a for a in argv if not a.startswith("--")]
sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)

import torch

import pls_amd

SHAPES = {"w1": (512, 262144, "f64", 1, 20), "w2": (1000, 500000, "f32", 1, 20), "w3": (2048, 131072, "f64", 4, 50),
          "w4": (8192, 65536, "f64", 1, 20)}
shape = args[0] if args else "w1"
plan = args[1] if len(args) > 1 else "dual"
N, K, st, M, A = SHAPES[shape]
if plan == "dual" and not hasattr(pls_amd, "ALGO_DUAL"):
    print(f"{shape} {plan} [{label}]: this library has no ALGO_DUAL, skipped")
    sys.exit(0)
algo = {"dual": getattr(pls_amd, "ALGO_DUAL", None), "kernel": pls_amd.ALGO_KERNEL, "auto": pls_amd.ALGO_AUTO,
        "nipals": pls_amd.ALGO_NIPALS}[plan]
dt = torch.float32 if st == "f32" else torch.float64

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    h.set_option(pls_amd.OPT_ALGO, algo)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
    Y = h.synth_y(0, N, M, pls_amd.SEED_DEFAULT, dtype=dt)
    h.synchronize()
    out = h.fit_device(X, Y, A)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        h.fit_device(X, Y, A, out=out)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    if "--profile" in flags:
        for _ in range(7):
            h.fit_device(X, Y, A, out=out)
        h.synchronize()
        print(json.dumps({"shape": shape, "plan": plan, "calls": 8}))
        sys.exit(0)
    for _ in range(5):
        h.fit_device(X, Y, A, out=out)
    h.synchronize()
    t = [timed() for _ in range(20)]

es = 4 if st == "f32" else 8
nb = -(-N // 128)
rec = {"shape": [N, K, st], "M": M, "A": A, "plan": plan, "label": label, "ms_median": statistics.median(t), "ms_min": min(t),
       "ms_max": max(t), "sweep_ms_at_6.29TBs": N * K * es / 6.29e12 * 1e3,
       "xxt_flops_executed": 2 * K * (128 * nb) ** 2 * (nb + 1) / (2 * nb)}
print(f"{shape} N={N} K={K} {st} M={M} A={A} {plan} [{label}]: {rec['ms_median']:.3f} ms ({rec['ms_min']:.3f} - {rec['ms_max']:.3f})")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{shape}/{plan}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
