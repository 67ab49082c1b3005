#!/usr/bin/env python3
"""pls_hip_fit_batch on device-resident data against the loop of single fits it replaces.
   python tools/fit_batch_bench.py {c3 | k4096} NPROB [--loop] [--tree DIR] [--profile] [--json FILE]
Shapes: c3 = config 3's X (1,048,576 x 512 fp64), k4096 = 131,072 x 4,096 fp32; M = 1, A = 20; problem 0 is Y, the others
are row permutations of it drawn on the device.
Default mode: Handle.fit_batch(want = Q, tt, ssy, B) on NPROB problems.
--loop: the baseline -- sequential pls_hip_fit(KERNEL_TYPE2) calls on (X, Y_b), timed on 16 problems and SCALED linearly to
        NPROB (the record says so: "scaled_from": 16).  It uses nothing this entry point added, so `--tree DIR` can point it
        at a checkout of the parent commit (its pls_amd package, built there) -- that is how the committed baseline was taken.
Either mode: a stream of its own (not the default stream), 5 warm-up calls, then 20 calls each bracketed by HIP events; the
median (min - max) is printed and the record is merged into FILE (default profiles/r6/fit_batch.json) under
"<shape>/<NPROB>/<batch|loop>".  One shape and mode per invocation: the caller gives every step its own `timeout` and chains
the steps with &&.
--profile: 7 calls and nothing else, for one `rocprofv3 --kernel-trace --stats -- python tools/fit_batch_bench.py c3 1024 --profile`
(no counters in the same run).  Model flops: X^T G 2 N K C; the component steps' GEMM 2 K^2 C A."""
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
json_path = opt("--json") or os.path.join(ROOT, "profiles", "r6", "fit_batch.json")
flags = {a for a in argv if a.startswith("--")}
args = [a for a in argv if not a.startswith("--")]
sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)

import torch

import pls_amd

SHAPES = {"c3": (1 << 20, 512, "f64"), "k4096": (131072, 4096, "f32")}
shape = args[0] if args else "c3"
nprob = int(args[1]) if len(args) > 1 else 256
N, K, st = SHAPES[shape]
M, A, LOOP_N = 1, 20, 16
dt = torch.float32 if st == "f32" else torch.float64
loop = "--loop" in flags

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
    Y = h.synth_y(0, N, 1, pls_amd.SEED_DEFAULT, dtype=dt)
    ncol = LOOP_N if loop else nprob
    Ys = pls_amd.colmajor_empty(N, ncol, dt, X.device)
    gen = torch.Generator(device=X.device)
    gen.manual_seed(20261016)
    Ys[:, 0] = Y[:, 0]
    for b in range(1, ncol):
        Ys[:, b] = Y[torch.randperm(N, device=X.device, generator=gen), 0]
    cols = [pls_amd.as_colmajor(Ys[:, b:b + 1]) for b in range(ncol)] if loop else None
    h.synchronize()

    def call():
        if loop:
            out = None
            for yb in cols:
                out = h.fit_device(X, yb, A, pls_amd.KERNEL_TYPE2, want_B=True, out=out)
            return out
        return h.fit_batch(X, Ys, M, A, want=("Q", "tt", "ssy", "B"))

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = call()
        e1.record(stream)
        e1.synchronize()
        del out
        return e0.elapsed_time(e1)

    if "--profile" in flags:
        for _ in range(7):
            call()
        h.synchronize()
        print(json.dumps({"shape": shape, "nprob": nprob, "calls": 7, "mode": "loop" if loop else "batch"}))
        sys.exit(0)
    for _ in range(5):
        call()
    h.synchronize()
    t = [timed() for _ in range(20)]

scale = nprob / LOOP_N if loop else 1.0
rec = {"shape": [N, K, st], "M": M, "A": A, "nprob": nprob, "mode": "loop" if loop else "batch",
       "ms_median": statistics.median(t) * scale, "ms_min": min(t) * scale, "ms_max": max(t) * scale,
       "flops_xtg": 2 * N * K * nprob * M, "flops_step_gemm": 2 * K * K * nprob * A}
if loop:
    rec.update(scaled_from=LOOP_N, ms_median_measured_16=statistics.median(t), tree="the checkout given with --tree" if tree else "this tree")
else:
    rec["xtg_lower_bound_ms_at_78.6TF"] = rec["flops_xtg"] / 78.6e12 * 1e3
print(f"{shape} N={N} K={K} {st} nprob={nprob} {'loop of single fits (16 timed, scaled)' if loop else 'pls_hip_fit_batch'}: "
      f"{rec['ms_median']:.3f} ms ({rec['ms_min']:.3f} - {rec['ms_max']:.3f})")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book[f"{shape}/{nprob}/{rec['mode']}"] = rec
b, l = book.get(f"{shape}/{nprob}/batch"), book.get(f"{shape}/{nprob}/loop")
if b and l:
    book[f"{shape}/{nprob}/ratio_loop_over_batch"] = l["ms_median"] / b["ms_median"]
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
