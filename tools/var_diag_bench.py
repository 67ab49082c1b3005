#!/usr/bin/env python3
"""pls_hip_var_diagnostics against pls_hip_x_diagnostics on a device-resident matrix: the column sweep (vardiag_sweep_kernel) next to
the row sweep (xdiag_sweep_kernel), which moves the same algorithmic bytes and does the same flops, reduced along the other axis.
   python tools/var_diag_bench.py [c3 | c4f32 | wide | N K A [f32]] [--launches n]
3 warm-up calls of each entry, then n (default 50) calls of each, ALTERNATING in one process, each bracketed by HIP events; prints
median (min - max) per call and one JSON line: the per-CALL times, to be taken WITHOUT the profiler.  The per-kernel times come
from the profiler, in a run of its own (its per-call lines carry the tracer's overhead and are not the ones to quote):
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/var_diag_bench.py c3
   python tools/var_diag_bench.py c3 --trace DIR/.../NAME_kernel_trace.csv
The second line reads the trace and prints, for both sweep kernels: launches, median, min, max and (max - min) / median per launch
of a range, the bytes over time against the 6.29 TB/s copy ceiling and the flops over time -- and the gate: the column sweep's
median against the row sweep's median of the same run, with the row sweep's own spread between repeats, the only margin, next to it.
Algorithmic traffic of one sweep over a range of nc counts that ends at c_hi (s = bytes per element of X):
   bytes  N K s + 8 N c_hi (scores in) + 8 N nc (row sweep: Q out) | 8 K (nc + 1) RS (column sweep: partial sums out)
   flops  4 N K nc + 2 N K c_lo (the components below the range, re-applied)
The model is a fit of the library itself on the same matrix (an input here, not what is measured)."""
import csv
import json
import os
import statistics
import sys

SHAPES = {"c3": (1 << 20, 512, 20, "f64"), "c4f32": (131072, 4096, 50, "f32"), "wide": (2000, 100000, 10, "f64")}
CEILING = 6.29e12
args = [a for a in sys.argv[1:] if not a.startswith("--")]
opts = sys.argv[1:]
launches = int(opts[opts.index("--launches") + 1]) if "--launches" in opts else 50
trace = opts[opts.index("--trace") + 1] if "--trace" in opts else None
args = [a for a in args if a not in (str(launches), trace)]
if args and args[0] in SHAPES:
    name = args[0]
    N, K, A, st = SHAPES[name]
elif len(args) >= 3:
    N, K, A = (int(v) for v in args[:3])
    st = "f32" if len(args) > 3 and args[3] == "f32" else "f64"
    name = f"{N}x{K}-a{A}-{st}"
else:
    name = "c3"
    N, K, A, st = SHAPES[name]
s = 4 if st == "f32" else 8
ranges = [(lo, min(A, lo + 24)) for lo in range(0, A, 24)]


def sweep_model(lo, hi):
    return N * K * s + 8 * N * hi + 8 * N * (hi - lo), 4 * N * K * (hi - lo) + 2 * N * K * lo


def summarise(path):
    """per-launch durations of the two sweep kernels from a rocprofv3 kernel trace; launches of one kernel come range by range"""
    rows = {"row": [], "col": []}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            kn = r["Kernel_Name"]
            key = "col" if "vardiag_sweep_kernel" in kn else "row" if "xdiag_sweep_kernel" in kn else None
            if key:
                rows[key].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    out = {"shape": name, "N": N, "K": K, "A": A, "storage": st, "source": os.path.basename(path)}
    for key, v in rows.items():
        v = [d for _, d in sorted(v)]
        v = v[3 * len(ranges):]   # the warm-up calls
        for j, (lo, hi) in enumerate(ranges):
            d = v[j::len(ranges)]
            if not d:
                continue
            b, fl = sweep_model(lo, hi)
            med = statistics.median(d)
            out[f"{key}_sweep_range{j}"] = {"counts": [lo + 1, hi], "launches": len(d), "median_us": med, "min_us": min(d), "max_us": max(d),
                                           "spread": (max(d) - min(d)) / med, "bytes": b, "of_copy_ceiling": b / (med * 1e-6) / CEILING,
                                           "TF": fl / (med * 1e-6) / 1e12}
        out[f"{key}_sweep_total_median_us"] = sum(out[f"{key}_sweep_range{j}"]["median_us"] for j in range(len(ranges)) if f"{key}_sweep_range{j}" in out)
    if "row_sweep_range0" in out and "col_sweep_range0" in out:
        r, c = out["row_sweep_range0"], out["col_sweep_range0"]
        out["gate"] = {"column_median_us": c["median_us"], "row_median_us": r["median_us"], "column_over_row": c["median_us"] / r["median_us"],
                       "column_no_longer_than_row": c["median_us"] <= r["median_us"], "row_min_us": r["min_us"], "row_max_us": r["max_us"],
                       "row_spread": r["spread"]}
    print(json.dumps(out, indent=1))


if trace is not None:
    summarise(trace)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import pls_amd  # noqa: E402

dt = torch.float32 if st == "f32" else torch.float64
h = pls_amd.Handle()
X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
Y = h.synth_y(0, N, 1, pls_amd.SEED_DEFAULT, dtype=dt)
if N >= K:
    fit = h.fit_device(X, Y, A, want_B=False)
    h.synchronize()
    W, R, P, Q = (fit[k] for k in "WRPQ")
    del fit
else:   # short and wide: any model will do for a time
    g = torch.Generator(device="cuda").manual_seed(1)
    W, R, P = (pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K).copy_(torch.randn(K, A, generator=g, device="cuda", dtype=torch.float64) / K ** 0.5)
               for _ in range(3))
    Q = torch.ones(1, A, dtype=torch.float64, device="cuda")
del Y


def row_call():
    return h.x_diagnostics(X, R, P, want=("Q", "T2", "ssx"))


def col_call():
    return h.var_diagnostics(X, W=W, R=R, P=P, Q=Q, want=("VIP", "ssxk"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


for _ in range(3):
    row_call(); col_call()
h.synchronize()
torch.cuda.synchronize()
t_row, t_col = [], []
for _ in range(launches):
    t_row.append(timed(row_call))
    t_col.append(timed(col_call))
fmt = lambda v: f"{statistics.median(v):.3f} ms ({min(v):.3f} - {max(v):.3f})"
print(f"{name}: {N} x {K} {st}, A = {A}, {launches} calls each, alternating")
print(f"  pls_hip_x_diagnostics   (Q, T2, ssx)   {fmt(t_row)}")
print(f"  pls_hip_var_diagnostics (VIP, ssxk)    {fmt(t_col)}")
print(json.dumps({"shape": name, "N": N, "K": K, "A": A, "storage": st, "launches": launches,
                  "x_diagnostics_ms": {"median": statistics.median(t_row), "min": min(t_row), "max": max(t_row)},
                  "var_diagnostics_ms": {"median": statistics.median(t_col), "min": min(t_col), "max": max(t_col)}}))
h.close()
