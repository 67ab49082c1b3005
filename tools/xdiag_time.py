#!/usr/bin/env python3
"""pls_hip_x_diagnostics on a device-resident matrix: time, algorithmic bytes and flops, and the torch composition a caller
had to write before the entry point existed.
   python tools/xdiag_time.py [c3 | c4 | N K A [f32]] [--profile] [--no-torch]
Default: device memory, 3 warm-up calls, then 20 calls of the library and 20 of the torch composition ALTERNATING in one
process, each bracketed by HIP events; prints median (min - max) and one JSON line.
--profile: 22 library calls and nothing else (for `rocprofv3 --kernel-trace --stats -- python tools/xdiag_time.py c3 --profile`:
the profiler run is separate from the timed run).
Algorithmic traffic of the general (two-sweep) route, s = bytes per element of X, ranges = ceil(A / 24):
   scores   N K s (fp32 storage: once per range) + N A 8          2 N K A flops
   sweep    ranges * N K s + N A 8 (scores in) + N A 8 (Q out)    4 N K A flops  (+ the rebuild below a range's first count)
The model comes from a fit of the library itself on the same matrix (it is an input here, not what is measured)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import pls_amd

SHAPES = {"c3": (1 << 20, 512, 20, "f64"), "c4": (131072, 4096, 50, "f32")}
args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = {a for a in sys.argv[1:] if a.startswith("--")}
if args and args[0] in SHAPES:
    N, K, A, st = SHAPES[args[0]]
elif len(args) >= 3:
    N, K, A = (int(v) for v in args[:3])
    st = "f32" if len(args) > 3 and args[3] == "f32" else "f64"
else:
    N, K, A, st = SHAPES["c3"]
dt = torch.float32 if st == "f32" else torch.float64
s = 4 if st == "f32" else 8
ranges = -(-A // 24)

h = pls_amd.Handle()
X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
Y = h.synth_y(0, N, 1, pls_amd.SEED_DEFAULT, dtype=dt)
fit = h.fit_device(X, Y, A, want_B=False)
h.synchronize()
R, P = fit["R"], fit["P"]
del fit, Y

bytes_scores = N * K * s * (ranges if st == "f32" else 1) + N * A * 8
bytes_sweep = ranges * N * K * s + 2 * N * A * 8
rebuild = sum(2 * N * K * c_lo for c_lo in range(0, A, 24))          # flops of the components re-applied below each range
flops = 6 * N * K * A + rebuild
model = {"bytes_scores": bytes_scores, "bytes_sweep": bytes_sweep, "flops": flops,
         "bound_ms_bytes_6.29TBps": (bytes_scores + bytes_sweep) / 6.29e12 * 1e3,
         "bound_ms_flops_78.6TF_datasheet": flops / 78.6e12 * 1e3}


def lib_call():
    return h.x_diagnostics(X, R, P, want=("Q", "T2", "ssx"))


def torch_call():
    """what a caller can do without the entry point: S = X R, then A rank-1 updates of a copy of X and A row sums"""
    Xd = X.to(torch.float64)
    S = Xd @ R
    F = Xd.clone()
    Q = torch.empty((N, A), dtype=torch.float64, device=X.device)
    for c in range(A):
        F -= torch.outer(S[:, c], P[:, c])
        Q[:, c] = (F * F).sum(1)
    tv = (S * S).sum(0) / (N - 1)
    T2 = torch.cumsum(S * S / tv, dim=1)
    return Q, T2


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1)


if "--profile" in flags:
    for _ in range(22):
        lib_call()
    h.synchronize()
    print(json.dumps({"shape": [N, K, A, st], "calls": 22, **model}))
    sys.exit(0)

use_torch = "--no-torch" not in flags
for _ in range(3):
    lib_call()
    if use_torch:
        torch_call()
torch.cuda.synchronize()
tl, tt = [], []
for _ in range(20):
    tl.append(timed(lib_call))
    if use_torch:
        tt.append(timed(torch_call))
fmt = lambda v: f"{statistics.median(v):.3f} ms ({min(v):.3f} - {max(v):.3f})"
print(f"N={N} K={K} A={A} {st}: pls_hip_x_diagnostics (Q, T2, ssx) {fmt(tl)}")
res = {"shape": [N, K, A, st], "lib_ms_median": statistics.median(tl), "lib_ms_min": min(tl), "lib_ms_max": max(tl), **model}
if use_torch:
    print(f"                     torch composition              {fmt(tt)}   ratio {statistics.median(tt) / statistics.median(tl):.1f}")
    res.update(torch_ms_median=statistics.median(tt), torch_ms_min=min(tt), torch_ms_max=max(tt),
               ratio=statistics.median(tt) / statistics.median(tl))
print(json.dumps(res))
