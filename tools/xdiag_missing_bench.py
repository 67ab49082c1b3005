#!/usr/bin/env python3
"""pls_hip_x_diagnostics_missing against what a user has to run without it, on one GPU.
   python tools/xdiag_missing_bench.py {c3 | wide | f32} [--mode new | baseline] [--lib FILE] [--route stream] [--missing PERCENT]
                                       [--reps N] [--label NAME] [--json FILE]
Shapes:  c3 = 1,048,576 x 512 fp64, A = 20    wide = 500 x 200,000 fp64, A = 10    f32 = 2,000 x 50,000 fp32, A = 10.
Device-resident synthetic data with PERCENT (default 10) of the cells of X set to NaN, W with unit columns and P random.
--mode new (default): pls_hip_x_diagnostics_missing with every output asked for ("all") and with S alone ("S"): ms per call, HIP
    events around the call and its synchronisation, profiling off.  Then, from calls under PLS_HIP_OPT_PROFILE = 1, the sweeps over
    X of the "all" call: launches, milliseconds, N K es bytes per read of X and their share of 8 TB/s.  --route stream sets
    PLS_HIP_XDIAGMISS_ROUTE=stream before the handle is created (the streaming route on a shape whose default is the resident one).
--mode baseline: pls_hip_scores_missing alone -- it yields only S, a lower bound of what a user runs today.  --lib FILE: another
    build of the library (the parent commit's, for a comparison in one session); only the entry points it exports are bound.
One warm-up call per timed series, then --reps (default 5) repetitions; the median is reported.  One JSON line per run is printed
and APPENDED to the list under "<shape>/<label>" of FILE (default profiles/xdiag_missing/xdiag_missing_bench.json)."""
import ctypes
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


mode = opt("--mode") or "new"
lib_path = opt("--lib")
route = opt("--route")
missing = float(opt("--missing") or 10.0)
reps = int(opt("--reps") or 5)
label = opt("--label")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "xdiag_missing", "xdiag_missing_bench.json")
args = [a for a in argv if not a.startswith("--")]
label = label or (mode + ("-stream" if route == "stream" else "") + ("-lib" if lib_path else ""))
sys.path.insert(0, ROOT)
if lib_path:
    os.environ["PLS_AMD_LIBRARY"] = os.path.abspath(lib_path)
if route:
    os.environ["PLS_HIP_XDIAGMISS_ROUTE"] = route

from pls_amd import _lib  # noqa: E402

if lib_path:  # an older build: bind what it exports
    probe = ctypes.CDLL(os.path.abspath(lib_path))
    _lib.PROTOTYPES = [p for p in _lib.PROTOTYPES if hasattr(probe, p[0])]

import torch  # noqa: E402

import pls_amd  # noqa: E402

SHAPES = {"c3": (1 << 20, 512, "f64", 20), "wide": (500, 200000, "f64", 10), "f32": (2000, 50000, "f32", 10)}
shape = args[0] if args else "c3"
N, K, st, A = SHAPES[shape]
dt = torch.float32 if st == "f32" else torch.float64
es = 4 if st == "f32" else 8
PEAK = 8e12
NK = N * K * es  # one read of the matrix

stream = torch.cuda.Stream()
rec = {"shape": [N, K, st], "A": A, "mode": mode, "label": label, "reps": reps, "missing_percent": missing,
       "library": lib_path or "this tree", "route_switch": route or "default"}

with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for k0 in range(0, K, 4096):  # (column blocks: no N x K temporary of the mask)
        blk = X[:, k0:k0 + 4096]
        blk[torch.rand(blk.shape, device="cuda", generator=g) < missing / 100.0] = float("nan")
    W = torch.randn(K, A, dtype=torch.float64, device="cuda", generator=g)
    W = W / W.norm(dim=0)
    P = torch.randn(K, A, dtype=torch.float64, device="cuda", generator=g) / K ** 0.5
    h.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        q = f()
        h.synchronize()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), q

    def median_ms(f):
        timed(f)  # warm-up: workspace, code objects
        return statistics.median(timed(f)[0] for _ in range(reps))

    if mode == "new":
        every = ("Q", "T2", "S", "ssx", "sst", "nobs")
        rec["all_ms"] = median_ms(lambda: h.x_diagnostics_missing(X, W, P, want=every))
        rec["S_ms"] = median_ms(lambda: h.x_diagnostics_missing(X, W, P, want=("S",)))
        out = h.x_diagnostics_missing(X, W, P, want=every)
        h.synchronize()
        rec["finite"] = bool(all(torch.isfinite(out[k]).all() for k in ("Q", "T2", "S", "ssx", "sst")))
        h.set_option(pls_amd.OPT_PROFILE, 1)
        h.x_diagnostics_missing(X, W, P, want=every); h.synchronize(); h.timing()
        runs = []
        for _ in range(reps):
            h.x_diagnostics_missing(X, W, P, want=every); h.synchronize()
            runs.append(h.timing())
        h.set_option(pls_amd.OPT_PROFILE, 0)
        ms = statistics.median(r["ms"]["xb"] for r in runs)
        n = runs[0]["launches"]["xb"]
        rec["sweeps"] = {"launches": n, "ms": ms, "reads_of_X": n, "TB/s": n * NK / (ms * 1e-3) / 1e12, "of_8TB/s": n * NK / (ms * 1e-3) / PEAK}
    else:
        rec["S_ms"] = median_ms(lambda: h.scores_missing(X, W, P))

print(f"{shape} N={N} K={K} {st} A={A} [{label}]")
for k in ("all_ms", "S_ms"):
    if k in rec:
        print(f"  {k:10s} {rec[k]:9.3f} ms")
if "sweeps" in rec:
    s = rec["sweeps"]
    print(f"  sweeps over X: {s['launches']} launches, {s['ms']:.3f} ms, {s['TB/s']:.2f} TB/s over N K es per read = {s['of_8TB/s']:.3f} of 8 TB/s")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{shape}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
