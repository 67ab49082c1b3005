#!/usr/bin/env python3
"""The sweeps of pls_hip_fit_missing against their unmasked counterparts, on one GPU.
   python tools/missing_bench.py {c3 | wide | f32} [--missing PERCENT] [--mode masked | unmasked] [--lib FILE] [--reps N]
                                 [--label NAME] [--json FILE]
Shapes:  c3 = 1,048,576 x 512 fp64, A = 20    wide = 500 x 200,000 fp64, A = 10    f32 = 2,000 x 50,000 fp32, A = 10;  M = 1.
--mode masked (default): pls_hip_fit_missing on X with PERCENT (default 0) of its cells set to NaN.  Reported: ms per fit (HIP
    events around the call and its synchronisation, profiling off) and, from a second set of calls under PLS_HIP_OPT_PROFILE = 1,
    per sweep the milliseconds, the algorithmic bytes and their share of 8 TB/s: "deflate+w" (reads X_a-1, writes X_a; the
    first of a fit reads the caller's matrix), "t" (the row sweep; its bytes include the partials of the K-split) and "p".
--mode unmasked: the counterparts on complete data -- pls_hip_xty with one response (the column sweep), pls_hip_xb with one
    column (the row sweep), pls_hip_deflate (read + write), each under PLS_HIP_OPT_PROFILE = 1, and the whole pls_hip_fit under
    PLS_HIP_ALGO_NIPALS with PLS_HIP_OPT_FUSE = 0 and = 1 (events, profiling off).  --lib FILE: another build of the library (the
    parent commit's, for a comparison in one session); only the entry points it exports are bound.
Data from the device generator, a stream of its own, one warm-up call per timed call, then --reps (default 5) repetitions; the
median is reported.  One JSON line per run is printed and APPENDED to the list under "<shape>/<label>" of FILE (default
profiles/missing/missing_bench.json).  The sweeps are HBM-bound streams: 8 TB/s is the datasheet peak, a float4 copy reaches
6.3 TB/s of it."""
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


mode = opt("--mode") or "masked"
missing = float(opt("--missing") or 0.0)
lib_path = opt("--lib")
reps = int(opt("--reps") or 5)
label = opt("--label")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "missing", "missing_bench.json")
args = [a for a in argv if not a.startswith("--")]
label = label or (f"masked-{missing:g}" if mode == "masked" else "unmasked" + ("-lib" if lib_path else ""))
sys.path.insert(0, ROOT)
if lib_path:
    os.environ["PLS_AMD_LIBRARY"] = os.path.abspath(lib_path)

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
rec = {"shape": [N, K, st], "A": A, "M": 1, "mode": mode, "label": label, "reps": reps, "library": lib_path or "this tree"}


def sweep(ms, nbytes):
    return {"ms": ms, "bytes": nbytes, "TB/s": nbytes / (ms * 1e-3) / 1e12, "of_8TB/s": nbytes / (ms * 1e-3) / PEAK}


with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=dt)
    Y = h.synth_y(0, N, 1, pls_amd.SEED_DEFAULT, dtype=dt)
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

    def profiled(f):
        """per family: (ms, launches, library bytes) per call of f under PLS_HIP_OPT_PROFILE = 1, median over the repetitions"""
        h.set_option(pls_amd.OPT_PROFILE, 1)
        f(); h.synchronize(); h.timing()
        runs = []
        for _ in range(reps):
            f(); h.synchronize()
            runs.append(h.timing())
        h.set_option(pls_amd.OPT_PROFILE, 0)
        return {fam: (statistics.median(r["ms"][fam] for r in runs), runs[0]["launches"][fam], runs[0]["bytes"][fam])
                for fam in ("xty", "xb", "deflate")}

    if mode == "masked":
        if missing > 0:
            g = torch.Generator(device="cuda"); g.manual_seed(1)
            for k0 in range(0, K, 4096):  # (column blocks: no N x K temporary of the mask)
                blk = X[:, k0:k0 + 4096]
                blk[torch.rand(blk.shape, device="cuda", generator=g) < missing / 100.0] = float("nan")
        rec["missing_percent"] = missing
        fit = lambda: h.fit_missing(X, Y, A, want=("W", "P", "Q", "R", "T", "B"))
        rec["fit_ms"] = median_ms(fit)
        rec["finite"] = bool(torch.isfinite(fit()["B"]).all())
        p = profiled(fit)
        rec["sweeps"] = {"deflate+w": sweep(p["deflate"][0] / p["deflate"][1], 2 * NK), "t": sweep(p["xb"][0] / p["xb"][1], p["xb"][2] // p["xb"][1]),
                         "p": sweep(p["xty"][0] / p["xty"][1], NK)}
        rec["launches_per_fit"] = {k: v[1] for k, v in p.items()}
    else:
        Bm = pls_amd.colmajor_empty(K, 1, torch.float64, "cuda", ld=K); Bm.fill_(1.0 / K)
        Z = pls_amd.colmajor_empty(N, K, dt, "cuda")
        tvec = Y[:, 0].contiguous()
        pvec = Bm[:, 0].contiguous()
        sw = {}
        p = profiled(lambda: h.xty(X, Y))
        sw["xty (column sweep)"] = sweep(p["xty"][0], NK)
        p = profiled(lambda: h.xb(X, Bm))
        sw["xb, 1 column (row sweep)"] = sweep(p["xb"][0], NK)
        p = profiled(lambda: h.deflate(X, tvec, pvec, dst=Z))
        sw["deflate (read + write)"] = sweep(p["deflate"][0], 2 * NK)
        rec["sweeps"] = sw
        del Z
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        out = None
        for fuse in (0, 1):
            h.set_option(pls_amd.OPT_FUSE, fuse)
            rec[f"nipals_fit_ms_fuse{fuse}"] = median_ms(lambda: h.fit_device(X, Y, A))

print(f"{shape} N={N} K={K} {st} A={A} [{label}]")
for k, v in rec.get("sweeps", {}).items():
    print(f"  {k:28s} {v['ms']:9.3f} ms  {v['bytes'] / 1e9:8.3f} GB  {v['TB/s']:.2f} TB/s  {v['of_8TB/s']:.3f} of 8 TB/s")
for k in ("fit_ms", "nipals_fit_ms_fuse0", "nipals_fit_ms_fuse1"):
    if k in rec:
        print(f"  {k:28s} {rec[k]:9.3f} ms")
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{shape}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
