#!/usr/bin/env python3
"""pls_hip_cv_folds_missing against what a user had before it, on one GPU.
   python tools/missing_cv_bench.py {small | tall} [--mode new | baseline] [--lib FILE] [--reps N] [--label NAME] [--json FILE]
Shapes, both fp64, M = 1, 10 % of the cells of X NaN, device-resident synthetic data:
   small = 200 x 2,000, A = 5, leave-one-out (200 folds)        tall = 1,048,576 x 512, A = 10, 5 contiguous folds
--mode new (default): one pls_hip_cv_folds_missing call.
--mode baseline, with --lib FILE the parent commit's library (run in the same session; only the entry points it exports are
    bound):  small: the per-fold loop a user writes without the call -- gather the training rows with torch, fit_missing,
    scores_missing on the held-out rows, xb for the fitted values -- over all 200 folds;  tall: ONE pls_hip_fit_missing of the
    whole (X, Y) with the same A, to be compared with the new call's time PER FOLD.
One warm-up call, then --reps (default 5) timed calls (HIP events around the call and its synchronisation); the median is
reported.  One JSON line per run is printed and APPENDED to the list under "<shape>/<label>" of FILE (default
profiles/missing/missing_cv_bench.json)."""
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
reps = int(opt("--reps") or 5)
label = opt("--label") or (mode + ("-lib" if lib_path else ""))
json_path = opt("--json") or os.path.join(ROOT, "profiles", "missing", "missing_cv_bench.json")
args = [a for a in argv if not a.startswith("--")]
sys.path.insert(0, ROOT)
if lib_path:
    os.environ["PLS_AMD_LIBRARY"] = os.path.abspath(lib_path)

from pls_amd import _lib  # noqa: E402

if lib_path:  # an older build: bind what it exports
    probe = ctypes.CDLL(os.path.abspath(lib_path))
    _lib.PROTOTYPES = [p for p in _lib.PROTOTYPES if hasattr(probe, p[0])]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pls_amd  # noqa: E402

SHAPES = {"small": (200, 2000, 5, 200, 1), "tall": (1 << 20, 512, 10, 5, (1 << 20) // 5)}  # N, K, A, folds, rows held out per fold
shape = args[0] if args else "small"
N, K, A, nf, ts = SHAPES[shape]
idx = np.arange(nf * ts, dtype=np.int64).reshape(nf, ts)  # contiguous folds (small: every row once)
rec = {"shape": [N, K, "f64"], "A": A, "M": 1, "folds": nf, "test_size": ts, "missing_percent": 10.0, "mode": mode, "label": label,
       "reps": reps, "library": lib_path or "this tree", "device": torch.cuda.get_device_name(0)}

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT, dtype=torch.float64)
    Y = h.synth_y(0, N, 1, pls_amd.SEED_DEFAULT, dtype=torch.float64)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for k0 in range(0, K, 64):  # (column blocks: no N x K temporary of the mask)
        blk = X[:, k0:k0 + 64]
        blk[torch.rand(blk.shape, device="cuda", generator=g) < 0.10] = float("nan")
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
        call = lambda: h.cv_folds_missing(X, Y, A, idx)
        rec["call_ms"] = median_ms(call)
        rec["per_fold_ms"] = rec["call_ms"] / nf
        rec["finite"] = bool(torch.isfinite(call()).all())
    elif shape == "small":
        rows = torch.arange(N, device="cuda")

        def loop():
            E = torch.empty((nf * ts, A), dtype=torch.float64, device="cuda")
            for f in range(nf):
                held = torch.from_numpy(idx[f]).cuda()
                keep = torch.ones(N, dtype=torch.bool, device="cuda")
                keep[held] = False
                tr = rows[keep]
                Xt = pls_amd.colmajor_empty(N - ts, K, torch.float64, "cuda"); Xt.copy_(X[tr])
                Yt = pls_amd.colmajor_empty(N - ts, 1, torch.float64, "cuda"); Yt.copy_(Y[tr])
                Xh = pls_amd.colmajor_empty(ts, K, torch.float64, "cuda"); Xh.copy_(X[held])
                m = h.fit_missing(Xt, Yt, A, want=("W", "P", "Q", "R", "T"))
                S = h.scores_missing(Xh, m["W"], m["P"])
                fitted = h.xb(S, m["Q"].t())   # all A components; the residuals of 1 .. A - 1 would be more calls still
                E[f * ts:(f + 1) * ts, A - 1] = Y[held, 0] - fitted[:, 0]
            return E
        rec["call_ms"] = median_ms(loop)
        rec["per_fold_ms"] = rec["call_ms"] / nf
        rec["finite"] = bool(torch.isfinite(loop()[:, A - 1]).all())
    else:
        fit = lambda: h.fit_missing(X, Y, A, want=("W", "P", "Q", "R", "T"))
        rec["call_ms"] = median_ms(fit)
        rec["finite"] = bool(torch.isfinite(fit()["Q"]).all())

print(f"{shape} N={N} K={K} f64 A={A} folds={nf} [{label}]  " + "  ".join(f"{k} {rec[k]:.3f}" for k in ("call_ms", "per_fold_ms") if k in rec))
print(json.dumps(rec))
os.makedirs(os.path.dirname(json_path), exist_ok=True)
book = {}
if os.path.exists(json_path):
    with open(json_path) as f:
        book = json.load(f)
book.setdefault(f"{shape}/{label}", []).append(rec)
with open(json_path, "w") as f:
    json.dump(book, f, indent=1, sort_keys=True)
