#!/usr/bin/env python3
"""One pls_hip_fit_batch call on a short, wide device-resident X with PLS_HIP_ALGO_DUAL set: every problem from one X X^T
(plan_dual_batch.hpp) against what the library does without that route -- a loop of DUAL pls_hip_fit calls, one per problem
(the wide shapes, where nothing else runs), or pls_hip_fit_batch on the X^T X route (the cross-over shape).
   python tools/dual_batch_bench.py {w1 | w2 | x} [--mode batch | fits | plain] [--B] [--sweeps] [--nprob N] [--label NAME]
                                    [--json FILE] [--reps N]
Calls:  w1 = 500 x 200,000 fp64    w2 = 2,000 x 50,000 fp64    x = 500 x 16,384 fp64 (the X^T X route covers it);  M = 1, A = 5.
--mode batch (default): fit_batch of 1,001 problems under ALGO_DUAL, want = (Q, tt, ssy), with --B also B.
--mode fits:   100 DUAL pls_hip_fit calls, one per problem (with --B each forms its B); the figure is for the 100.
--mode plain:  fit_batch of 1,001 problems on a handle without the option (the X^T X route; shape x only).
--sweeps: PLS_HIP_DUALBATCH_SWEEPS=1, the back-projection beyond 64 columns as one sweep per 64 columns.
Neither baseline runs code this route changes, so both are measured in the same tree, alternating with the batched call.
Data from the device generator, a stream of its own, one warm-up call (two where a call takes less than half a second), then
repeated calls each bracketed by HIP events on the handle's stream around the call and its synchronisation: 20 of them, or 3
where a call takes more than half a second (--reps overrides).  The median (min - max) is printed and APPENDED to the list
under "<call>/<label>" of FILE (default profiles/dual/batch_bench.json).  With --B a last call under PLS_HIP_OPT_PROFILE=1
reports the time of the back-projection launches alone (the xty family less the X X^T sweep of a call without B) and its
rate, 2 N K nprob M flops, as a fraction of the 78.6 TF fp64 matrix rate."""
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


mode = opt("--mode") or "batch"
label = opt("--label")
json_path = opt("--json") or os.path.join(ROOT, "profiles", "dual", "batch_bench.json")
reps = opt("--reps")
nprob = int(opt("--nprob") or (100 if mode == "fits" else 1001))
flags = {a for a in argv if a.startswith("--")}
args = [a for a in argv if not a.startswith("--")]
want_b = "--B" in flags
if "--sweeps" in flags:
    os.environ["PLS_HIP_DUALBATCH_SWEEPS"] = "1"
label = label or (mode + ("+B" if want_b else "") + ("+sweeps" if "--sweeps" in flags else ""))
sys.path.insert(0, ROOT)

import torch

import pls_amd

CALLS = {"w1": (500, 200000), "w2": (2000, 50000), "x": (500, 16384)}
call = args[0] if args else "w1"
N, K = CALLS[call]
M, A = 1, 5
PEAK_TF = 78.6
want = ("Q", "tt", "ssy", "B") if want_b else ("Q", "tt", "ssy")

stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    h = pls_amd.Handle(stream=stream.cuda_stream)
    if mode != "plain":
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_DUAL)
    X = h.synth_x(0, N, K, pls_amd.SEED_DEFAULT)
    Ys = h.synth_y(0, N, nprob * M, pls_amd.SEED_DEFAULT)
    h.synchronize()
    cols = [pls_amd.as_colmajor(Ys[:, b * M:(b + 1) * M].clone()) for b in range(nprob)] if mode == "fits" else None
    out = None

    def once():
        global out
        if mode == "fits":
            for b in range(nprob):
                out = h.fit_device(X, cols[b], A, pls_amd.KERNEL_TYPE1, want_B=want_b, out=out)
            return out["Q"]
        return h.fit_batch(X, Ys, M, A, want=want)["Q"]

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
    rec = {"call": call, "shape": [N, K, "f64"], "M": M, "A": A, "nprob": nprob, "mode": mode, "want": list(want), "label": label,
           "reps": n, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "Q_finite": finite}
    if want_b and mode == "batch":
        h.set_option(pls_amd.OPT_PROFILE, 1)
        fam = {}
        for w in (("Q", "tt", "ssy"), want):
            h.timing()
            h.fit_batch(X, Ys, M, A, want=w)
            h.synchronize()
            fam[len(w)] = h.timing()
        h.set_option(pls_amd.OPT_PROFILE, 0)
        back = fam[4]["ms"]["xty"] - fam[3]["ms"]["xty"]
        tf = 2.0 * N * K * nprob * M / (back * 1e-3) / 1e12
        rec.update(xxt_ms=fam[3]["ms"]["xty"], backproj_ms=back, backproj_launches=fam[4]["launches"]["xty"] - fam[3]["launches"]["xty"],
                   backproj_tf=tf, backproj_of_peak=tf / PEAK_TF)

print(f"{call} N={N} K={K} M={M} A={A} nprob={nprob} [{label}]: {rec['ms_median']:.3f} ms "
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
