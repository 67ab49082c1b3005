#!/usr/bin/env python3
"""Back-to-back time of the one-workgroup single-launch kernels (tiny_fit_kernel, tiny_fit_m_kernel: fits and fold calls), which
tools/small_fit_time.py and tools/resident_check.py do not reach with more than one response: best of 5 runs of 200 calls, in us.
Honours PLS_AMD_LIBRARY, to compare two builds in alternating processes.
    python tools/one_workgroup_time.py out.json"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, pls_amd
h = pls_amd.Handle()


def best_us(call):
    call(); h.synchronize()
    best = 1e30
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(200): call()
        h.synchronize(); best = min(best, (time.perf_counter() - t0) / 200 * 1e6)
    return round(best, 2)


out = {}
for (N, K, M, A, dt) in ((60, 40, 4, 6, "f64"), (64, 300, 8, 5, "f64"), (130, 100, 3, 7, "f64"), (700, 26, 8, 4, "f64"), (1000, 20, 2, 6, "f32"),
                         (200, 50, 2, 4, "f64"), (200, 50, 6, 4, "f32"), (65, 200, 1, 8, "f64"), (1024, 26, 1, 6, "f64"), (1000, 20, 1, 6, "f32")):
    tdt = torch.float64 if dt == "f64" else torch.float32
    X = h.synth_x(0, N, K, 31, dtype=tdt); Y = h.synth_y(0, N, M, 31, dtype=tdt)
    o = h.fit_device(X, Y, A)
    out["fit N=%d K=%d M=%d A=%d %s us" % (N, K, M, A, dt)] = best_us(lambda: h.fit_device(X, Y, A, out=o))
rng = np.random.default_rng(5)
for (N, K, M, A, nf, ts) in ((300, 24, 1, 5, 30, 6), (200, 24, 3, 5, 20, 7), (90, 30, 4, 5, 12, 27), (200, 24, 8, 5, 20, 7)):
    X = h.synth_x(0, N, K, 31); Y = h.synth_y(0, N, M, 31)
    idx = np.stack([rng.permutation(N)[:ts] for _ in range(nf)])
    out["folds N=%d K=%d M=%d A=%d %dx%d us" % (N, K, M, A, nf, ts)] = best_us(lambda: h.cv_folds(X, Y, A, idx))
json.dump(out, open(sys.argv[1], "w"), indent=1)
