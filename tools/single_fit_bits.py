#!/usr/bin/env python3
"""One SHA-256 per case over the bytes of W, P, Q, R, T, B (fits) or E (fold calls) of the single-launch kernels
(tiny_kernels.hpp, resident_kernels.hpp): run under two builds of the library (PLS_AMD_LIBRARY), the outputs must be equal
line for line.  The fits are the shapes of test_single_launch_fit, test_single_launch_fit_several_responses and
test_resident_single_launch_fit, and 1..8 responses at one shape of each kind; the fold calls one per fold kernel.
    python tools/single_fit_bits.py [out.txt]"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, pls_amd

DATA = os.path.join(ROOT, "tests", "golden", "data")
h = pls_amd.Handle()


def zs(name):  # z-scores of a data file (src/pls.cpp:69-88)
    x = np.loadtxt(os.path.join(DATA, name), delimiter=",", ndmin=2, dtype=np.float64)
    return torch.from_numpy(np.asfortranarray((x - x.mean(0)) / x.std(0, ddof=1))).cuda()


def digest(tensors):
    d = hashlib.sha256()
    for t in tensors:
        d.update(t.cpu().contiguous().numpy().tobytes())
    return d.hexdigest()


FITS = [(60, 401, 1, 10, "f64", 0), (64, 416, 1, 12, "f64", 3), (10, 15, 1, 3, "f64", 0), (65, 200, 1, 8, "f64", 1), (130, 120, 1, 9, "f64", 0),
        (1024, 26, 1, 6, "f64", 0), (1000, 20, 1, 6, "f32", 8), (1, 5, 1, 1, "f64", 0),
        (10, 15, 2, 2, "f64", 0), (60, 40, 4, 6, "f64", 3), (64, 300, 8, 5, "f64", 0), (130, 100, 3, 7, "f64", 1), (1000, 20, 2, 6, "f32", 8),
        (700, 26, 8, 4, "f64", 0), (5, 7, 2, 3, "f64", 0),
        (1025, 26, 1, 5, "f64", 0), (5000, 128, 1, 10, "f64", 0), (4001, 416, 1, 6, "f64", 3), (20000, 16, 1, 5, "f64", 1), (100000, 40, 1, 12, "f64", 0),
        (262144, 26, 1, 4, "f64", 0), (3001, 77, 1, 7, "f32", 5), (70000, 50, 1, 9, "f32", 0), (1024, 40, 1, 6, "f64", 0), (1025, 26, 3, 5, "f64", 0),
        (5000, 128, 4, 8, "f64", 2), (4001, 416, 2, 5, "f64", 0), (100000, 40, 8, 12, "f64", 0), (3001, 77, 5, 7, "f32", 1), (2000, 300, 8, 4, "f64", 0)]
FITS += [(200, 50, M, 4, dt, 1) for M in range(1, 9) for dt in ("f64", "f32")] + [(3000, 50, M, 4, dt, 1) for M in range(1, 9) for dt in ("f64", "f32")]
lines = []
for N, K, M, A, dt, pad in FITS:
    tdt = torch.float64 if dt == "f64" else torch.float32
    if (N, K) == (60, 401):
        X, Y = zs("nir.csv"), zs("octane.csv")
    elif (N, K, M) == (10, 15, 2):
        X, Y = zs("toyX.csv"), zs("toyY.csv")
    else:
        X, Y = h.synth_x(0, N, K, 31, dtype=tdt), h.synth_y(0, N, M, 31, dtype=tdt)
    Xbig = torch.zeros((K, N + pad), dtype=tdt, device="cuda")
    Xbig[:, :N] = X.T
    out = h.fit_device(Xbig.T[:N], Y, A)  # column-major view, ld = N + pad
    h.synchronize()
    lines.append("fit N=%d K=%d M=%d A=%d %s pad=%d  %s" % (N, K, M, A, dt, pad, digest(out[k] for k in "WPQRTB")))
rng = np.random.default_rng(5)
FOLDS = [("tiny 300x24 M=1", h.synth_x(0, 300, 24, 31), h.synth_y(0, 300, 1, 31), 5, rng.permutation(300)[:180].reshape(30, 6)),
         ("tiny_m 200x24 M=3", h.synth_x(0, 200, 24, 31), h.synth_y(0, 200, 3, 31), 5, np.stack([rng.permutation(200)[:7] for _ in range(20)])),
         ("micro toy leave-one-out", zs("toyX.csv"), zs("toyY.csv"), 2, np.arange(10)[:, None]),
         ("tiny_m 90x30 M=4", h.synth_x(0, 90, 30, 31), h.synth_y(0, 90, 4, 31), 5, np.stack([rng.permutation(90)[:27] for _ in range(12)]))]
for name, X, Y, A, idx in FOLDS:
    lines.append("folds %s A=%d  %s" % (name, A, digest([h.cv_folds(X, Y, A, idx)])))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
