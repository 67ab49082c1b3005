#!/usr/bin/env python3
"""One SHA-256 per case over the output bytes of the missing-value family (missing_kernels.hpp, missing_cv_kernels.hpp,
xdiag_missing_kernels.hpp) and of the column sums of pls_hip_x_diagnostics: run under two builds of the library
(PLS_AMD_LIBRARY), the outputs must be equal line for line.  The cases are the tables of tests/test_missing_ref.py (fit_missing
with one response and with three, scores_missing), tests/test_missing_cv_ref.py (cv_folds_missing) and
tests/test_xdiag_missing_ref.py (x_diagnostics_missing with every output, on the route the library chooses and on the streaming
route, PLS_HIP_XDIAGMISS_ROUTE=stream; x_diagnostics with ssx and sst on the complete data), each in the aligned layout (leading
dimension a multiple of 16 bytes) and with ld = N.
    python tools/missing_bits.py [out.txt]"""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, pls_amd
from test_missing_ref import CASES as FIT_CASES, case_data, case_yardstick
from test_missing_cv_ref import CV_CASES, case_folds
from test_xdiag_missing_ref import CASES as XD_CASES, xd_case

EVERY = ("Q", "T2", "S", "ssx", "sst", "nobs")
LAYOUTS = ("aligned", "ld=N")


def digest(tensors):
    d = hashlib.sha256()
    for t in tensors:
        d.update(np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).tobytes())
    return d.hexdigest()


def dev(a, st, layout="ld=N"):
    """a host matrix as a column-major device view in storage `st`; aligned: ld = the rows rounded up to 16 bytes"""
    dt = torch.float32 if st == "f32" else torch.float64
    N, K = a.shape
    pad = (-N) % (16 // dt.itemsize) if layout == "aligned" else 0
    big = torch.zeros((K, N + pad), dtype=dt, device="cuda")
    big[:, :N] = torch.from_numpy(np.array(a.T, order="C")).to(dt)
    return big.T[:N]


def xdiag_lines(h, route):
    lines = []
    for name, c in XD_CASES.items():
        X, Xc, m = xd_case(name)
        W, P, R = (torch.from_numpy(np.array(m[k])).cuda() for k in "WPR")
        for lay in LAYOUTS:
            out = h.x_diagnostics_missing(dev(X, c[4], lay), W, P, want=EVERY)
            lines.append("x_diagnostics_missing[%s] %s %s  %s" % (route, name, lay, digest(out[k] for k in EVERY)))
            if route == "chosen":
                out = h.x_diagnostics(dev(Xc, c[4], lay), R, P, want=("ssx", "sst"))
                lines.append("x_diagnostics %s %s  %s" % (name, lay, digest(out[k] for k in ("ssx", "sst"))))
    return lines


if os.environ.get("PLS_HIP_XDIAGMISS_ROUTE") == "stream" and "--stream-lines" in sys.argv:  # the child process of the run below
    print("\n".join(xdiag_lines(pls_amd.Handle(), "stream")))
    sys.exit(0)

h = pls_amd.Handle()
lines = []
for name, (N, K, M, A, frac, st) in FIT_CASES.items():
    X, Y, Xc = case_data(name)
    y = case_yardstick(name)
    Y3 = np.column_stack([Y[:, 0], Xc[:, 0] + 0.5 * Y[:, 0], Xc[:, 1] - Y[:, 0]])
    W, P = (torch.from_numpy(np.array(y[k])).cuda() for k in "WP")
    for lay in LAYOUTS:
        Xd = dev(X, st, lay)
        for Yh in (Y[:, :1], Y3):
            out = h.fit_missing(Xd, dev(Yh, st), A)
            lines.append("fit_missing %s M=%d %s  %s" % (name, Yh.shape[1], lay, digest(out[k] for k in ("W", "P", "Q", "R", "T", "B", "iters"))))
        lines.append("scores_missing %s %s  %s" % (name, lay, digest([h.scores_missing(Xd, W, P)])))
for name in CV_CASES:
    N, K, M, A, frac, st = FIT_CASES[name]
    X, Y, _ = case_data(name)
    for lay in LAYOUTS:
        E, iters = h.cv_folds_missing(dev(X, st, lay), dev(Y, st), A, case_folds(name), want_iters=True)
        lines.append("cv_folds_missing %s %s  %s" % (name, lay, digest([E, iters])))
lines += xdiag_lines(h, "chosen")
h.synchronize()
# the streaming route is chosen when the handle is created: a process of its own
r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stream-lines"], env=dict(os.environ, PLS_HIP_XDIAGMISS_ROUTE="stream"),
                   capture_output=True, text=True, timeout=600)
if r.returncode != 0:
    sys.exit("the streaming-route process failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
lines += r.stdout.splitlines()
print("\n".join(lines))
if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
