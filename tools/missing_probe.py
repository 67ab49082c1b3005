#!/usr/bin/env python3
"""Bit-for-bit probe of pls_hip_fit_missing, run by tests/test_gpu_missing.py in a child process on
pls_amd/csrc/testing/libpls_hip.so (PLS_AMD_LIBRARY names it when pls_amd is imported).

For each case named on the command line (tests/test_missing_ref.py: CASES) the SHA-256 of every output of a device-memory
fit on a fresh handle is the baseline; the same call must return the same bits
  again            a second call in a row
  host             from host memory (the pinned staging pipeline)
  poison 0xNN      after pls_hip_test_poison_workspace has filled every scratch workspace of the handle, and every later
                   allocation, with 0xFF / 0x7F
  after fit        after an unrelated pls_hip_fit on the same handle
  after fit_batch  after an unrelated pls_hip_fit_batch on the same handle
One line per comparison, "same" or "DIFFERS", then "done: <cases> cases, <n> differ".  Exit status 1 when anything differs.
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import pls_amd
from pls_amd import _lib as L
from test_missing_ref import CASES, case_data

NAMES = ("W", "P", "Q", "R", "T", "B", "iters")


def poison(h, byte, also_new):
    f = L.lib().pls_hip_test_poison_workspace   # (AttributeError: not the testing build)
    f.restype = ctypes.c_longlong
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    n = int(f(h.h, byte, also_new))
    assert n >= 0, "pls_hip_test_poison_workspace failed"
    return n


def digest(out):
    s = hashlib.sha256()
    for k in NAMES:
        v = out[k]
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        s.update(np.ascontiguousarray(a).tobytes())
    return s.hexdigest()


def dev(a, dt):
    t = pls_amd.colmajor_empty(a.shape[0], a.shape[1], dt, "cuda")
    t.copy_(torch.from_numpy(np.array(a, order="C")).to(dt))
    return t


def main(names):
    torch.cuda.set_device(0)
    bad = 0
    for name in names:
        N, K, M, A, frac, st = CASES[name]
        X, Y, _ = case_data(name)
        dt, ndt = (torch.float32, np.float32) if st == "f32" else (torch.float64, np.float64)
        Xd, Yd = dev(X, dt), dev(Y, dt)
        h = pls_amd.Handle()
        runs = []
        base = digest(h.fit_missing(Xd, Yd, A))
        runs.append(("again", digest(h.fit_missing(Xd, Yd, A))))
        runs.append(("host", digest(h.fit_missing(X.astype(ndt), Y.astype(ndt), A))))
        for byte in (0xFF, 0x7F):
            n = poison(h, byte, 1)
            assert n > 0, "nothing was poisoned"
            runs.append((f"poison 0x{byte:02X} ({n} bytes)", digest(h.fit_missing(Xd, Yd, A))))
        poison(h, 0x01, 0)
        Xo, Yo = h.synth_x(0, 300, 40, 7), h.synth_y(0, 300, 2, 7)
        h.fit_device(Xo, Yo, 3)
        runs.append(("after fit", digest(h.fit_missing(Xd, Yd, A))))
        h.fit_batch(Xo, h.synth_y(0, 300, 6, 9), 2, 3)
        runs.append(("after fit_batch", digest(h.fit_missing(Xd, Yd, A))))
        h.synchronize()
        h.close()
        for what, d in runs:
            same = d == base
            bad += not same
            print(f"{'same' if same else 'DIFFERS'}: {name}: {what}: {d[:16]} / {base[:16]}")
    print(f"done: {len(names)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
