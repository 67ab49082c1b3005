"""Every entry point with a matrix argument, held to its reference at LONG leading dimensions.

include/pls_hip.h promises "any ld >= N".  Below that promise the routes address groups of columns through 32-bit buffer
descriptors and either check a span limit, fall to an EDGE instantiation, or decline the shape (fit_route.hpp, xb_route.hpp,
the launchers' own checks).  tests/long_ld.py keeps the matrices small and only their columns far apart; two kinds of stress:

  (a) pitch rungs: few columns, 48 ... 520 MiB apart (and 2 GiB for 9 columns), each rung one 16-byte vector more than the round
      figure so that ld is aligned but no power of two.  48 MiB is the control: every fast route is still accepted, offsets are
      already beyond 2^31 bytes.  72 MiB: the xb4 routes and the 32-group tile are past one descriptor.  136 MiB: the 16-group
      tile is.  320 MiB: the 8-group tile is, and 8 ld s lies between 2^31 and 2^32 for the SYRK.  520 MiB: past 2^32 there.
      The single-launch fits decline much earlier (2.46, 4.92, 16 and 64 MiB per column): rungs of their own.
  (b) total offset: thousands of columns at a moderate pitch, chosen so that the LAST column begins beyond 2^31 ELEMENTS
      (17.2 GB in fp64, 8.6 GB in fp32): the split X * B routes, the short-tile and row-pack plans, the K-split row sweep of the
      missing-value plans, ALGO_DUAL.

Each case asserts: the result against the CPU yardstick the entry point's own GPU test uses, at that test's bar (imported where
it has a name); the same call on compact copies on the same handle within that bar (not bit-equal: the header allows bits to
depend on ld); the arena's checks (inputs bit-identical, exactly the outputs' cells written); and the route, where the
handle's launch counts tell it apart.  tests/test_long_ld_cover.py recomputes, on the CPU, the side of every guard a case here
claims to cross.  test_zz_record prints the table of what ran.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import handle_with_env
from test_gpu_bounds import CV_BAR, DEFLATE_BAR_F64, SSE_BAR, XTY_BAR, Z_BAR, _sse_reference, _tols, xb_bar
from test_gpu_parity import _fold_reference, check_against, oracle_ref

pytestmark = pytest.mark.gpu

MiB = 1 << 20
ES = {"f64": 8, "f32": 4}
ARENA_BYTES = 257 * (72 * MiB + 16) + MiB          # the largest case: 257 columns 72 MiB apart (18.07 GiB)
GEN = dict(PLS_HIP_RESIDENT=0, PLS_HIP_TINY=0)     # a handle whose fits take the general plans
KERNEL, NIPALS, GRAM, AUTO, DUAL = 0, 1, 2, 3, 4
RECORD = []                                        # (entry point, case, dt, N, K, ld, guards, route observed, error / bar, seconds)


def case_ld(pitch, dt, cols):
    """leading dimension in elements: `pitch` MiB plus one 16-byte vector; "total": the smallest aligned one at which column
    cols - 1 begins beyond 2^31 elements"""
    es = ES[dt]
    if pitch == "total":
        V = 16 // es
        ld = -(-((1 << 31) + 1) // (cols - 1))      # (cols - 1) ld > 2^31
        return -(-ld // V) * V
    return (int(pitch * MiB) + 16) // es


# ---- the cases (plain data: tests/test_long_ld_cover.py reads them without a GPU) -------------------------------------------------
def F(name, N, K, M, A, dt, pitch, long, env=GEN, route=None, guards=None, method=0, **opts):
    return dict(name=name, N=N, K=K, M=M, A=A, dt=dt, pitch=pitch, long=long, env=env, route=route, guards=guards or {},
                method=method, opts=opts)


ONE, WAVE_ = "fused-one-descriptor", "fused-per-wave"
FIT = [
    # 48 MiB, the control: one descriptor for the 32 groups
    F("kernel-48", 5000, 257, 1, 6, "f64", 48, "X", route="fused", guards={ONE: "below"}),
    F("nipals-48-all", 5000, 257, 2, 6, "f32", 48, "XYT", route="fused", guards={ONE: "below"}, ALGO=NIPALS),
    F("defer2-48", 5000, 257, 1, 6, "f64", 48, "XT", route="fused", guards={ONE: "below", "defer": "below"}, ALGO=NIPALS, DEFER=2),
    # 72 MiB: the 32 groups past one descriptor -- a descriptor per wave (EDGE 1), still one sweep per component
    F("kernel-72", 5000, 257, 1, 6, "f64", 72, "X", route="fused", guards={ONE: "past", WAVE_: "below"}),
    F("nipals-72", 5000, 257, 1, 6, "f64", 72, "X", route="fused", guards={ONE: "past", WAVE_: "below"}, ALGO=NIPALS),
    F("kernel-72-f32", 5000, 257, 1, 6, "f32", 72, "X", route="fused", guards={ONE: "past"}),
    F("nipals-72-all-f32", 5000, 257, 2, 6, "f32", 72, "XYT", route="fused", guards={ONE: "past"}, ALGO=NIPALS),
    F("kernel-72-y", 5000, 257, 2, 6, "f64", 72, "Y", route="fused"),
    F("nipals-72-t", 5000, 257, 1, 6, "f64", 72, "T", route="fused", ALGO=NIPALS),
    F("kernel-72-all", 5000, 257, 3, 6, "f64", 72, "XYT", route="fused", guards={ONE: "past"}),
    F("nipals-72-nofuse", 5000, 257, 1, 4, "f64", 72, "XYT", route="unfused", ALGO=NIPALS, FUSE=0),
    F("nipals-72-defer2", 5000, 257, 1, 6, "f64", 72, "XT", route="fused", guards={ONE: "past", "defer": "past"}, ALGO=NIPALS, DEFER=2),
    F("nipals-72-layout0", 5000, 257, 2, 5, "f64", 72, "X", route="fused", guards={ONE: "past"}, ALGO=NIPALS, WORK_LAYOUT=0),
    # the 16-group tile (128 < K <= 256): 128 MiB
    F("nipals-120", 5000, 129, 1, 6, "f64", 120, "X", route="fused", guards={ONE: "below"}, ALGO=NIPALS),
    F("kernel-136", 5000, 129, 1, 6, "f64", 136, "X", route="fused", guards={ONE: "past", WAVE_: "below"}),
    F("nipals-136-all-f32", 5000, 129, 2, 6, "f32", 136, "XYT", route="fused", guards={ONE: "past"}, ALGO=NIPALS),
    # the 8-group tile (K <= 128): 256 MiB
    F("nipals-160", 5000, 100, 1, 6, "f64", 160, "X", route="fused", guards={ONE: "below"}, ALGO=NIPALS),
    F("kernel-160-all-f32", 5000, 100, 2, 6, "f32", 160, "XYT", route="fused", guards={ONE: "below"}),
    F("kernel-320", 5000, 40, 1, 6, "f64", 320, "X", route="fused", guards={ONE: "past", WAVE_: "below"}),
    F("nipals-320-all", 5000, 40, 2, 6, "f64", 320, "XYT", route="fused", guards={ONE: "past"}, ALGO=NIPALS),
    F("nipals-320-f32", 5000, 40, 1, 6, "f32", 320, "X", route="fused", guards={ONE: "past"}, ALGO=NIPALS),
    F("auto-320", 5000, 40, 1, 6, "f64", 320, "X", route="fused", guards={ONE: "past"}, ALGO=AUTO),
    # X^T X: 8 ld s between 2^31 and 2^32 (the SYRK's int casts), then past 2^32 (its LDS-DMA form declines)
    F("gram-320", 5000, 40, 2, 6, "f64", 320, "XYT", route="gram", guards={"syrk-signed": "past", "syrk-dma": "below"}, ALGO=GRAM),
    F("gram-320-f32", 5000, 40, 1, 6, "f32", 320, "XY", route="gram", guards={"syrk-signed": "past", "syrk-dma": "below"}, ALGO=GRAM),
    F("type2-320", 5000, 40, 2, 6, "f64", 320, "XY", route="type2", guards={"syrk-signed": "past", "syrk-dma": "below"}, method=1),
    F("gram-48", 5000, 257, 1, 6, "f64", 48, "XY", route="gram", guards={"syrk-signed": "below"}, ALGO=GRAM),
    F("gram-520", 5000, 33, 2, 6, "f64", 520, "XYT", route="gram", guards={"syrk-dma": "past"}, ALGO=GRAM),
    F("gram-520-f32", 5000, 33, 1, 6, "f32", 520, "X", route="gram", guards={"syrk-dma": "past"}, ALGO=GRAM),
    F("gram-520-y", 5000, 33, 2, 6, "f64", 520, "Y", route="gram", ALGO=GRAM),
    F("type2-520-f32", 5000, 33, 2, 6, "f32", 520, "XY", route="type2", guards={"syrk-dma": "past"}, method=1),
    F("kernel-520", 5000, 33, 1, 6, "f64", 520, "X", route="fused", guards={ONE: "past", WAVE_: "below"}),
    F("nipals-520-f32", 5000, 33, 2, 6, "f32", 520, "XYT", route="fused", guards={ONE: "past"}, ALGO=NIPALS),
    F("kernel-520-nofuse", 5000, 33, 1, 5, "f64", 520, "XT", route="unfused", FUSE=0),
    F("nipals-520-layout0", 5000, 33, 1, 5, "f64", 520, "X", route="fused", guards={ONE: "past"}, ALGO=NIPALS, WORK_LAYOUT=0),
    # 2 GiB: even one group per wave is past a descriptor -- "not addressable", the one-product kernels take the fit
    F("kernel-2g", 5000, 9, 1, 5, "f64", 2048, "X", route="unfused", guards={WAVE_: "past"}),
    F("nipals-2g", 5000, 9, 2, 5, "f64", 2048, "XYT", route="unfused", guards={WAVE_: "past"}, ALGO=NIPALS),
    F("kernel-2g-f32", 5000, 9, 1, 5, "f32", 2048, "X", route="unfused", guards={WAVE_: "past"}),
    F("gram-2g", 5000, 9, 1, 4, "f64", 2048, "X", route="gram", guards={"syrk-dma": "past"}, ALGO=GRAM),
    # the single-launch fits (a default handle): each declines at its own span limit and the next route takes the fit
    F("tiny-2", 130, 100, 1, 7, "f64", 2, "XYT", env={}, route="single", guards={"tiny": "below"}),
    F("tiny-3", 130, 100, 1, 7, "f64", 3, "X", env={}, route="single", guards={"tiny": "past", "resident": "below"}),   # (the resident fit, one workgroup)
    F("tiny-48", 130, 100, 1, 7, "f64", 48, "X", env={}, route="general", guards={"tiny": "past", "resident": "past"}),
    F("tiny-2-f32", 1000, 20, 1, 6, "f32", 2, "XYT", env={}, route="single", guards={"tiny": "below"}),
    F("tiny-m3-2", 130, 100, 3, 7, "f64", 2, "XYT", env={}, route="single", guards={"tiny": "below"}),
    F("tiny-m3-48", 130, 100, 3, 7, "f64", 48, "XYT", env={}, route="general", guards={"tiny": "past", "resident": "past"}),
    F("resident-4", 5000, 128, 1, 10, "f64", 4, "XYT", env={}, route="single", guards={"tiny": "past", "resident": "below"}),
    F("resident-5", 5000, 128, 1, 10, "f64", 5, "X", env={}, route="general", guards={"resident": "past"}),
    F("resident-m5-4-f32", 3001, 77, 5, 7, "f32", 4, "XYT", env={}, route="single", guards={"resident": "below"}),
    F("resident-m5-5-f32", 3001, 77, 5, 7, "f32", 5, "X", env={}, route="general", guards={"resident": "past"}),
    F("resident-ldt-160", 5000, 128, 1, 10, "f64", 160, "T", env={}, route="single", guards={"single-ldt": "below"}),
    F("resident-ldt-320", 5000, 128, 1, 10, "f64", 320, "T", env={}, route="general", guards={"single-ldt": "past"}),
    F("resident-m5-ldt-320", 3001, 77, 5, 7, "f64", 320, "YT", env={}, route="single"),   # (2..8 responses: plain stores, no limit)
    F("rgram-15", 5003, 128, 1, 11, "f64", 15, "XYT", env={}, route="single", guards={"resident-gram": "below", "resident": "past"}, ALGO=AUTO),
    F("rgram-17", 5003, 128, 1, 11, "f64", 17, "X", env={}, route="general", guards={"resident-gram": "past"}, ALGO=AUTO),
    F("rgram-m2-15-f32", 2000, 120, 2, 6, "f32", 15, "XYT", env={}, route="single", guards={"resident-gram": "below"}, ALGO=AUTO),
    F("micro-48", 60, 24, 4, 6, "f64", 48, "XYT", env={}, route="single", guards={"micro": "below", "tiny": "past", "resident": "past"}),
    F("micro-72", 60, 24, 4, 6, "f64", 72, "XYT", env={}, route="general", guards={"micro": "past"}),
    F("micro-48-f32", 64, 32, 1, 5, "f32", 48, "X", env={}, route="single", guards={"micro": "below"}),
    # (b) the last column beyond 2^31 elements
    F("short-total", 516, 2050, 2, 5, "f64", "total", "X", route="short", guards={"total": "past"}, ALGO=NIPALS),
    F("short-total-kernel", 516, 2050, 1, 4, "f64", "total", "X", route="short", guards={"total": "past"}),
    F("short-total-all-f32", 1031, 2500, 2, 4, "f32", "total", "XYT", route="short", guards={"total": "past"}, ALGO=NIPALS),
    F("rowpack-total", 261, 5000, 1, 4, "f64", "total", "X", route="rowpack", guards={"total": "past"}, ALGO=NIPALS),
    F("rowpack-total-kernel-f32", 263, 6000, 2, 4, "f32", "total", "X", route="rowpack", guards={"total": "past"}),
    F("half-total", 1030, 700, 2, 5, "f64", "total", "X", route="fused", guards={"total": "past", ONE: "below"}, ALGO=NIPALS),
    F("gram-total", 4096, 700, 1, 5, "f64", "total", "X", route="gram", guards={"total": "past"}, ALGO=GRAM),
    F("type2-total-f32", 600, 2050, 2, 4, "f32", "total", "XY", route="type2", guards={"total": "past"}, method=1),
    F("dual-total", 97, 1500, 1, 12, "f64", "total", "XYT", env={}, route="dual", guards={"total": "past"}, ALGO=DUAL),
    F("dual-total-f32", 2049, 3001, 4, 6, "f32", "total", "XYT", env={}, route="dual", guards={"total": "past"}, ALGO=DUAL),
    F("dual-320", 37, 40, 2, 5, "f64", 320, "XYT", env={}, route="dual", ALGO=DUAL),
    F("dual-72-f32", 200, 257, 1, 6, "f32", 72, "X", env={}, route="dual", ALGO=DUAL),
]

# X * Bm: (N, K) by storage type so that the 4 x 4 x 4 matrix-core routes take 9 and 20 columns at 48 MiB (32 MiB of X, a tile per CU)
XB_TALL = {"f64": (16400, 257), "f32": (32704, 257)}


def XB(N, K, C, dt, pitch, long, guards=None):
    return dict(name=f"{N}x{K}-c{C}-{dt}-{pitch}-{long}", N=N, K=K, C=C, dt=dt, pitch=pitch, long=long, guards=guards or {}, A=C)


XB_CASES = (
    [XB(*XB_TALL[dt], C, dt, 48, "Xo", {"xb4": "below"}) for dt in ES for C in (9, 20)] +
    [XB(*XB_TALL[dt], C, dt, 72, "X", {"xb4": "past"}) for dt in ES for C in (1, 3, 9, 20, 33)] +
    [XB(*XB_TALL[dt], C, dt, 72, "o", {"xb4": "past"}) for dt in ES for C in (3, 20)] +
    [XB(*XB_TALL[dt], C, dt, 72, "Xo", {"xb4": "past"}) for dt in ES for C in (9, 33)] +
    [XB(5000, 40, 3, "f64", 320, "Xo"), XB(5000, 40, 20, "f32", 320, "Xo"), XB(4099, 33, 9, "f64", 520, "X"), XB(4099, 33, 1, "f32", 520, "o"),
     XB(1301, 9, 3, "f64", 2048, "X")] +
    # (b): xb_split (1, 3 columns) and the column-split matrix-core form (9, 20; 33 = 32 + 1) of a short, wide matrix
    [XB(2000, 5000, C, "f64", "total", "X", {"total": "past"}) for C in (1, 3, 9, 20, 33)] +
    [XB(2100, 5000, C, "f32", "total", "X", {"total": "past"}) for C in (3, 9, 20)]
)

# (N, K, M, dt, pitch, long)
XTY_CASES = [(5000, 257, 1, "f64", 72, "X"), (5000, 257, 9, "f32", 72, "XY"), (5000, 129, 4, "f64", 136, "XY"), (5000, 40, 8, "f64", 320, "XY"),
             (5000, 40, 2, "f32", 320, "X"), (5000, 33, 2, "f32", 520, "Y"), (5000, 33, 4, "f64", 520, "XY"), (4099, 9, 3, "f64", 2048, "XY"),
             (1001, 2050, 3, "f64", "total", "X"), (1001, 2050, 1, "f32", "total", "XY")]
# (N, K, dt, pitch, mode): which of src / dst is long; "inplace": dst == src, long
DEFLATE_CASES = [(5000, 257, "f64", 72, "both"), (5000, 257, "f32", 72, "inplace"), (4099, 40, "f32", 320, "src"), (4099, 40, "f64", 320, "inplace"),
                 (4099, 33, "f64", 520, "dst"), (4099, 33, "f32", 520, "both"), (1001, 9, "f64", 2048, "both"),
                 (1001, 2050, "f64", "total", "inplace"), (1001, 2050, "f32", "total", "both")]
ZSCORE_CASES = [(5000, 257, "f64", 72, "both"), (5000, 257, "f32", 72, "src"), (4099, 40, "f32", 320, "inplace"), (4099, 40, "f64", 320, "dst"),
                (4099, 33, "f64", 520, "inplace"), (4099, 33, "f32", 520, "both"), (1001, 9, "f64", 2048, "both"),
                (1001, 2050, "f64", "total", "both"), (1001, 2050, "f32", "total", "inplace")]
# (N, A, M, dt, pitch, long): S is N x A
SSE_CASES = [(2000, 257, 2, "f32", 72, "S"), (2000, 40, 3, "f64", 320, "SY"), (2000, 33, 2, "f32", 520, "SY"), (2000, 33, 1, "f64", 520, "Y"),
             (1001, 2050, 2, "f64", "total", "S"), (1001, 2050, 2, "f32", "total", "SY")]
# (N, K, M, A, dt, pitch, long)
MODEL_SSE_CASES = [(3001, 40, 3, 12, "f64", 320, "XY"), (3001, 33, 2, 5, "f32", 520, "XY"), (3001, 257, 1, 8, "f64", 72, "X"),
                   (1001, 2050, 2, 6, "f64", "total", "X"), (1001, 2050, 1, 5, "f32", "total", "XY")]
# (N, K, A, dt, pitch, long): Q, T, S = the outputs Qres, T2, S
XDIAG_CASES = [(3000, 40, 8, "f64", 320, "XQTS"), (3000, 257, 8, "f64", 72, "X"), (3000, 257, 8, "f32", 72, "XS"), (3000, 33, 6, "f32", 520, "QT"),
               (3000, 33, 6, "f64", 520, "QTS"), (300, 2050, 8, "f64", "total", "X"), (300, 2050, 8, "f32", "total", "XS")]
# (which, row0, n, cols, dt, pitch)
SYNTH_CASES = [("x", 777, 1001, 257, "f64", 72), ("x", 5, 4099, 33, "f32", 520), ("y", 1000, 3001, 9, "f64", 2048), ("y", 64, 515, 40, "f32", 320),
               ("x", 3, 301, 2050, "f64", "total"), ("x", 12345, 301, 2050, "f32", "total")]
# (route, N, K, M, A, ts, nf, dt, pitch, long)
CV_CASES = [("batched", 1500, 40, 2, 4, 25, 9, "f64", 320, "XY"), ("batched", 400, 40, 2, 4, 25, 9, "f32", 320, "XY"),
            ("batched", 1500, 257, 1, 4, 25, 9, "f64", 72, "X"), ("refit", 301, 33, 2, 4, 17, 5, "f64", 520, "XY"),
            ("refit", 301, 33, 2, 4, 17, 5, "f32", 520, "X"), ("batched", 600, 2050, 1, 3, 20, 5, "f64", "total", "X")]
CV_DUAL_CASES = [("97x1500", "total", "XY"), ("2049x3001-f32", "total", "XY"), ("nir-25x18", 40, "XY")]
# fit_batch: (route, N, K, M, A, nprob, dt, pitch, long).  "batched": the shared X^T X; the per-problem route (one KERNEL_TYPE2 fit per
# problem, Y_b = Ys + b M ldy: plan_batch.hpp, fit_batch_refit) by its switch ("refit") or by more than 32 responses ("m40")
BATCH_CASES = [("batched", 1000, 7, 2, 3, 5, "f64", 2048, "XY"), ("batched", 1000, 7, 2, 3, 5, "f32", 2048, "X"),
               ("batched", 2048, 128, 4, 6, 17, "f64", 136, "XY"), ("batched", 1000, 64, 1, 10, 37, "f32", 160, "XY"),
               ("batched", 300, 2050, 1, 3, 2, "f64", "total", "X"), ("batched", 300, 20, 1, 3, 2050, "f64", "total", "Y"),
               ("refit", 1000, 7, 2, 3, 5, "f64", 2048, "XY"), ("refit", 1000, 7, 2, 3, 5, "f32", 2048, "Y"),
               ("refit", 2048, 128, 4, 6, 17, "f64", 136, "X"), ("refit", 1000, 64, 1, 10, 37, "f32", 160, "Y"),
               ("m40", 1000, 64, 40, 5, 3, "f64", 136, "XY"), ("m40", 1000, 64, 40, 5, 3, "f32", 136, "Y"),
               # the last column of Ys (2080 of them) beyond 2^31 elements
               ("m40", 300, 20, 40, 3, 52, "f64", "total", "Y"), ("m40", 300, 20, 40, 3, 52, "f32", "total", "XY"),
               ("refit", 300, 20, 1, 3, 2050, "f32", "total", "Y")]
BATCH_DUAL_CASES = [("97x1500", "total", "XY"), ("1031x3000-f32", "total", "XY"), ("17x1003", "total", "X")]
RESAMPLE_CASES = [("5000x64", 160, "XYW", False), ("5000x64", 160, "W", False), ("97x1500", "total", "XYW", False), ("97x1500", "total", "XYW", True), ("1031x3000-f32", "total", "XY", True),
                  ("17x1003", "total", "X", True)]
CVBATCH_CASES = [("97x1500", "total", "XY", True), ("1031x3000-f32", "total", "XY", True), ("97x1500", "total", "X", False),
                 ("17x1003", 16, "XY", True)]
# the missing-value entry points: (case of test_missing_ref, pitch, long)
MISSING_FIT_CASES = [("5000x40", 320, "XYT"), ("1031x130-f32", 136, "XYT"), ("257x33-m3", 520, "XY"), ("40x300-m2", 48, "XT"),
                     ("33x20011", "total", "X"), ("97x1003-m3", "total", "XYT")]
MISSING_SCORES_CASES = [("130x70", 160, "XS"), ("1031x130-f32", 136, "XS"), ("257x33-m3", 520, "S"), ("33x20011", "total", "X")]
MISSING_Z_CASES = [("5000x40", 320, "both"), ("1031x130-f32", 136, "inplace"), ("67x19", 520, "src"), ("33x20011", "total", "both")]
MISSING_CV_CASES = [("5000x40", 320, "XY"), ("1031x130-f32", 136, "XY"), ("257x33-m3", 520, "X"), ("33x20011", "total", "X")]


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _tdt(dt):
    torch = _torch()
    return torch.float64 if dt == "f64" else torch.float32


def _code(dt):
    from pls_amd import _lib as L
    return L.F64 if dt == "f64" else L.F32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ldv(t):
    from pls_amd.model import _ld
    return _ld(t)


def _round(a, dt):
    """the fp64 image of a in its storage type"""
    a = np.asarray(a, dtype=np.float64)
    return np.asfortranarray(a.astype(np.float32).astype(np.float64) if dt == "f32" else a)


@pytest.fixture(scope="module")
def arena():
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    from long_ld import Arena
    a = Arena(ARENA_BYTES)
    yield a
    a.release()


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    """a device left in error by an earlier case ends the session here, before anything more is launched on it"""
    torch = _torch()
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:   # (the sticky error of a fault)
            pytest.exit(f"the device is in error, nothing more is run on it: {e}", returncode=3)
    yield


class Lay:
    """the matrices of one call: those named in `long` inside the arena at leading dimension ld, one row window each (so that they
    interleave: the memory of the widest alone), the others compact.  long = "": the compact twin of the call."""

    def __init__(self, arena, dt, ld, long, fill="nan"):
        self.arena, self.dt, self.tdt, self.ld, self.long = arena, dt, _tdt(dt), ld, set(long)
        self.V = 16 // ES[dt]
        self.pos = 16 * self.V
        if self.long:
            arena.begin(self.tdt, fill)

    def _window(self, rows):
        off = self.pos
        self.pos += -(-(rows + 40) // self.V) * self.V
        assert self.pos <= self.ld, "the row windows do not fit the pitch"
        return off

    def inp(self, name, a, inout=False, dtype=None):
        import pls_amd
        torch = _torch()
        if name in self.long:
            assert dtype is None or dtype == self.tdt
            return self.arena.place(a, self.tdt, self.ld, self._window(a.shape[0]), inout=inout)
        t = pls_amd.colmajor_empty(a.shape[0], a.shape[1], dtype or self.tdt, "cuda")
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype or self.tdt))
        return t

    def out(self, name, rows, cols, dtype=None):
        import pls_amd
        if name in self.long:
            assert dtype is None or dtype == self.tdt
            return self.arena.out(rows, cols, self.tdt, self.ld, self._window(rows))
        t = pls_amd.colmajor_empty(rows, cols, dtype or self.tdt, "cuda")
        t.fill_(float("nan"))
        return t

    def check(self):
        if self.long:
            self.arena.check()


def _both(arena, dt, ld, long, call, fill="nan"):
    """the call on the long layout (arena checked), then on compact copies"""
    lay = Lay(arena, dt, ld, long, fill)
    got = call(lay)
    lay.check()
    return got, call(Lay(arena, dt, ld, "", fill))


def _launches(h, fn):
    """fn() and the launches it made, by family (OPT_PROFILE = 2: the `small` family -- the single-launch fits -- is counted too)"""
    import pls_amd
    h.set_option(pls_amd.OPT_PROFILE, 2)
    h.timing()
    out = fn()
    h.synchronize()
    lau = h.timing()["launches"]
    h.set_option(pls_amd.OPT_PROFILE, 0)
    return out, lau


def _record(entry, case, dt, N, K, ld, guards, route, err, t0):
    RECORD.append((entry, case, dt, N, K, ld, ", ".join(f"{g} {s}" for g, s in guards.items()) or "-", route, err, time.time() - t0))


def _set_opts(h, opts):
    import pls_amd
    for k, v in opts.items():
        h.set_option(getattr(pls_amd, "OPT_" + k), v)


_REFS = {}


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ---- pls_hip_fit --------------------------------------------------------------------------------------------------------------------
def _route_check(route, lau, A, what):
    total = sum(lau.values())
    if route == "fused":        # one sweep per component on the caller's matrix (test_gpu_edge.py)
        assert lau["fused"] == A and lau["xb"] == 0, (what, lau)
    elif route == "unfused":    # the one-product kernels
        assert lau["fused"] == 0 and total > 1, (what, lau)
    elif route == "short":      # one copy into short tiles in the X^T Y sweep + A fused passes (test_gpu_edge.py)
        assert lau["fused"] == A and lau["deflate"] == 1 and lau["xty"] == 0, (what, lau)
    elif route == "rowpack":
        assert lau["fused"] == A and lau["deflate"] == 1, (what, lau)
    elif route == "gram":       # test_gpu_hard_data._launch_check
        assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] <= 1, (what, lau)
    elif route in ("type2", "dual"):
        assert lau["fused"] == 0 and lau["deflate"] == 0 and lau["xb"] == 0 and lau["xty"] >= 1, (what, lau)
    elif route == "single":
        assert total == 1 and lau["small"] == 1, (what, lau)
    elif route == "general":    # a single-launch shape past its span limit: the general plan's one sweep per component (with the
        assert total > 1 and lau["fused"] == A, (what, lau)   # profile at 2 its update kernels count as `small` too)
    else:
        assert route is None, route


def _fit_bars(c):
    if c["opts"].get("ALGO") == DUAL and c["dt"] == "f32":   # test_gpu_dual.py: the bars of test_wide_matrix_fp32
        return dict(tol_b=2e-5, tol_col=2e-5, tol_inv=1e-4)
    return _tols(c["dt"])                                   # test_gpu_bounds.py: every route of pls_hip_fit


@pytest.mark.parametrize("c", FIT, ids=[c["name"] for c in FIT])
def test_fit(arena, oracle, po, c):
    import pls_amd
    t0 = time.time()
    torch = _torch()
    N, K, M, A, dt = c["N"], c["K"], c["M"], c["A"], c["dt"]
    ld = case_ld(c["pitch"], dt, K)
    Xh, Yh = _round(oracle.synth_x(0, N, K), dt), _round(oracle.synth_y(0, N, M), dt)
    type2 = c["method"] == 1
    tols = _fit_bars(c)

    def call(h, lay):
        X, Y = lay.inp("X", Xh), lay.inp("Y", Yh)
        out = {k: pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K) for k in "WPR"}
        out["Q"] = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M)
        out["B"] = pls_amd.colmajor_empty(K, M, torch.float64, "cuda", ld=K)
        out["T"] = None if type2 else lay.out("T", N, A)
        _, lau = _launches(h, lambda: h.fit_device(X, Y, A, method=c["method"], out=out))
        return out, lau

    with handle_with_env(**c["env"]) as h:
        _set_opts(h, c["opts"])
        (got, lau), (twin, _) = _both(arena, dt, ld, c["long"], lambda lay: call(h, lay))
    _route_check(c["route"], lau, A, c["name"])
    if type2:   # test_gpu_parity.test_kernel_type2 / test_kernel_type2_fp32_storage: B alone
        Bref = _cached(("t2", N, K, M, A, dt), lambda: (lambda r: oracle.coefficients(r["R"], r["Q"]))(oracle.plsr(Xh, Yh, A, method=1)))
        err = po.rel_fro(got["B"].cpu().numpy(), Bref)
        assert err < tols["tol_b"], err
        assert po.rel_fro(got["B"].cpu().numpy(), twin["B"].cpu().numpy()) < tols["tol_b"]
    else:
        ref, Bref, cerr = _cached(("fit", N, K, M, A, dt), lambda: oracle_ref(oracle, po, Xh, Yh, A))
        check_against(po, got, ref, Bref, ref["T"], col_err=cerr, **tols)
        # the compact twin on the same handle, at the same bars
        tw = {k: twin[k].cpu().numpy().astype(np.float64) for k in "WPQRTB"}
        check_against(po, got, tw, tw["B"], tw["T"], col_err=cerr, **tols)
        err = po.rel_fro(got["B"].cpu().numpy(), Bref)
    _record("fit", c["name"], dt, N, K, ld, c["guards"], f"{c['route']}: {dict(lau)}", f"B {err:.1e} / {tols['tol_b']:.0e}", t0)


# ---- pls_hip_xb ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XB_CASES, ids=[c["name"] for c in XB_CASES])
def test_xb(arena, oracle, c):
    from pls_amd import _lib as L
    import pls_amd
    t0 = time.time()
    torch = _torch()
    N, K, C, dt = c["N"], c["K"], c["C"], c["dt"]
    ld = case_ld(c["pitch"], dt, K)
    Xh = _cached(("xbx", N, K, dt), lambda: _round(oracle.synth_x(0, N, K), dt))
    Bh = np.asfortranarray(np.random.default_rng(N + K + C).standard_normal((K, C)))
    Bd = pls_amd.colmajor_empty(K, C, torch.float64, "cuda", ld=K); Bd.copy_(torch.from_numpy(Bh))

    def call(h, lay):
        X = lay.inp("X", Xh)
        out = lay.out("o", N, C)
        _, lau = _launches(h, lambda: L.check(L.lib().pls_hip_xb(h.h, _ptr(X), _ldv(X), N, K, _ptr(Bd), K, C, _code(dt), L.MEM_DEVICE,
                                                                   _ptr(out), _ldv(out)), h.h))
        return out.cpu().numpy().astype(np.float64), lau

    with handle_with_env() as h:
        (got, lau), (twin, _) = _both(arena, dt, ld, c["long"], lambda lay: call(h, lay))
    ref = Xh @ Bh
    bar = xb_bar(dt, K)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert np.isfinite(got).all() and err < bar, err
    assert np.linalg.norm(got - twin) / np.linalg.norm(ref) < bar
    assert lau["xb"] >= 1 and lau["fused"] == 0, lau
    _record("xb", c["name"], dt, N, K, ld, c["guards"], f"not observable (family xb: {lau['xb']} launches)", f"{err:.1e} / {bar:.1e}", t0)


# ---- pls_hip_xty --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,dt,pitch,long", XTY_CASES)
def test_xty(arena, N, K, M, dt, pitch, long):
    t0 = time.time()
    ld = case_ld(pitch, dt, K)
    rng = np.random.default_rng(N * M + K)
    Xh, Yh = _round(rng.standard_normal((N, K)), dt), _round(rng.standard_normal((N, M)), dt)

    def call(h, lay):
        out = h.xty(lay.inp("X", Xh), lay.inp("Y", Yh)); h.synchronize()
        return out.cpu().numpy()

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    ref, scale = Xh.T @ Yh, np.abs(Xh).T @ np.abs(Yh)
    assert (np.abs(got - ref) <= XTY_BAR * scale).all()
    assert (np.abs(got - twin) <= XTY_BAR * scale).all()
    _record("xty", f"m{M}-{long}", dt, N, K, ld, {}, "not observable", f"{(np.abs(got - ref) / scale).max():.1e} / 1e-13 of |X|^T|Y|", t0)


# ---- pls_hip_deflate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,dt,pitch,mode", DEFLATE_CASES)
def test_deflate(arena, N, K, dt, pitch, mode):
    t0 = time.time()
    torch = _torch()
    ld = case_ld(pitch, dt, K)
    rng = np.random.default_rng(N + K)
    Sh, th, ph = _round(rng.standard_normal((N, K)), dt), _round(rng.standard_normal((N, 1)), dt)[:, 0], rng.standard_normal(K)
    t = torch.from_numpy(th).to(_tdt(dt)).cuda(); p = torch.from_numpy(ph).cuda()
    long = {"src": "s", "dst": "d", "both": "sd", "inplace": "s"}[mode]

    def call(h, lay):
        src = lay.inp("s", Sh, inout=mode == "inplace")
        dst = src if mode == "inplace" else lay.out("d", N, K)
        h.deflate(src, t, p, dst=dst); h.synchronize()
        return dst.cpu().numpy().astype(np.float64)

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    outer = np.outer(th, ph)
    ref = Sh - outer
    for g in (got, twin):   # test_gpu_bounds.test_deflate_writes_exactly_dst
        if dt == "f64":
            assert (np.abs(g - ref) <= DEFLATE_BAR_F64 * (np.abs(Sh) + np.abs(outer))).all()
        else:
            r32 = ref.astype(np.float32)
            assert (np.abs(g - r32) <= np.spacing(np.abs(r32))).all()
    _record("deflate", mode, dt, N, K, ld, {}, "not observable", "every cell within 1e-15 (|s| + |t p|) / 1 ulp of fp32", t0)


# ---- pls_hip_colwise_z_scores ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,dt,pitch,mode", ZSCORE_CASES)
def test_colwise_z_scores(arena, oracle, N, K, dt, pitch, mode):
    from pls_amd import _lib as L
    t0 = time.time()
    torch = _torch()
    ld = case_ld(pitch, dt, K)
    rng = np.random.default_rng(N * 7 + K)
    Xh = _round(oracle.synth_x(0, N, K) * rng.uniform(0.1, 30, K) + rng.uniform(-50, 50, K), dt)
    long = {"src": "s", "dst": "d", "both": "sd", "inplace": "s"}[mode]

    def call(h, lay):
        X = lay.inp("s", Xh, inout=mode == "inplace")
        Z = X if mode == "inplace" else lay.out("d", N, K)
        mean = torch.empty(K, dtype=torch.float64, device="cuda"); sd = torch.empty(K, dtype=torch.float64, device="cuda")
        L.check(L.lib().pls_hip_colwise_z_scores(h.h, _ptr(X), _ldv(X), N, N, K, _code(dt), _ptr(Z), _ldv(Z), _ptr(mean), _ptr(sd)), h.h)
        h.synchronize()
        return Z.cpu().numpy().astype(np.float64), mean.cpu().numpy(), sd.cpu().numpy()

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    xl = Xh.astype(np.longdouble)
    mr = xl.mean(0); sr = np.sqrt(((xl - mr) ** 2).sum(0) / (N - 1))
    zr = ((xl - mr) / sr).astype(np.float64)
    zbar = Z_BAR[dt]
    for Z, mean, sd in (got, twin):
        assert np.allclose(mean, mr.astype(np.float64), rtol=1e-13, atol=1e-13)
        assert np.allclose(sd, sr.astype(np.float64), rtol=1e-12)
        assert np.abs(Z - zr).max() < zbar
    _record("colwise_z_scores", mode, dt, N, K, ld, {}, "not observable", f"Z {np.abs(got[0] - zr).max():.1e} / {zbar:.0e}", t0)


# ---- pls_hip_sse_by_components, pls_hip_model_sse -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A,M,dt,pitch,long", SSE_CASES)
def test_sse_by_components(arena, N, A, M, dt, pitch, long):
    t0 = time.time()
    torch = _torch()
    ld = case_ld(pitch, dt, A)
    rng = np.random.default_rng(A + M)
    Sh, Yh = _round(rng.standard_normal((N, A)) / np.sqrt(A), dt), _round(rng.standard_normal((N, M)), dt)
    Qh = rng.standard_normal((M, A))
    Q = torch.from_numpy(Qh).cuda()

    def call(h, lay):
        out = h.sse_by_components(lay.inp("S", Sh), lay.inp("Y", Yh), Q); h.synchronize()
        return out.cpu().numpy()

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    ref = _sse_reference(Sh, Yh, Qh)
    bar = SSE_BAR * np.abs(ref).max()
    assert np.abs(got - ref).max() < bar and np.abs(got - twin).max() < bar
    _record("sse_by_components", f"m{M}-{long}", dt, N, A, ld, {}, "not observable", f"{np.abs(got - ref).max() / np.abs(ref).max():.1e} / 1e-10", t0)


@pytest.mark.parametrize("N,K,M,A,dt,pitch,long", MODEL_SSE_CASES)
def test_model_sse(arena, oracle, N, K, M, A, dt, pitch, long):
    """fp64: the bar of test_gpu_bounds.test_model_sse_writes_exactly_sse.  fp32 storage has no test of its own there: the scores
    S = X R are stored in the type of X, so each carries a relative 2^-24; d SSE = 2 sum |r| |dS q| <= 2 A 2^-24 max(SSE) by
    Cauchy-Schwarz over at most A terms per row -- 2 A 2^-24 of the largest entry"""
    from pls_amd import _lib as L
    import pls_amd
    t0 = time.time()
    torch = _torch()
    ld = case_ld(pitch, dt, K)
    rng = np.random.default_rng(9)
    Xh, Yh = _round(oracle.synth_x(0, N, K), dt), _round(oracle.synth_y(0, N, M), dt)
    Rh = np.asfortranarray(rng.standard_normal((K, A)) / K); Qh = np.asfortranarray(rng.standard_normal((M, A)))
    R = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K); R.copy_(torch.from_numpy(Rh))
    Q = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M); Q.copy_(torch.from_numpy(Qh))

    def call(h, lay):
        X, Y = lay.inp("X", Xh), lay.inp("Y", Yh)
        out = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M)
        L.check(L.lib().pls_hip_model_sse(h.h, _ptr(X), _ldv(X), _ptr(Y), _ldv(Y), N, K, M, A, _ptr(R), _ptr(Q), _code(dt), L.MEM_DEVICE,
                                          _ptr(out)), h.h)
        h.synchronize()
        return out.cpu().numpy()

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    ref = _sse_reference(Xh @ Rh, Yh, Qh)
    rel = SSE_BAR if dt == "f64" else 2 * A * 2.0 ** -24
    assert np.abs(got - ref).max() < rel * np.abs(ref).max() and np.abs(got - twin).max() < rel * np.abs(ref).max()
    _record("model_sse", f"m{M}-a{A}-{long}", dt, N, K, ld, {}, "not observable", f"{np.abs(got - ref).max() / np.abs(ref).max():.1e} / {rel:.1e}", t0)


# ---- pls_hip_x_diagnostics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,A,dt,pitch,long", XDIAG_CASES)
def test_x_diagnostics(arena, oracle, N, K, A, dt, pitch, long):
    """X and S live in the storage type, Qres and T2 in fp64: an arena holds one type, so fp32 cases place X and S, or (with a
    compact fp32 X) Qres and T2 in an fp64 arena"""
    from pls_amd import _lib as L
    from test_gpu_xdiag import check_outputs
    import pls_amd
    t0 = time.time()
    torch = _torch()
    f64 = torch.float64
    adt = "f64" if (dt == "f32" and set(long) <= set("QT")) else dt      # the arena's type
    ld = case_ld(pitch, adt, K if "X" in long else A)
    Xh = _round(oracle.synth_x(0, N, K), dt)
    fit = _cached(("xd", N, K, A), lambda: oracle.plsr(oracle.synth_x(0, N, K), oracle.synth_y(0, N, 1), A))
    Rh, Ph = np.asfortranarray(fit["R"]), np.asfortranarray(fit["P"])
    R = pls_amd.colmajor_empty(K, A, f64, "cuda", ld=K); R.copy_(torch.from_numpy(Rh))
    P = pls_amd.colmajor_empty(K, A, f64, "cuda", ld=K); P.copy_(torch.from_numpy(Ph))

    def call(h, lay):
        X = lay.inp("X", Xh, dtype=_tdt(dt))
        o = dict(Q=lay.out("Q", N, A, dtype=f64), T2=lay.out("T", N, A, dtype=f64), S=lay.out("S", N, A, dtype=_tdt(dt)),
                 ssx=torch.empty(A + 1, dtype=f64, device="cuda"), sst=torch.empty(A, dtype=f64, device="cuda"))
        L.check(L.lib().pls_hip_x_diagnostics(h.h, _ptr(X), _ldv(X), N, N, K, A, _ptr(R), _ptr(P), None, _code(dt), L.MEM_DEVICE,
                                              _ptr(o["Q"]), _ldv(o["Q"]), _ptr(o["T2"]), _ldv(o["T2"]), _ptr(o["S"]), _ldv(o["S"]),
                                              _ptr(o["ssx"]), _ptr(o["sst"])), h.h)
        h.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    with handle_with_env() as h:
        got, twin = _both(arena, adt, ld, long, lambda lay: call(h, lay))
    pre = check_outputs(f"long ld {N}x{K} {dt} {pitch} {long}", got, Xh, Rh, Ph, record=False)
    check_outputs("its compact twin", twin, Xh, Rh, Ph, record=False, pre=pre)
    _record("x_diagnostics", long, dt, N, K, ld, {}, "not observable", "inside the bars of test_xdiag_ref.xdiag_bars", t0)


# ---- pls_hip_synth_x / _y -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,row0,n,cols,dt,pitch", SYNTH_CASES)
def test_synth(arena, oracle, which, row0, n, cols, dt, pitch):
    from pls_amd import _lib as L
    import pls_amd
    t0 = time.time()
    ld = case_ld(pitch, dt, cols)
    lay = Lay(arena, dt, ld, "o")
    out = lay.out("o", n, cols)
    with handle_with_env() as h:
        fn = L.lib().pls_hip_synth_x if which == "x" else L.lib().pls_hip_synth_y
        L.check(fn(h.h, _ptr(out), ld, row0, n, cols, pls_amd.SEED_DEFAULT, _code(dt)), h.h)
        h.synchronize()
    lay.check()
    twin = (oracle.synth_x if which == "x" else oracle.synth_y)(row0, n, cols)          # the host twin: the same bits
    want = twin.astype(np.float32) if dt == "f32" else twin                           # (fp32 storage: the fp64 value rounded once)
    assert np.array_equal(out.cpu().numpy(), want)
    _record("synth_" + which, f"rows {row0}+{n}", dt, n, cols, ld, {}, "not observable", "bit-equal to the host twin", t0)


# ---- pls_hip_cv_folds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,N,K,M,A,ts,nf,dt,pitch,long", CV_CASES)
def test_cv_folds(arena, oracle, route, N, K, M, A, ts, nf, dt, pitch, long):
    t0 = time.time()
    ld = case_ld(pitch, dt, K)
    Xh, Yh = _round(oracle.synth_x(0, N, K), dt), _round(oracle.synth_y(0, N, M), dt)
    rng = np.random.default_rng(N + nf)
    idx = np.stack([rng.permutation(N)[:ts] for _ in range(nf)]).astype(np.int64)

    def call(h, lay):
        (E, lau) = _launches(h, lambda: h.cv_folds(lay.inp("X", Xh), lay.inp("Y", Yh), A, idx))
        return E.cpu().numpy(), lau

    with handle_with_env(**({"PLS_HIP_CV_REFIT": 1} if route == "refit" else {})) as h:
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    ref = _cached(("cv", N, K, M, A, ts, nf, dt), lambda: _fold_reference(oracle, Xh, Yh, A, idx))
    # test_gpu_bounds.test_cv_folds_write_exactly_e; fp32 refits store their scores in fp32: test_cv_folds_refit_per_fold; the batched
    # route accumulates in fp64 throughout: test_batched_cv_folds_fp32_storage, 1e-8 absolute
    bar = 1e-8 if (dt == "f32" and route == "batched") else (2e-4 if dt == "f32" else CV_BAR) * max(np.abs(ref).max(), 1.0)
    assert np.abs(got - ref).max() < bar and np.abs(got - twin).max() < bar
    _record("cv_folds", f"{route}-{long}", dt, N, K, ld, {}, f"{route} by its switch: {dict(lau)}", f"{np.abs(got - ref).max():.1e} / {bar:.1e}", t0)


@pytest.mark.parametrize("name,pitch,long", CV_DUAL_CASES)
def test_cv_folds_dual(arena, name, pitch, long):
    import pls_amd
    from test_dual_cv_ref import BAR, CASES, case_data, case_reference, rel_err
    t0 = time.time()
    N, K, M, A, ts, nf, dt = CASES[name]
    ld = case_ld(pitch, dt, K)
    Xh, Yh, A, idx = case_data(name)

    def call(h, lay):
        (E, lau) = _launches(h, lambda: h.cv_folds(lay.inp("X", Xh), lay.inp("Y", Yh), A, idx))
        return E.cpu().numpy(), lau

    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, DUAL)
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    err = rel_err(got, case_reference(name))
    assert err < BAR and rel_err(got, twin) < BAR
    _route_check("dual", lau, A, name)
    _record("cv_folds DUAL", f"{name}-{long}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {}, f"dual: {dict(lau)}", f"{err:.1e} / {BAR:.0e}", t0)


# ---- pls_hip_fit_batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,N,K,M,A,nprob,dt,pitch,long", BATCH_CASES)
def test_fit_batch(arena, oracle, po, route, N, K, M, A, nprob, dt, pitch, long):
    from test_gpu_fit_batch import as_np, check_batch, problem_set
    t0 = time.time()
    cols = max(K if "X" in long else 0, nprob * M if "Y" in long else 0)      # the widest of the long matrices
    ld = case_ld(pitch, dt, cols)
    Xh, Ysh, y = problem_set(po, oracle, N, K, M, A, nprob, dt)

    def call(h, lay):
        out, lau = _launches(h, lambda: h.fit_batch(lay.inp("X", Xh), lay.inp("Y", Ysh), M, A, want=("R", "Q", "tt", "B", "ssy")))
        return as_np(out), lau

    with handle_with_env(**({"PLS_HIP_BATCH_REFIT": 1} if route == "refit" else {})) as h:
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    check_batch(po, got, y, Xh, A, f"long ld {route} {N}x{K} m{M} a{A} p{nprob} {dt} {pitch} {long}")
    check_batch(po, got, twin, Xh, A, "against its compact twin")
    assert lau["fused"] == 0 and lau["deflate"] == 0, lau      # test_gpu_hard_data._launch_check, "batch": no pass over X per component
    if route == "batched":    # X^T X and X^T Ys once for the call, whatever the number of problems
        assert lau["xty"] < max(nprob, 3) and lau["xb"] == 0, lau      # (2 in one round of problems)
    else:                     # one KERNEL_TYPE2 fit per problem: each forms its own X^T X and X^T Y_b
        assert nprob >= 3 and lau["xty"] >= nprob and lau["xb"] == 0, lau
    _record("fit_batch", f"{route}-m{M}-a{A}-p{nprob}-{long}", dt, N, cols, ld, {"total": "past"} if pitch == "total" else {},
            f"{'X^T X once' if route == 'batched' else 'one fit per problem'}: {dict(lau)}", "inside test_gpu_fit_batch.bars", t0)


@pytest.mark.parametrize("name,pitch,long", BATCH_DUAL_CASES)
def test_fit_batch_dual(arena, name, pitch, long):
    import pls_amd
    from test_dual_batch_ref import CASES, case_data, case_yardstick, check
    from test_gpu_dual_batch import NAMES, _as_np
    t0 = time.time()
    N, K, M, A, nprob, dt, columns = CASES[name]
    ld = case_ld(pitch, dt, K)
    Xh, Ysh = case_data(name)

    def call(h, lay):
        out, lau = _launches(h, lambda: h.fit_batch(lay.inp("X", Xh), lay.inp("Y", Ysh), M, A, want=NAMES))
        return _as_np(out), lau

    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, DUAL)
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    check(got, case_yardstick(name), name + " long ld", columns)
    check(got, twin, name + " against its compact twin", columns)
    _route_check("dual", lau, A, name)
    _record("fit_batch DUAL", f"{name}-{long}", dt, N, K, ld, {"total": "past"}, f"dual: {dict(lau)}", "inside test_dual_batch_ref.check", t0)


# ---- pls_hip_fit_resampled ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pitch,long,dual", RESAMPLE_CASES)
def test_fit_resampled(arena, name, pitch, long, dual):
    """(the weights are fp64 whatever X is stored in: with fp32 storage they stay compact, an arena holds one type)"""
    import pls_amd
    from test_gpu_resample import NAMES, _as_np
    from test_resample_ref import CASES, case_data, case_yardstick, check
    t0 = time.time()
    torch = _torch()
    N, K, M, A, nrep, dt, _ = CASES[name]
    ld = case_ld(pitch, dt, K)
    Xh, Yh, Wh = case_data(name)
    assert dt == "f64" or "W" not in long

    def call(h, lay):
        Wt = lay.inp("W", Wh, dtype=torch.float64)
        out, lau = _launches(h, lambda: h.fit_resampled(lay.inp("X", Xh), lay.inp("Y", Yh), A, Wt, want=NAMES))
        return _as_np(out), lau

    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, DUAL if dual else KERNEL)
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    y = case_yardstick(name)
    check(got, y, name + " long ld")
    check(twin, y, name + " compact twin")
    # ... and against each other at the same bars (the twin's own standard errors in the yardstick's place)
    check(got, dict(twin, se=np.sqrt(np.maximum(twin["Bm2"], 0.0)), rho=y["rho"]), name + " against its compact twin")
    if dual:
        assert lau["fused"] == 0 and lau["deflate"] == 0, lau
    _record("fit_resampled" + (" DUAL" if dual else ""), f"{name}-{long}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {},
            f"{'dual' if dual else 'refits'}: {dict(lau)}", "inside test_resample_ref.check", t0)


# ---- pls_hip_cv_press_batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pitch,long,dual", CVBATCH_CASES)
def test_cv_press_batch(arena, name, pitch, long, dual):
    import pls_amd
    from test_dual_cv_ref import BAR, CASES, rel_err
    from test_dual_cvbatch_ref import CASES_B, PRESS_TOL, case_data_b, case_reference_b, press_err
    t0 = time.time()
    Xh, Ysh, M, A, idx, nprob = case_data_b(name)
    dt = CASES[CASES_B[name][0]][6]
    N, K = Xh.shape
    ld = case_ld(pitch, dt, K)

    def call(h, lay):
        out, lau = _launches(h, lambda: h.cv_press_batch(lay.inp("X", Xh), lay.inp("Y", Ysh), M, A, idx, want=("PRESS", "ssy", "E")))
        return {k: v.cpu().numpy().copy() for k, v in out.items()}, lau

    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, DUAL if dual else KERNEL)
        (got, lau), (twin, _) = _both(arena, dt, ld, long, lambda lay: call(h, lay))
    err = rel_err(got["E"], case_reference_b(name))
    assert err < BAR and rel_err(got["E"], twin["E"]) < BAR            # test_gpu_dual_cvbatch._check
    assert press_err(got["PRESS"], got["E"]) <= PRESS_TOL
    assert np.array_equal(got["ssy"], twin["ssy"]) or np.abs(got["ssy"] / twin["ssy"] - 1).max() <= PRESS_TOL
    _record("cv_press_batch" + (" DUAL" if dual else ""), f"{name}-{long}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {},
            f"{'dual' if dual else 'one cross-validation per problem'}: {dict(lau)}", f"E {err:.1e} / {BAR:.0e}", t0)


# ---- the missing-value entry points: the gaps hold 1e300 / 3e38, NaN means "missing" ---------------------------------------------------
def _missing_case(name):
    from test_missing_ref import CASES, case_data
    N, K, M, A, frac, dt = CASES[name]
    X, Y, Xc = case_data(name)
    return N, K, M, A, dt, X, Y, Xc


@pytest.mark.parametrize("name,pitch,long", MISSING_FIT_CASES)
def test_fit_missing(arena, name, pitch, long):
    from pls_amd import _lib as L
    from test_gpu_missing import _check
    from test_missing_ref import case_yardstick, gpu_bar
    import pls_amd
    t0 = time.time()
    torch = _torch()
    N, K, M, A, dt, Xh, Yh, _ = _missing_case(name)
    ld = case_ld(pitch, dt, K)

    def call(h, lay):
        X, Y, T = lay.inp("X", Xh), lay.inp("Y", Yh), lay.out("T", N, A)
        o = {k: pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K) for k in "WPR"}
        o["Q"] = pls_amd.colmajor_empty(M, A, torch.float64, "cuda", ld=M); o["B"] = pls_amd.colmajor_empty(K, M, torch.float64, "cuda", ld=K)
        iters = torch.empty(A, dtype=torch.int64, device="cuda")
        L.check(L.lib().pls_hip_fit_missing(h.h, _ptr(X), _ldv(X), _ptr(Y), _ldv(Y), N, K, M, A, _code(dt), L.MEM_DEVICE, _ptr(o["W"]),
                                            _ptr(o["P"]), _ptr(o["Q"]), _ptr(o["R"]), _ptr(T), _ldv(T), _ptr(o["B"]), _ptr(iters)), h.h)
        h.synchronize()
        o = {k: v.cpu().numpy().astype(np.float64) for k, v in o.items()}
        o["T"] = T.cpu().numpy()
        o["iters"] = iters.cpu().numpy()
        return o

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay), fill="huge")
    y = case_yardstick(name)
    w = _check(got, y, gpu_bar(name), M > 1, f"{name} long ld {pitch} {long}")
    _check(got, twin, gpu_bar(name), M > 1, f"{name} against its compact twin")
    assert (np.abs(got["iters"] - y["iters"]) <= 1).all()
    _record("fit_missing", f"{name}-{long}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {}, "not observable",
            f"{max(w.values()):.1e} / {gpu_bar(name):.1e}", t0)


@pytest.mark.parametrize("name,pitch,long", MISSING_SCORES_CASES)
def test_scores_missing(arena, handle, name, pitch, long):
    from pls_amd import _lib as L
    from test_gpu_missing import _dev, _heldout
    from test_missing_ref import TOL_F32, TOL_F64, rel, scores_missing_ref
    import pls_amd
    t0 = time.time()
    torch = _torch()
    N, K, M, A, dt, Xh, Yh, _ = _missing_case(name)
    ld = case_ld(pitch, dt, K if "X" in long else A)
    m = _cached(("mfit", name), lambda: {k: v.cpu().numpy() for k, v in handle.fit_missing(_dev(Xh, _tdt(dt)), _dev(Yh, _tdt(dt)), A).items()})
    W = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K); W.copy_(torch.from_numpy(m["W"]))
    P = pls_amd.colmajor_empty(K, A, torch.float64, "cuda", ld=K); P.copy_(torch.from_numpy(m["P"]))
    _, Xm = _heldout(name)            # 37 rows the model has not seen, a fifth of their cells missing
    n = Xm.shape[0]
    bar = TOL_F32 if dt == "f32" else TOL_F64     # test_gpu_missing.test_scores_missing

    def call(h, rows, lay):
        X, S = lay.inp("X", rows), lay.out("S", rows.shape[0], A)
        L.check(L.lib().pls_hip_scores_missing(h.h, _ptr(X), _ldv(X), rows.shape[0], K, A, _ptr(W), _ptr(P), _code(dt), L.MEM_DEVICE,
                                               _ptr(S), _ldv(S)), h.h)
        h.synchronize()
        return S.cpu().numpy().astype(np.float64)

    with handle_with_env() as h:
        train, train_twin = _both(arena, dt, ld, long, lambda lay: call(h, Xh, lay), fill="huge")
        held, held_twin = _both(arena, dt, ld, long, lambda lay: call(h, Xm, lay), fill="huge")
    e1 = rel(train, m["T"])                                   # the training X reproduces T
    ref = scores_missing_ref(Xm, m["W"], m["P"])
    e2 = max(rel(held[:, a], ref[:, a]) for a in range(A))
    assert e1 <= bar and e2 <= bar and rel(train, train_twin) <= bar and max(rel(held[:, a], held_twin[:, a]) for a in range(A)) <= bar
    _record("scores_missing", f"{name}-{long}", dt, n, K, ld, {"total": "past"} if pitch == "total" else {}, "not observable",
            f"{max(e1, e2):.1e} / {bar:.0e}", t0)


@pytest.mark.parametrize("name,pitch,mode", MISSING_Z_CASES)
def test_colwise_z_scores_missing(arena, name, pitch, mode):
    from pls_amd import _lib as L
    from test_missing_ref import rel, z_scores_missing_ref
    t0 = time.time()
    torch = _torch()
    N, K, M, A, dt, Xh, _, _ = _missing_case(name)
    ld = case_ld(pitch, dt, K)
    Xs = _round(np.array(Xh + np.linspace(-2.0, 3.0, K), order="F"), dt)
    Zr, mr, sr, nr = z_scores_missing_ref(Xs)
    long = {"src": "s", "dst": "d", "both": "sd", "inplace": "s"}[mode]

    def call(h, lay):
        X = lay.inp("s", Xs, inout=mode == "inplace")
        Z = X if mode == "inplace" else lay.out("d", N, K)
        mean = torch.empty(K, dtype=torch.float64, device="cuda"); sd = torch.empty(K, dtype=torch.float64, device="cuda")
        nobs = torch.empty(K, dtype=torch.int64, device="cuda")
        L.check(L.lib().pls_hip_colwise_z_scores_missing(h.h, _ptr(X), _ldv(X), N, K, _code(dt), L.MEM_DEVICE, _ptr(Z), _ldv(Z), _ptr(mean),
                                                         _ptr(sd), _ptr(nobs)), h.h)
        h.synchronize()
        return Z.cpu().numpy().astype(np.float64), mean.cpu().numpy(), sd.cpu().numpy(), nobs.cpu().numpy()

    with handle_with_env() as h:
        got, twin = _both(arena, dt, ld, long, lambda lay: call(h, lay), fill="huge")
    zbar = 1e-12 if dt == "f64" else 1e-6         # test_gpu_missing.test_z_scores_missing
    for Z, mean, sd, nobs in (got, twin):
        assert np.array_equal(nobs, nr) and np.array_equal(np.isnan(Z), np.isnan(Zr))
        assert rel(mean, mr) <= 1e-12 and rel(sd, sr) <= 1e-12 and rel(np.nan_to_num(Z), np.nan_to_num(Zr)) <= zbar
    _record("colwise_z_scores_missing", f"{name}-{mode}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {}, "not observable",
            f"Z {rel(np.nan_to_num(got[0]), np.nan_to_num(Zr)):.1e} / {zbar:.0e}", t0)


@pytest.mark.parametrize("name,pitch,long", MISSING_CV_CASES)
def test_cv_folds_missing(arena, name, pitch, long):
    from test_gpu_missing_cv import _check
    from test_missing_cv_ref import case_folds, cv_gpu_bar, cv_yardstick
    t0 = time.time()
    N, K, M, A, dt, Xh, Yh, _ = _missing_case(name)
    ld = case_ld(pitch, dt, K)
    idx = case_folds(name)

    def call(h, lay):
        E, iters = h.cv_folds_missing(lay.inp("X", Xh), lay.inp("Y", Yh), A, idx, want_iters=True)
        h.synchronize()
        return np.ascontiguousarray(E.cpu().numpy()), iters.cpu().numpy()

    with handle_with_env() as h:
        (E, iters), (Et, it) = _both(arena, dt, ld, long, lambda lay: call(h, lay), fill="huge")
    Eref, iref = cv_yardstick(name)
    _check(E, iters, Eref, iref, cv_gpu_bar(name), M, f"{name} long ld {pitch} {long}")
    _check(E, iters, Et, it, cv_gpu_bar(name), M, f"{name} against its compact twin")
    _record("cv_folds_missing", f"{name}-{long}", dt, N, K, ld, {"total": "past"} if pitch == "total" else {}, "not observable",
            f"inside cv_gpu_bar {cv_gpu_bar(name):.1e}", t0)


# ---- the record -------------------------------------------------------------------------------------------------------------------------
def test_zz_record():
    """what ran: entry point, case, storage, N, K, ld, the guards crossed and their side, the route observed, error / bar, seconds"""
    if not RECORD:
        pytest.skip("no case of this module ran in this session")
    print()
    print(f"{'entry point':26s} {'case':26s} {'dt':3s} {'N':>6s} {'K':>6s} {'ld':>10s}  {'s':>5s}  guards | route | error / bar")
    for entry, case, dt, N, K, ld, guards, route, err, secs in RECORD:
        print(f"{entry:26s} {case:26s} {dt:3s} {N:6d} {K:6d} {ld:10d}  {secs:5.1f}  {guards} | {route} | {err}")
    slow = max(RECORD, key=lambda r: r[-1])
    print(f"{len(RECORD)} cases, {sum(r[-1] for r in RECORD):.0f} s in all, the slowest {slow[0]} {slow[1]} at {slow[-1]:.1f} s")
