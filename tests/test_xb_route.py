"""The routes of X * Bm, checked without a GPU: xb_next (pls_amd/csrc/xb_route.hpp) is a pure function of the shape, so the
kernel, template selectors and column count of every step of every row of test_gpu_bounds.XB_ROUTES can be asserted on the
CPU, and so can what a call falls back to when a route is refused its resource (dynamic LDS, the partial buffer) -- which
no GPU test provokes.  tests/cpp/xb_route.cpp, built with ASan + UBSan, plans the steps."""
import os
import re
import subprocess

import pytest

from test_gpu_bounds import XB_ROUTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CU = 256
# bits of plsk::XbRoute
SPLIT, MFMA4, MFMA4W, MFMA4W_SPLIT = 1 << 3, 1 << 5, 1 << 6, 1 << 7
OPTIONAL = SPLIT | MFMA4 | MFMA4W | MFMA4W_SPLIT

# (row, refused routes) -> the steps: the next branch of the cascade, derived by hand from the thresholds
A, E = "aligned", "eigen"
XB_DENIED = {
    ((512, 20000, 1, "f64", A, A, None), SPLIT): ["xb_kernel<1,1> (1)"],           # (Bm beyond LDS: not the "few" form)
    ((5000, 1200, 3, "f64", A, A, None), SPLIT): ["xb_kernel<1,4> (3)"],
    ((300, 9000, 6, "f64", E, E, None), SPLIT): ["xb_wide<1,8> (6)"],
    ((2100, 3000, 2, "f32", E, A, None), SPLIT): ["xb_kernel<1,2> (2)"],
    ((262144 + 37, 70, 21, "f64", A, A, None), MFMA4): ["xb_mfma4w<2,6> (21)"],
    ((262144 + 37, 70, 21, "f64", A, A, None), MFMA4 | MFMA4W): ["xb_wide<1,24> (21)"],
    ((524288 + 5, 33, 26, "f32", A, A, None), MFMA4): ["xb_mfma_lds<4,2> (26)"],    # (26 columns: beyond the windowed form's 20)
    ((262144 + 5, 128, 3, "f64", A, A, None), MFMA4): ["xb_kernel<1,4> (3)"],
    ((40001, 200, 19, "f64", A, A, None), MFMA4W): ["xb_wide<1,20> (19)"],
    ((70000 + 3, 130, 18, "f32", A, A, None), MFMA4W): ["xb_mfma_lds<4,2> (18)"],
    ((2000, 5000, 21, "f64", A, A, None), MFMA4W_SPLIT): ["xb_split<1,4> + finish (4)"] * 5 + ["xb_split<1,4> + finish (1)"],
    ((2000, 5000, 21, "f64", A, A, None), MFMA4W_SPLIT | SPLIT): ["xb_wide<1,24> (21)"],
    ((1001, 9001, 5, "f64", A, E, None), MFMA4W_SPLIT): ["xb_split<1,4> + finish (4)", "xb_split<1,4> + finish (1)"],
    ((1001, 9001, 5, "f64", A, E, None), MFMA4W_SPLIT | SPLIT): ["xb_wide<1,8> (5)"],
    ((515, 20000, 6, "f32", A, A, None), MFMA4W_SPLIT): ["xb_split<1,4> + finish (4)", "xb_split<1,4> + finish (2)"],
    ((515, 20000, 6, "f32", A, A, None), MFMA4W_SPLIT | SPLIT): ["xb_wide<1,8> (6)"],
}


# Long leading dimensions: the 4 x 4 x 4 MFMA kernels address 36 columns (32 + a prefetched group) of X and of out behind one
# descriptor, so each of their three predicates asks for 36 max(ldx, ldo) es < 2^31 (xb4_ok, xb4_few) or 36 ldx es < 2^31 (the
# column-split form, whose finish kernel writes out with plain stores).  2^31 / 36 = 59,652,323.6 bytes: the last 16-byte
# aligned ld below it and the first one beyond, on X alone, on out alone.  Past the limit the call takes what a refusal of the
# route gives in XB_DENIED above.
def _ld_limit(dt, below):
    es, V = (8, 2) if dt == "f64" else (4, 4)
    return (1 << 31) // (36 * es) // V * V + (0 if below else V)


LO64, HI64, LO32, HI32 = _ld_limit("f64", True), _ld_limit("f64", False), _ld_limit("f32", True), _ld_limit("f32", False)
assert (LO64, HI64, LO32, HI32) == (7456540, 7456542, 14913080, 14913084)
RESIDENT, FEW, SPLIT_Y = (262144 + 37, 70, 21, "f64"), (262144 + 5, 128, 3, "f64"), (2000, 5000, 21, "f64")
RESIDENT32, WINDOWED32 = (524288 + 5, 33, 26, "f32"), (70000 + 3, 130, 18, "f32")
XB_LONG_LD = {
    # xb4_ok, the resident form
    (*RESIDENT, LO64, LO64, None): ["xb_mfma4<2,6> (21)"],
    (*RESIDENT, HI64, A, None): ["xb_wide<1,24> (21)"],
    (*RESIDENT, A, HI64, None): ["xb_wide<1,24> (21)"],
    (*RESIDENT32, LO32, LO32, None): ["xb_mfma4<4,6> (24)", "xb_kernel<1,2> (2)"],
    (*RESIDENT32, HI32, A, None): ["xb_mfma_lds<4,2> (26)"],
    (*RESIDENT32, A, HI32, None): ["xb_mfma_lds<4,2> (26)"],
    # xb4_ok, the windowed form
    (*WINDOWED32, LO32, LO32, None): ["xb_mfma4w<4,5> (18)"],
    (*WINDOWED32, HI32, A, None): ["xb_mfma_lds<4,2> (18)"],
    (*WINDOWED32, A, HI32, None): ["xb_mfma_lds<4,2> (18)"],
    # xb4_few
    (*FEW, LO64, LO64, None): ["xb_mfma4<2,1> (3)"],
    (*FEW, HI64, A, None): ["xb_kernel<1,4> (3)"],
    (*FEW, A, HI64, None): ["xb_kernel<1,4> (3)"],
    # the column-split form: ldx alone
    (*SPLIT_Y, LO64, LO64, None): ["xb_mfma4w<2,6> split y=7 + finish (21)"],
    (*SPLIT_Y, LO64, HI64, None): ["xb_mfma4w<2,6> split y=7 + finish (21)"],
    (*SPLIT_Y, HI64, A, None): ["xb_split<1,4> + finish (4)"] * 5 + ["xb_split<1,4> + finish (1)"],
}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xb_route") / "xb_route")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "xb_route.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def plan(calls):
        """calls: [(row of XB_ROUTES, mask of refused routes)] -> per call the list of its steps, `kernel<selectors> (columns)`"""
        lines = []
        for (N, K, C, dt, xl, ol, xb4), denied in calls:
            es = 8 if dt == "f64" else 4
            V = 16 // es
            # test_gpu_bounds.Guarded; a number: that leading dimension (whole 16-byte vectors) on a 16-byte base
            ld = lambda layout: layout if isinstance(layout, int) else N if layout == "eigen" else -(-N // V) * V + V
            assert all(ld(l) % V == 0 and ld(l) >= N for l in (xl, ol) if isinstance(l, int))
            lines.append(f"{N} {K} {C} {es} {ld(xl)} {ld(ol)} {int(xl != 'eigen')} {int(ol != 'eigen')} {NUM_CU} "
                         f"{1 if xb4 is None else xb4} 0 {denied}")
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
        out = [[re.sub(r" \[[^\]]*\]$", "", step) for step in line.split("; ")] for line in p.stdout.splitlines()]
        assert len(out) == len(calls)
        return out
    return plan


def test_every_row_takes_its_route(planner):
    rows = list(XB_ROUTES)
    for row, got in zip(rows, planner([(r, 0) for r in rows])):
        assert got == XB_ROUTES[row], row


def test_long_leading_dimensions_leave_the_xb4_routes(planner):
    rows = list(XB_LONG_LD)
    for row, got in zip(rows, planner([(r, 0) for r in rows])):
        assert got == XB_LONG_LD[row], row


def test_a_refused_route_falls_to_the_next(planner):
    calls = list(XB_DENIED)
    assert {r for r, _ in calls} == {r for r, steps in XB_ROUTES.items() if re.match(r"xb_(split|mfma4)", steps[0])}
    for call, got in zip(calls, planner(calls)):
        assert got == XB_DENIED[call], call


def test_every_shape_ends_on_a_route_that_needs_nothing(planner):
    rows = list(XB_ROUTES)
    for row, got in zip(rows, planner([(r, OPTIONAL) for r in rows])):
        assert all(re.match(r"xb_(kernel|wide|mfma_lds)<", step) for step in got), (row, got)
