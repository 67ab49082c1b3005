"""The turn-around of the deflating passes: consecutive in-place sweeps of a NIPALS fit walk the tiles in opposite directions
(components 0 and 1 ascend, component 2 descends, component 3 ascends, ...) and the first / last S bytes of a sweep -- its
edges -- drop the streaming cache policy, so that the Infinity Cache hands them from one sweep to the next
(fused_pass_kernel, "direction and edges").  Read-only passes (component 0, the KERNEL plan) keep the ascending walk.

Reversing a sweep changes which tiles a workgroup sums, nothing else.  Checked here: parity against the oracle with the
tolerances test_gpu_parity.py uses for the storage type, switch on and off, on one shape per route of
test_gpu_last_pass.py's table and on matrices with more / fewer tiles than two edges; that a fit gives the same bits twice
and whatever ran before it on the handle; the EDGE instantiations; and that the profiler books the same bytes.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import handle_with_env
from test_gpu_parity import check_against, oracle_ref, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AS = [1, 2, 3, 6, 7]  # both parities of the last component
F32_TOL = dict(tol_b=2e-5, tol_col=2e-5, tol_inv=1e-4)  # test_fp32_storage, test_wide_matrix_fp32


def _torch():
    import torch
    return torch


@contextlib.contextmanager
def _nipals_handle(switch, layout=1, **env):
    import pls_amd
    with handle_with_env(PLS_HIP_TURNAROUND=switch, **env) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        h.set_option(pls_amd.OPT_FUSE, 1)
        h.set_option(pls_amd.OPT_WORK_LAYOUT, layout)
        yield h


def _fit_and_check(h, oracle, po, X, Y, A, dt, Xh=None, Yh=None):
    if Xh is None:
        Xh, Yh = X.cpu().numpy().astype(np.float64), Y.cpu().numpy().astype(np.float64)
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    out = h.fit_device(X, Y, A); h.synchronize()
    check_against(po, out, ref, Bref, ref["T"], col_err=cerr, **(F32_TOL if dt == "f32" else {}))


# one shape per route of test_gpu_last_pass.py's SHAPES (route, N, K, M, storage, work layout); all of them have fewer
# tiles than two edges: every tile takes the edge's policy
SHAPES = [("tall", 4098, 512, 1, "f64", 1), ("tall-ragged", 3000, 96, 3, "f32", 1), ("layout0", 3000, 96, 3, "f64", 0),
          ("half", 1030, 700, 2, "f64", 1), ("short", 516, 2048, 8, "f32", 1), ("tailrows", 4097, 200, 2, "f64", 1)]


@pytest.mark.parametrize("switch", [0, 1])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("route,N,K,M,dt,layout", SHAPES)
def test_turnaround_parity(oracle, po, route, N, K, M, dt, layout, A, switch):
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    with _nipals_handle(switch, layout) as h:
        X = h.synth_x(0, N, K, 41, dtype=dtype); Y = h.synth_y(0, N, M, 41, dtype=dtype)
        _fit_and_check(h, oracle, po, X, Y, A, dt)


@pytest.mark.parametrize("switch", [0, 1])
@pytest.mark.parametrize("A", [3, 6])
def test_turnaround_parity_kernel_plan(oracle, po, A, switch):
    """the KERNEL plan's passes are read-only: they keep the ascending walk and one policy, so the switch must be inert
    there -- same parity either way"""
    import pls_amd
    with handle_with_env(PLS_HIP_TURNAROUND=switch, PLS_HIP_TINY=0, PLS_HIP_RESIDENT=0) as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_KERNEL)
        X = h.synth_x(0, 4098, 512, 41); Y = h.synth_y(0, 4098, 2, 41)
        _fit_and_check(h, oracle, po, X, Y, A, "f64")


# More tiles than two edges: the edge is overridden (testing build only, PLS_HIP_TEST_TURN_EDGE_BYTES) to an EIGHTH of the
# matrix, so that a sweep has a leading edge, a streaming bulk with the weighted walk's switch point in it, and a trailing
# edge.  The launcher rounds the edge down to whole rounds of its grid (grid x tile bytes); the matrices are sized so that
# an eighth of them holds at least one round for any grid up to 512 workgroups and any tile up to 128 KB (64 MB per
# round), whatever tile height the plan picks -- and two edges of an eighth each can never cover the sweep.  The testing
# build reports what the launcher made of it (pls_hip_test_last_turn), so the case checks itself: were the override ignored,
# every tile would be edge and the assertion on 2 * edge < ntiles fails.
# Runs in a child process: the testing library is chosen when pls_amd is first imported.
_BULK_CODE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch, pls_amd
from oracle import pls_oracle as po
from test_gpu_parity import check_against, oracle_ref
import ctypes
torch.cuda.set_device(0)
ora = po.OracleLib()
lib = ctypes.CDLL(os.environ["PLS_AMD_LIBRARY"])  # (the testing build: already loaded by pls_amd, the same image)
lib.pls_hip_test_last_turn.argtypes = [ctypes.POINTER(ctypes.c_int)]
F32_TOL = dict(tol_b=2e-5, tol_col=2e-5, tol_inv=1e-4)
for N, K, M, dt in ((131074, 512, 1, "f64"), (450002, 300, 3, "f32")):
    dtype = torch.float64 if dt == "f64" else torch.float32
    s = 8 if dt == "f64" else 4
    edge_bytes = N * K * s // 8
    assert edge_bytes >= 512 * 128 * 1024, "an eighth of the matrix must hold a whole round of the largest grid"
    refs = {}
    for switch in (0, 1):
        os.environ["PLS_HIP_TURNAROUND"] = str(switch)
        os.environ["PLS_HIP_TEST_TURN_EDGE_BYTES"] = str(edge_bytes)
        h = pls_amd.Handle()
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        h.set_option(pls_amd.OPT_WORK_LAYOUT, 1)  # (the tiled working copy: the route that has edges)
        X = h.synth_x(0, N, K, 41, dtype=dtype); Y = h.synth_y(0, N, M, 41, dtype=dtype)
        Xh, Yh = X.cpu().numpy().astype(np.float64), Y.cpu().numpy().astype(np.float64)
        for A in (1, 2, 3, 6, 7):
            if A not in refs:
                refs[A] = oracle_ref(ora, po, Xh, Yh, A)
            ref, Bref, cerr = refs[A]
            out = {k: v.clone() for k, v in h.fit_device(X, Y, A).items()}; h.synchronize()
            check_against(po, out, ref, Bref, ref["T"], col_err=cerr, **(F32_TOL if dt == "f32" else {}))
            again = h.fit_device(X, Y, A); h.synchronize()
            for k in "WPQRTB":
                assert torch.equal(out[k], again[k]), (N, K, A, switch, k)
            if A >= 6:
                # what the launcher handed the last storing pass (component A - 2, in place on the tiled copy): with the switch
                # on whole rounds of edge at either end and a bulk between them, direction by the component index; off: neither
                rec = (ctypes.c_int * 4)()
                assert lib.pls_hip_test_last_turn(rec) == 0
                rev, edge, ntiles, grid = list(rec)
                if switch:
                    assert edge > 0 and edge %% grid == 0 and 2 * edge < ntiles, (N, K, A, list(rec))
                    assert rev == (1 if (A - 2) %% 2 == 0 else 0), (A, list(rec))
                else:
                    assert edge == 0 and rev == 0 and ntiles > 0, (N, K, A, list(rec))
        h.close()
print("bulk ok")
'''


def test_turnaround_parity_more_tiles_than_two_edges():
    env = dict(os.environ, PLS_AMD_LIBRARY=os.path.join(ROOT, "pls_amd", "csrc", "testing", "libpls_hip.so"))
    r = subprocess.run([sys.executable, "-c", _BULK_CODE % (ROOT, ROOT)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "bulk ok" in r.stdout, r.stdout[-1500:]


@pytest.mark.parametrize("N,K,M,dt,layout", [(4098, 512, 1, "f64", 1), (3000, 96, 3, "f32", 1), (1030, 700, 2, "f64", 1),
                                             (4097, 200, 2, "f64", 0), (200000, 512, 1, "f64", 1)])
def test_turnaround_is_deterministic(N, K, M, dt, layout):
    """the same fit twice, and the same fit after a fit with another number of components (whose last sweep ran the other
    way) on the same handle: the direction is a function of the component index alone, so all outputs are bit-equal"""
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    A = 5
    with _nipals_handle(1, layout) as h:
        X = h.synth_x(0, N, K, 47, dtype=dtype); Y = h.synth_y(0, N, M, 47, dtype=dtype)
        first = {k: v.clone() for k, v in h.fit_device(X, Y, A).items()}; h.synchronize()
        second = {k: v.clone() for k, v in h.fit_device(X, Y, A).items()}; h.synchronize()
        h.fit_device(X, Y, A + 1); h.synchronize()
        X2 = h.synth_x(0, N // 2 + 1, K, 48, dtype=dtype); Y2 = h.synth_y(0, N // 2 + 1, M, 48, dtype=dtype)
        h.fit_device(X2, Y2, 2); h.synchronize()
        third = h.fit_device(X, Y, A); h.synchronize()
        for k in "WPQRTB":
            assert torch.isfinite(first[k]).all(), k
            assert torch.equal(first[k], second[k]), k
            assert torch.equal(first[k], third[k]), k


@pytest.mark.parametrize("A", [3, 6])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_turnaround_edge_route_unaligned_columns(oracle, po, dt, A):
    """ld = N with N odd (EDGE = 2: the tiles are dealt out per XCD; the walk turns around, the policy stays)"""
    from test_gpu_edge import _place
    torch = _torch()
    tdt = torch.float64 if dt == "f64" else torch.float32
    N, K, M = 1001, 37, 2
    Xh = oracle.synth_x(0, N, K); Yh = oracle.synth_y(0, N, M)
    if dt == "f32":
        Xh = Xh.astype(np.float32).astype(np.float64); Yh = Yh.astype(np.float32).astype(np.float64)
    with _nipals_handle(1, 1, PLS_HIP_TINY=0) as h:
        X, keepx = _place(Xh, tdt, 0, 0)
        Y, keepy = _place(Yh, tdt, 0, 0)
        _fit_and_check(h, oracle, po, X, Y, A, dt, Xh, Yh)
        assert np.array_equal(X.cpu().numpy().astype(np.float64), Xh)


@pytest.mark.parametrize("A", [3, 6])
def test_turnaround_edge_route_long_leading_dimension(oracle, po, A):
    """a leading dimension of 2^23 + 2 rows: the 32 column groups of a tile span more than one buffer descriptor addresses
    (EDGE = 1, a descriptor per wave) -- the route test_gpu_edge.py reaches with a 2^24-row matrix, here with few rows in
    long columns so that the oracle can follow"""
    from test_gpu_edge import _place
    torch = _torch()
    N, K, M = 5000, 260, 1
    Xh = oracle.synth_x(0, N, K); Yh = oracle.synth_y(0, N, M)
    with _nipals_handle(1, 1, PLS_HIP_TINY=0, PLS_HIP_RESIDENT=0) as h:
        X, keepx = _place(Xh, torch.float64, (1 << 23) + 2 - N, 0)
        Y = to_dev(Yh)
        _fit_and_check(h, oracle, po, X, Y, A, "f64", Xh, Yh)
        assert np.array_equal(X.cpu().numpy(), Xh)


@pytest.mark.parametrize("switch", [0, 1])
@pytest.mark.parametrize("A", [1, 2, 3, 7])
@pytest.mark.parametrize("N,K,dt,layout", [(4098, 512, "f64", 1), (3000, 96, "f32", 1), (4098, 512, "f64", 0)])
def test_turnaround_books_the_same_bytes(N, K, dt, layout, A, switch):
    """algorithmic bytes do not depend on where they are served from: the `fused` family books what
    test_gpu_last_pass.py::test_profiler_books_one_sweep_for_the_last_pass states, switch on or off"""
    import pls_amd
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    s = 8 if dt == "f64" else 4
    want = 0
    for a in range(A):
        sweeps = 1 if (a == 0 or a == A - 1) else 2
        want += sweeps * N * K * s + (1 if a == 0 else 2) * N * s + (2 if a == 0 else 3) * K * 8
    with _nipals_handle(switch, layout) as h:
        h.set_option(pls_amd.OPT_PROFILE, 1)
        X = h.synth_x(0, N, K, 53, dtype=dtype); Y = h.synth_y(0, N, 1, 53, dtype=dtype)
        h.timing()
        h.fit_device(X, Y, A); h.synchronize()
        tm = h.timing()
        assert tm["launches"]["fused"] == A
        assert tm["bytes"]["fused"] == want, (tm["bytes"]["fused"], want)
