"""The last deflating pass of a fused NIPALS fit stores nothing: X_{A-1} is read by no later launch, so the pass deflates
its tiles in registers only (fused_pass_kernel<..., STORE = false>, tail_rows_kernel without a destination).

Checked here, on one shape per route that now ends in such a pass: parity against the oracle with the tolerances
test_gpu_parity.py uses for the same storage type; that no fit relies on what an earlier fit left in the work buffer; and
that the profiler books the bytes the launches now move.
"""
import numpy as np
import pytest

from conftest import handle_with_env
from test_gpu_parity import check_against, oracle_ref, to_dev

pytestmark = pytest.mark.gpu

AS = [1, 2, 3, 6]
F32_TOL = dict(tol_b=2e-5, tol_col=2e-5, tol_inv=1e-4)  # test_fp32_storage, test_wide_matrix_fp32


def _torch():
    import torch
    return torch


@pytest.fixture
def nipals(handle):
    import pls_amd
    handle.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
    handle.set_option(pls_amd.OPT_FUSE, 1)
    yield handle
    handle.set_option(pls_amd.OPT_WORK_LAYOUT, 1)
    handle.set_option(pls_amd.OPT_ALGO, 0)


def _fit_and_check(h, oracle, po, X, Y, A, dt):
    Xh, Yh = X.cpu().numpy().astype(np.float64), Y.cpu().numpy().astype(np.float64)
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    out = h.fit_device(X, Y, A); h.synchronize()
    check_against(po, out, ref, Bref, ref["T"], col_err=cerr, **(F32_TOL if dt == "f32" else {}))


# route, N, K, M, storage, work layout:
#   tall: 256-byte-segment tiles, K <= 512 -- the headline's route; component 1 reads the caller's matrix (A = 2: it is the
#         last pass and no tile copy is made), later ones the tiled copy; a ragged last tile and K no multiple of 32;
#   layout0: the column-major work buffer (the non-TILED instantiation);
#   half: 513 <= K <= 1024, half-height tiles from component 2 on (A = 2: the first deflation must not be handed their shape);
#   short: K = 2048 / 4096 in fp32 with 8 responses (short tiles, the copy made by the X^T Y sweep);
#   tailrows: N no multiple of the 16-byte row pack -- the last N % V rows are tail_rows_kernel's, which then has no destination.
SHAPES = [("tall", 4098, 512, 1, "f64", 1), ("tall", 4098, 512, 1, "f32", 1), ("tall-ragged", 3000, 96, 3, "f64", 1),
          ("tall-ragged", 3000, 96, 3, "f32", 1), ("layout0", 3000, 96, 3, "f64", 0), ("layout0", 4098, 512, 1, "f32", 0),
          ("half", 1030, 700, 2, "f64", 1), ("half", 2052, 1024, 1, "f32", 1), ("short", 516, 2048, 8, "f32", 1),
          ("short", 260, 4096, 8, "f32", 1), ("tailrows", 4097, 200, 2, "f64", 1), ("tailrows", 5003, 200, 2, "f32", 1),
          ("tailrows-layout0", 4097, 200, 2, "f64", 0)]


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("route,N,K,M,dt,layout", SHAPES)
def test_last_pass_parity(nipals, oracle, po, route, N, K, M, dt, layout, A):
    import pls_amd
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    nipals.set_option(pls_amd.OPT_WORK_LAYOUT, layout)
    X = nipals.synth_x(0, N, K, 41, dtype=dtype); Y = nipals.synth_y(0, N, M, 41, dtype=dtype)
    _fit_and_check(nipals, oracle, po, X, Y, A, dt)


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_last_pass_parity_unaligned_columns(nipals, oracle, po, dt, A):
    """odd leading dimension and an X pointer off the 16-byte grid (EDGE = 2): with A = 2 the non-storing pass itself reads
    the caller's unaligned matrix"""
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    N, K, M = 1001, 37, 2
    big = torch.empty((K, N + 3), dtype=dtype, device="cuda")
    X = big[:, 1:N + 1].t()
    X.copy_(nipals.synth_x(0, N, K, 43, dtype=dtype))
    Y = nipals.synth_y(0, N, M, 43, dtype=dtype)
    _fit_and_check(nipals, oracle, po, X, Y, A, dt)


@pytest.mark.parametrize("A", [2, 3, 6])
@pytest.mark.parametrize("N,K,M", [(4098, 96, 3), (4097, 512, 1)])
def test_last_pass_parity_two_ranks_one_gpu(oracle, po, N, K, M, A):
    """row-sharded over two members on one device: every member's last pass stores nothing, the sums they exchange are
    the ones a storing pass would have formed"""
    import pls_amd
    g = pls_amd.Group([0, 0])
    try:
        Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
        ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
        g.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        X, Y = g.upload(Xh), g.upload(Yh)
        out = g.fit(X, Y, A)
        got = dict(out); got["T"] = g.download(out["T"])
        assert po.rel_fro(out["B"], Bref) < 1e-10
        assert (po.column_errors(ref, got) <= np.maximum(1e-9, 20 * cerr)).all()
    finally:
        g.close()


@pytest.mark.parametrize("N,K,M,dt", [(3000, 96, 3, "f64"), (4098, 512, 1, "f64"), (1030, 700, 2, "f64"), (516, 2048, 8, "f32"),
                                      (4097, 200, 2, "f32")])
def test_no_fit_relies_on_the_work_buffer_of_the_previous_one(N, K, M, dt):
    """A, then A + 2, then A - 1 components on ONE handle: after a fit the work buffer holds X_{A-2}, not X_{A-1} -- it is
    scratch, and every fit starts from the caller's matrix.  Same bits as fresh handles give."""
    import pls_amd
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    A = 4
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        X = h.synth_x(0, N, K, 47, dtype=dtype); Y = h.synth_y(0, N, M, 47, dtype=dtype)
        for a in (A, A + 2, A - 1):
            got = {k: v.clone() for k, v in h.fit_device(X, Y, a).items()}; h.synchronize()
            with handle_with_env() as fresh:
                fresh.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
                ref = fresh.fit_device(X, Y, a); fresh.synchronize()
                for k in "WPQRTB":
                    assert torch.isfinite(ref[k]).all(), (a, k)
                    assert torch.equal(got[k], ref[k]), (a, k)


@pytest.mark.parametrize("A", [1, 2, 3, 7])
@pytest.mark.parametrize("N,K,dt,layout", [(4098, 512, "f64", 1), (3000, 96, "f32", 1), (4098, 512, "f64", 0)])
def test_profiler_books_one_sweep_for_the_last_pass(N, K, dt, layout, A):
    """OPT_PROFILE = 1: the byte count of the `fused` family after one NIPALS fit on the tall route.  Component 0 reads X,
    writes t_0 and reads v, writes the partial row (2 K doubles); a deflating component reads t_{a-1} and writes t_a, reads v
    and p_{a-1} and writes the partial row (3 K doubles) and sweeps X twice (read + write) -- except the last one, which
    only reads it."""
    import pls_amd
    torch = _torch()
    dtype = torch.float64 if dt == "f64" else torch.float32
    s = 8 if dt == "f64" else 4
    want = 0
    for a in range(A):
        sweeps = 1 if (a == 0 or a == A - 1) else 2
        want += sweeps * N * K * s + (1 if a == 0 else 2) * N * s + (2 if a == 0 else 3) * K * 8
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, pls_amd.ALGO_NIPALS)
        h.set_option(pls_amd.OPT_WORK_LAYOUT, layout)
        h.set_option(pls_amd.OPT_PROFILE, 1)
        X = h.synth_x(0, N, K, 53, dtype=dtype); Y = h.synth_y(0, N, 1, 53, dtype=dtype)
        h.timing()
        h.fit_device(X, Y, A); h.synchronize()
        tm = h.timing()
        assert tm["launches"]["fused"] == A
        assert tm["bytes"]["fused"] == want, (tm["bytes"]["fused"], want)
