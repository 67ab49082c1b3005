"""Every kernel route writes only inside its output matrices, and writes every element of them.

The parity tests read the rows x cols region of each output and nothing else: a store into the padding rows of an
aligned column, past the last column, or past K*A of W/P/R lands in memory no test looks at -- and behind the Eigen
drop-in (ld == rows, matrices next to each other on the caller's heap) it corrupts the caller's data.  An element the
kernel never stores can still hold the right value when the caching allocator hands back the block of an identical
earlier call.  Here every output is placed inside one flat buffer (`Guarded`): the cells around it hold a sentinel NaN,
the region itself a NaN of another payload.  Each case compares the region with a plain fp64 host reference, checks
every guard cell bit for bit, checks that no prefill is left, and checks that every input is bit-identical afterwards.

Two layouts: "aligned" (ld = rows rounded up to 16 bytes plus one 16-byte vector, 16-byte base: the vector / matrix-core
routes stay selected, ragged last tiles have padding rows to overrun into) and "eigen" (ld == rows, base one element
past a 16-byte boundary: the narrow routes).
"""
import ctypes

import numpy as np
import pytest

from conftest import handle_with_env
from test_gpu_parity import _fold_reference, check_against, oracle_ref

pytestmark = pytest.mark.gpu

# sentinel NaN of the guard cells / NaN the regions are prefilled with, by element size
SENTINEL = {8: 0x7FF4DEADBEEF0001, 4: 0x7FA5BEEF}
PREFILL = {8: 0x7FF4DEADBEEF0002, 4: 0x7FA5BEE2}
LEAD_BYTES = 64
TRAIL_BYTES = 4096

# the bars of the step entry points below, by name: tests/test_gpu_long_ld.py holds the same calls to them at long leading dimensions
XTY_BAR = 1e-13                        # of |X|^T |Y|, entry by entry
DEFLATE_BAR_F64 = 1e-15                # of |src| + |t p^T|, cell by cell (fp32 storage: one ulp of the rounded reference)
Z_BAR = {"f64": 1e-10, "f32": 5e-6}    # max |Z - Z_ref|
SSE_BAR = 1e-10                        # of the largest entry of the reference
CV_BAR = 1e-8                          # of max(max |E_ref|, 1)


def xb_bar(dt, K):
    """relative Frobenius error of X * Bm"""
    return 2e-7 if dt == "f32" else 1e-14 * max(1.0, (K / 2000.0) ** 0.5)


def _torch():
    import torch
    return torch


def _esize(dtype):
    """element size of a torch or numpy floating dtype"""
    if isinstance(dtype, np.dtype) or (isinstance(dtype, type) and issubclass(dtype, np.generic)):
        return np.dtype(dtype).itemsize
    return _torch().empty((), dtype=dtype).element_size()


class Guarded:
    """Column-major matrices inside ONE flat buffer, each between guard cells.

    specs: [(rows, cols)] or [(rows, cols, ld)]; layout "aligned" or "eigen" sets the default ld and the base alignment
    of every region.  Before each region: at least LEAD_BYTES of guard; after it: at least max(4 ld elements,
    TRAIL_BYTES), which is also the gap to the next region, so an overrun of one output into its neighbour is caught.
    device: "cuda" / "cpu" (torch tensors) or "numpy".  g[i] is the float view of region i (rows x cols, strides 1, ld),
    g.bits(i) the integer view of the same cells."""

    def __init__(self, specs, dtype, layout="aligned", device="cuda"):
        assert layout in ("aligned", "eigen")
        self.np = device == "numpy"
        es = _esize(dtype)
        self.es = es
        V = 16 // es
        self.specs, self.offs, self.lds = [], [], []
        pos = 0
        for s in specs:
            rows, cols = s[0], s[1]
            ld = s[2] if len(s) > 2 else (rows if layout == "eigen" else -(-rows // V) * V + V)
            assert ld >= max(rows, 1)
            pos += LEAD_BYTES // es
            pos = -(-pos // V) * V + (1 if layout == "eigen" else 0)
            self.specs.append((rows, cols)); self.offs.append(pos); self.lds.append(ld)
            pos += ld * cols
            pos += max(4 * ld, TRAIL_BYTES // es)
        total = pos + V
        if self.np:
            idt = np.int64 if es == 8 else np.int32
            self.raw = np.full(total, SENTINEL[es], dtype=idt)
            self.flat = self.raw.view(np.dtype(dtype))
            self.inside = np.zeros(total, dtype=bool)
        else:
            torch = _torch()
            idt = torch.int64 if es == 8 else torch.int32
            self.raw = torch.full((total,), SENTINEL[es], dtype=idt, device=device)
            self.flat = self.raw.view(dtype)
            self.inside = torch.zeros(total, dtype=torch.bool, device=device)
        for i in range(len(self.specs)):
            self._region(self.inside, i)[...] = True
        self.refill()

    def _region(self, a, i):
        (rows, cols), off, ld = self.specs[i], self.offs[i], self.lds[i]
        blk = a[off:off + ld * cols]
        blk = blk.reshape(cols, ld) if self.np else blk.view(cols, ld)
        return blk[:, :rows].T if self.np else blk[:, :rows].t()

    def __getitem__(self, i):
        return self._region(self.flat, i)

    def __len__(self):
        return len(self.specs)

    def bits(self, i):
        return self._region(self.raw, i)

    def ld(self, i):
        return self.lds[i]

    def ptr(self, i):
        """address of region i's first element (a ctypes void pointer)"""
        if self.np:
            return ctypes.c_void_p(self.raw.ctypes.data + self.offs[i] * self.es)
        return ctypes.c_void_p(self.raw.data_ptr() + self.offs[i] * self.es)

    def refill(self):
        """every region back to the prefill payload (the guard cells are never rewritten)"""
        self.raw[self.inside] = PREFILL[self.es]

    def _where(self, j):
        for i, ((rows, cols), off, ld) in enumerate(zip(self.specs, self.offs, self.lds)):
            if off - LEAD_BYTES // self.es - 16 <= j < off + ld * cols + max(4 * ld, TRAIL_BYTES // self.es):
                d = j - off
                return f"region {i} ({rows} x {cols}, ld {ld}): element offset {d} = row {d % ld}, column {d // ld}"
        return f"flat element {j}"

    def assert_untouched(self):
        """every guard cell still holds the sentinel, bit for bit"""
        bad = (self.raw != SENTINEL[self.es]) & ~self.inside
        if self.np:
            idx = np.flatnonzero(bad)
        else:
            idx = bad.nonzero().flatten().cpu().numpy()
        if idx.size:
            raise AssertionError(f"{idx.size} guard cells written; first at " +
                                 "; ".join(self._where(int(j)) for j in idx[:4]))

    def assert_written(self, i=None, cols=None):
        """no prefill payload left in region i (all regions if None), in its leading `cols` columns if given"""
        for k in (range(len(self)) if i is None else [i]):
            b = self.bits(k)[:, :cols] if cols is not None else self.bits(k)
            left = b == PREFILL[self.es]
            n = int(left.sum())
            if n:
                pos = np.argwhere(left) if self.np else left.nonzero().cpu().numpy()
                raise AssertionError(f"region {k}: {n} elements never written, first (row, column) {pos[:4].tolist()}")

    def assert_prefilled(self, i):
        """region i untouched as well (an output the call documents it leaves alone)"""
        b = self.bits(i)
        assert bool((b == PREFILL[self.es]).all()), f"region {i} was written"

    def check(self, cols=None):
        self.assert_untouched()
        self.assert_written(cols=cols)


def _bitsof(a):
    if isinstance(a, np.ndarray):
        return a.view(np.int64 if a.itemsize == 8 else np.int32).copy()
    torch = _torch()
    return a.view(torch.int64 if a.element_size() == 8 else torch.int32).clone()


class Inputs:
    """bit snapshots of the inputs of a call; .check() asserts they are unchanged"""

    def __init__(self, **named):
        self.named = named
        self.snap = {k: _bitsof(v) for k, v in named.items()}

    def check(self):
        for k, v in self.named.items():
            now = _bitsof(v)
            same = np.array_equal(now, self.snap[k]) if isinstance(now, np.ndarray) else bool((now == self.snap[k]).all())
            assert same, f"input {k} was modified"


def _place(a, dtype, layout, device="cuda"):
    """guarded copy of the numpy matrix a (an input): (Guarded, view)"""
    torch = _torch()
    g = Guarded([a.shape], dtype, layout, device)
    if g.np:
        g[0][...] = a
    else:
        g[0].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
    return g, g[0]


def _rows_sample(N, n=4096, seed=0):
    """rows for a value check of a large output: the first and last 200 and a random sample between"""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(min(200, N)), np.arange(max(0, N - 200), N), rng.integers(0, N, n)])
    return np.unique(idx)


@pytest.fixture(scope="module")
def gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _dt(name):
    torch = _torch()
    return torch.float64 if name == "f64" else torch.float32


def _code(tdt):
    from pls_amd import _lib as L
    return L.F64 if tdt == _torch().float64 else L.F32


# ------------------------------------------------------------------------------------------------------------------------
# X * Bm (pls_hip_xb): every kernel family of launch_xb
# ------------------------------------------------------------------------------------------------------------------------

# the call -> the steps xb_next (xb_route.hpp) plans for it on 256 CUs, as `kernel<selectors> (columns)`: tests/test_xb_route.py
# checks them on the CPU
XB_ROUTES = {
    # N, K, C, dt, X layout, out layout, PLS_HIP_XB4
    (600001, 16, 1, "f64", "aligned", "aligned", None): ["xb_kernel<2,1> (1)"],    # wide (>= 4 row groups per CU of 512 rows)
    (600001, 16, 2, "f64", "aligned", "aligned", None): ["xb_kernel<2,2> (2)"],
    (600001, 16, 3, "f64", "aligned", "aligned", None): ["xb_kernel<2,4> (3)"],
    (600001, 16, 3, "f64", "eigen", "eigen", None): ["xb_kernel<1,4> (3)"],        # narrow
    (1001, 37, 2, "f64", "eigen", "eigen", None): ["xb_kernel<1,2> (2)"],          # a short matrix
    (1048579, 8, 3, "f32", "aligned", "aligned", None): ["xb_kernel<4,4> (3)"],
    (4099, 30, 1, "f32", "eigen", "eigen", None): ["xb_kernel<1,1> (1)"],
    (512, 20000, 1, "f64", "aligned", "aligned", None): ["xb_split<1,1> + finish (1)"],   # too few row groups for 2 rows per lane
    (5000, 1200, 3, "f64", "aligned", "aligned", None): ["xb_split<2,4> + finish (3)"],
    # below 32 MB: not the MFMA split; the tile of 4 columns is fixed for the call
    (300, 9000, 6, "f64", "eigen", "eigen", None): ["xb_split<1,4> + finish (4)", "xb_split<1,4> + finish (2)"],
    (2100, 3000, 2, "f32", "eigen", "aligned", None): ["xb_split<1,2> + finish (2)"],
    (600001, 16, 7, "f64", "aligned", "aligned", None): ["xb_wide<2,8> (7)"],      # K < 128, 8 columns or fewer: no MFMA
    (1030, 37, 13, "f64", "eigen", "eigen", None): ["xb_wide<1,16> (13)"],
    (1048579, 8, 6, "f32", "aligned", "aligned", None): ["xb_wide<4,8> (6)"],
    (1048576 + 37, 16, 17, "f64", "aligned", "aligned", 0): ["xb_wide<2,20,2> (17)"],   # the two-pack form (PLS_HIP_XB4=0 only)
    (4099, 130, 45, "f64", "aligned", "aligned", None): ["xb_mfma_lds<2,3> (45)"],
    (2049, 515, 99, "f64", "aligned", "eigen", None): ["xb_mfma_lds<2,4> (64)", "xb_mfma_lds<2,3> (35)"],   # into an unaligned out
    (1030, 37, 42, "f32", "aligned", "aligned", None): ["xb_mfma_lds<4,2> (32)", "xb_mfma_lds<4,1> (10)"],
    (262144 + 37, 70, 21, "f64", "aligned", "aligned", None): ["xb_mfma4<2,6> (21)"],   # resident, partial last tile
    # 24 columns, then 2 on the NARROW xb_kernel: 512 row groups of 1,024 rows on 256 CUs are too few for 4 rows per lane
    (524288 + 5, 33, 26, "f32", "aligned", "aligned", None): ["xb_mfma4<4,6> (24)", "xb_kernel<1,2> (2)"],
    (262144 + 5, 128, 3, "f64", "aligned", "aligned", None): ["xb_mfma4<2,1> (3)"],     # the 1-4 column "few" form
    (40001, 200, 19, "f64", "aligned", "aligned", None): ["xb_mfma4w<2,5> (19)"],       # too few tiles for the resident form
    (70000 + 3, 130, 18, "f32", "aligned", "aligned", None): ["xb_mfma4w<4,5> (18)"],
    (2000, 5000, 21, "f64", "aligned", "aligned", None): ["xb_mfma4w<2,6> split y=7 + finish (21)"],   # split over blockIdx.y
    (1001, 9001, 5, "f64", "aligned", "eigen", None): ["xb_mfma4w<2,2> split y=3 + finish (5)"],   # the finish into an unaligned out
    (515, 20000, 6, "f32", "aligned", "aligned", None): ["xb_mfma4w<4,2> split y=7 + finish (6)"],
}
XB_CASES = list(XB_ROUTES)


@pytest.mark.parametrize("N,K,C,dt,xl,ol,xb4", XB_CASES)
def test_xb_writes_exactly_its_output(gpu, N, K, C, dt, xl, ol, xb4):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    env = {} if xb4 is None else {"PLS_HIP_XB4": xb4}
    with handle_with_env(**env) as h:
        gx = Guarded([(N, K)], tdt, xl)
        X = gx[0]
        assert L.lib().pls_hip_synth_x(h.h, gx.ptr(0), gx.ld(0), 0, N, K, 41, _code(tdt)) == 0
        gb = Guarded([(K, C)], torch.float64, "aligned")
        g = torch.Generator(device="cpu"); g.manual_seed(N + K + C)
        Bh = torch.randn(K, C, generator=g, dtype=torch.float64).numpy()
        gb[0].copy_(torch.from_numpy(Bh))
        h.synchronize()
        ins = Inputs(X=X, Bm=gb[0])
        go = Guarded([(N, C)], tdt, ol)
        rc = L.lib().pls_hip_xb(h.h, gx.ptr(0), gx.ld(0), N, K, gb.ptr(0), gb.ld(0), C, _code(tdt), L.MEM_DEVICE,
                                go.ptr(0), go.ld(0))
        L.check(rc, h.h)
        h.synchronize()
    go.check()
    gx.assert_untouched(); gb.assert_untouched()
    ins.check()
    rows = _rows_sample(N) if N * K > 1 << 22 else np.arange(N)
    ri = torch.from_numpy(rows).cuda()
    ref = X[ri].cpu().numpy().astype(np.float64) @ Bh
    got = go[0][ri].cpu().numpy().astype(np.float64)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert err < xb_bar(dt, K), err


# ------------------------------------------------------------------------------------------------------------------------
# dst = src - t p^T (pls_hip_deflate)
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,dt,layout,inplace", [
    (1001, 37, "f64", "aligned", False),    # deflate_piece_kernel<double, 2>
    (1001, 37, "f32", "aligned", True),     # deflate_piece_kernel<float, 4>, in place
    (4099, 20, "f32", "aligned", False),
    (64, 70000, "f64", "aligned", False),   # K > 65,535: deflate_kernel<double, 2>
    (64, 70000, "f64", "aligned", True),
    (1001, 37, "f64", "eigen", False),      # deflate_kernel<double, 1>
    (2051, 33, "f32", "eigen", True),       # deflate_kernel<float, 1>, in place
])
def test_deflate_writes_exactly_dst(gpu, N, K, dt, layout, inplace):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    npdt = np.float64 if dt == "f64" else np.float32
    rng = np.random.default_rng(N + K)
    src_h = rng.standard_normal((N, K)).astype(npdt)
    t_h = rng.standard_normal(N).astype(npdt)
    p_h = rng.standard_normal(K)
    gs, src = _place(src_h, tdt, layout)
    gt = Guarded([(N, 1)], tdt, "aligned"); gt[0].copy_(torch.from_numpy(t_h[:, None]))
    gp = Guarded([(K, 1)], torch.float64, layout); gp[0].copy_(torch.from_numpy(p_h[:, None]))
    ins = Inputs(t=gt[0], p=gp[0]) if inplace else Inputs(src=src, t=gt[0], p=gp[0])
    gd = gs if inplace else Guarded([(N, K)], tdt, layout)
    with handle_with_env() as h:
        rc = L.lib().pls_hip_deflate(h.h, gs.ptr(0), gs.ld(0), gd.ptr(0), gd.ld(0), N, K, gt.ptr(0), gp.ptr(0), _code(tdt))
        L.check(rc, h.h)
        h.synchronize()
    gd.check()
    gs.assert_untouched(); gt.assert_untouched(); gp.assert_untouched()
    ins.check()
    s64, t64 = src_h.astype(np.float64), t_h.astype(np.float64)
    ref = s64 - np.outer(t64, p_h)
    got = gd[0].cpu().numpy()
    if dt == "f64":
        assert (np.abs(got - ref) <= DEFLATE_BAR_F64 * (np.abs(s64) + np.abs(np.outer(t64, p_h)))).all()
    else:
        r32 = ref.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - r32) <= np.spacing(np.abs(r32))).all()


# ------------------------------------------------------------------------------------------------------------------------
# XY = X^T Y (pls_hip_xty), ld K
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,M,dt,layout", [
    (4099, 300, 1, "f64", "aligned"),   # retile_xty_kernel (K >= 256, M in 1, 2, 4, 8)
    (4099, 300, 4, "f32", "aligned"),
    (4099, 300, 8, "f64", "aligned"),
    (4099, 128, 8, "f64", "aligned"),   # xty8_kernel
    (4099, 128, 9, "f32", "aligned"),   # xty8_kernel + xty_kernel<., 32, 1>
    (4099, 130, 9, "f64", "aligned"),   # xty_kernel<2, 4, 8> + <2, 32, 1>: two m-tiles
    (1001, 37, 5, "f64", "aligned"),    # xty_kernel<2, 8, 4> + <2, 32, 1>
    (1001, 37, 3, "f64", "eigen"),      # narrow: xty_kernel<1, 16, 2> + <1, 32, 1>
    (2051, 300, 9, "f32", "eigen"),
])
def test_xty_writes_exactly_xy(gpu, N, K, M, dt, layout):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    npdt = np.float64 if dt == "f64" else np.float32
    rng = np.random.default_rng(N * M + K)
    Xh = rng.standard_normal((N, K)).astype(npdt); Yh = rng.standard_normal((N, M)).astype(npdt)
    gx, X = _place(Xh, tdt, layout)
    gy, Y = _place(Yh, tdt, layout)
    ins = Inputs(X=X, Y=Y)
    go = Guarded([(K, M, K)], torch.float64, layout)
    with handle_with_env() as h:
        L.check(L.lib().pls_hip_xty(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, _code(tdt), go.ptr(0)), h.h)
        h.synchronize()
    go.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    X64, Y64 = Xh.astype(np.float64), Yh.astype(np.float64)
    ref = X64.T @ Y64
    scale = np.abs(X64).T @ np.abs(Y64)
    assert (np.abs(go[0].cpu().numpy() - ref) <= XTY_BAR * scale).all()


# ------------------------------------------------------------------------------------------------------------------------
# pls_hip_fit on device memory: T (ldt) and W, P, Q, R, B (ld = rows) in one flat buffer
# ------------------------------------------------------------------------------------------------------------------------

FIT_CASES = [
    # id, N, K, M, A, dt, layout, handle environment, options
    ("kernel-fused", 4099, 400, 2, 6, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {}),
    ("kernel-fused-edge", 1001, 37, 2, 6, "f64", "eigen", {"PLS_HIP_RESIDENT": 0, "PLS_HIP_TINY": 0}, {}),
    ("kernel-unfused", 1001, 37, 3, 5, "f64", "eigen", {"PLS_HIP_RESIDENT": 0, "PLS_HIP_TINY": 0}, {"FUSE": 0}),
    ("nipals-tiles", 2050, 120, 4, 8, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 1}),
    ("nipals-colmajor", 2050, 120, 4, 8, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 1, "WORK_LAYOUT": 0}),
    ("nipals-unfused", 1001, 37, 2, 5, "f64", "eigen", {"PLS_HIP_RESIDENT": 0, "PLS_HIP_TINY": 0}, {"ALGO": 1, "FUSE": 0}),
    # (the deferred write-back: 256 < K <= 512, N a multiple of the row pack, 16-byte columns of X and T)
    ("defer2", 4098, 300, 3, 7, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 1, "DEFER": 2}),
    ("defer3", 3000, 400, 2, 6, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 1, "DEFER": 3}),
    ("defer4", 4098, 512, 1, 7, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 1, "DEFER": 4}),
    ("gram", 3001, 64, 2, 6, "f64", "eigen", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 2}),
    ("gram-f32", 5004, 200, 3, 5, "f32", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 2}),
    # (16-byte columns, N ragged for either row pack: the register-staged X^T X -- a diagonal block, an off-diagonal block with
    # its mirror, a ragged second diagonal block; three column blocks in fp32)
    ("gram-ragged-rows", 2051, 130, 2, 5, "f64", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 2}),
    ("gram-ragged-rows-f32", 2051, 300, 2, 5, "f32", "aligned", {"PLS_HIP_RESIDENT": 0}, {"ALGO": 2}),
    ("resident", 5000, 128, 1, 10, "f64", "aligned", {}, {}),
    ("resident-m5-f32", 3001, 77, 5, 7, "f32", "eigen", {}, {}),
    ("resident-gram", 5003, 128, 1, 11, "f64", "eigen", {}, {"ALGO": 3}),
    ("resident-gram-m2", 2000, 120, 2, 6, "f64", "aligned", {}, {"ALGO": 3}),
    ("tiny", 130, 100, 1, 7, "f64", "eigen", {}, {}),
    ("tiny-f32", 1000, 20, 1, 6, "f32", "aligned", {}, {}),
    ("tiny-m3", 130, 100, 3, 7, "f64", "aligned", {}, {}),
    ("tiny-m8", 700, 26, 8, 4, "f64", "eigen", {}, {}),
    ("micro", 60, 40, 4, 6, "f64", "eigen", {}, {}),
    ("coop", 300, 2048, 8, 6, "f64", "aligned", {}, {}),                 # coop_update_kernel: K M >= 16,384
    ("coop-ragged", 260, 8200, 2, 5, "f64", "eigen", {}, {"ALGO": 1}),   # ... ragged last workgroup
    ("wide-m1", 260, 4500, 1, 4, "f64", "aligned", {}, {}),              # wide1_*_kernel: one response, K > 4096
    ("wide-m2", 100, 17000, 2, 3, "f64", "eigen", {}, {}),               # widem_*_kernel: beyond the cooperative kernel
    ("m33", 300, 40, 33, 4, "f64", "eigen", {}, {}),
    ("f32-kernel", 2051, 300, 2, 5, "f32", "eigen", {"PLS_HIP_RESIDENT": 0}, {}),
    ("f32-nipals", 1001, 37, 2, 6, "f32", "aligned", {"PLS_HIP_RESIDENT": 0, "PLS_HIP_TINY": 0}, {"ALGO": 1}),
]


def _set_opts(h, opts):
    import pls_amd
    for k, v in opts.items():
        h.set_option(getattr(pls_amd, "OPT_" + k), v)


def _fit_buffers(N, K, M, A, tdt, layout, ldt=None):
    torch = _torch()
    gt = Guarded([(N, A) if ldt is None else (N, A, ldt)], tdt, layout)
    gw = Guarded([(K, A, K), (K, A, K), (M, A, M), (K, A, K), (K, M, K)], torch.float64, layout)
    return gt, gw


def _fit_out(gt, gw):
    out = {k: gw[i] for i, k in enumerate("WPQRB")}
    out["T"] = gt[0]
    return out


def _tols(dt):
    if dt == "f32":
        return dict(tol_b=2e-5, tol_col=2e-4, tol_inv=1e-3)
    return dict(tol_b=1e-10, tol_col=1e-9, tol_inv=1e-7)


def _synth_inputs(oracle, N, K, M, dt, layout):
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    if dt == "f32":
        Xh = np.asfortranarray(Xh.astype(np.float32).astype(np.float64)); Yh = np.asfortranarray(Yh.astype(np.float32).astype(np.float64))
    tdt = _dt(dt)
    gx, X = _place(Xh, tdt, layout)
    gy, Y = _place(Yh, tdt, layout)
    return Xh, Yh, gx, X, gy, Y


@pytest.mark.parametrize("name,N,K,M,A,dt,layout,env,opts", FIT_CASES, ids=[c[0] for c in FIT_CASES])
def test_fit_device_writes_exactly_its_outputs(gpu, oracle, po, name, N, K, M, A, dt, layout, env, opts):
    tdt = _dt(dt)
    Xh, Yh, gx, X, gy, Y = _synth_inputs(oracle, N, K, M, dt, layout)
    ins = Inputs(X=X, Y=Y)
    gt, gw = _fit_buffers(N, K, M, A, tdt, layout)
    with handle_with_env(**env) as h:
        _set_opts(h, opts)
        h.fit_device(X, Y, A, out=_fit_out(gt, gw)); h.synchronize()
    gt.check(); gw.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    check_against(po, _fit_out(gt, gw), ref, Bref, ref["T"], col_err=cerr, **_tols(dt))


def test_kernel_type2_leaves_t_alone(gpu, oracle, po):
    """KERNEL_TYPE2 does not compute T: a T buffer passed anyway keeps its prefill, bit for bit"""
    import pls_amd
    N, K, M, A = 1500, 70, 2, 5
    Xh, Yh, gx, X, gy, Y = _synth_inputs(oracle, N, K, M, "f64", "aligned")
    ins = Inputs(X=X, Y=Y)
    gt, gw = _fit_buffers(N, K, M, A, _torch().float64, "aligned")
    with handle_with_env() as h:
        h.fit_device(X, Y, A, method=pls_amd.KERNEL_TYPE2, out=_fit_out(gt, gw)); h.synchronize()
    gt.assert_untouched(); gt.assert_prefilled(0)
    gw.check()
    ins.check()
    ref = oracle.plsr(Xh, Yh, A, method=1)
    assert po.rel_fro(gw[4].cpu().numpy(), oracle.coefficients(ref["R"], ref["Q"])) < 1e-10


def test_graph_replay_writes_exactly_its_outputs(gpu, oracle, po):
    """OPT_GRAPH: three fits on the same pointers on a stream of its own (eager, captured, replayed); the outputs are
    prefilled again before the replay, which must write every element and nothing else"""
    import pls_amd
    torch = _torch()
    N, K, M, A = 3000, 96, 2, 5
    Xh, Yh, gx, X, gy, Y = _synth_inputs(oracle, N, K, M, "f64", "aligned")
    ins = Inputs(X=X, Y=Y)
    gt, gw = _fit_buffers(N, K, M, A, torch.float64, "aligned")
    ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side), handle_with_env(PLS_HIP_RESIDENT=0) as h:
        for algo in (pls_amd.ALGO_KERNEL, pls_amd.ALGO_NIPALS):
            h.set_option(pls_amd.OPT_ALGO, algo)
            h.set_option(pls_amd.OPT_GRAPH, 1)
            for rep in range(3):
                gt.refill(); gw.refill()
                h.fit_device(X, Y, A, out=_fit_out(gt, gw)); side.synchronize()
                gt.check(); gw.check()
                check_against(po, _fit_out(gt, gw), ref, Bref, ref["T"], col_err=cerr)
            h.set_option(pls_amd.OPT_GRAPH, 0)
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()


# ------------------------------------------------------------------------------------------------------------------------
# pls_hip_fit on host memory: interior pointers of guarded numpy arrays
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,M,A,dt,layout,algo", [
    (1001, 37, 2, 6, "f64", "eigen", 0),      # ldt == N
    (1001, 37, 2, 6, "f32", "aligned", 0),    # ldt > N
    (2051, 300, 1, 5, "f32", "eigen", 1),
    (90000, 200, 1, 8, "f64", "aligned", 3),  # AUTO: X^T X accumulated while X crosses PCIe, then T = X R
    (90001, 200, 3, 5, "f32", "eigen", 3),    # (no 16-byte columns: plain upload)
])
def test_fit_host_writes_exactly_its_outputs(gpu, oracle, po, N, K, M, A, dt, layout, algo):
    import pls_amd
    from pls_amd import _lib as L
    npdt = np.float64 if dt == "f64" else np.float32
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    Xh = Xh.astype(npdt).astype(np.float64); Yh = Yh.astype(npdt).astype(np.float64)
    gx, X = _place(Xh, npdt, layout, "numpy")
    gy, Y = _place(Yh, npdt, layout, "numpy")
    ins = Inputs(X=X, Y=Y)
    gt = Guarded([(N, A)], npdt, layout, "numpy")
    gw = Guarded([(K, A, K), (K, A, K), (M, A, M), (K, A, K), (K, M, K)], np.float64, layout, "numpy")
    with handle_with_env() as h:
        h.set_option(pls_amd.OPT_ALGO, algo)
        rc = L.lib().pls_hip_fit(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A, L.KERNEL_TYPE1,
                                 L.F64 if dt == "f64" else L.F32, L.MEM_HOST, gw.ptr(0), gw.ptr(1), gw.ptr(2), gw.ptr(3),
                                 gt.ptr(0), gt.ld(0), gw.ptr(4))
        L.check(rc, h.h)
    gt.check(); gw.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    torch = _torch()
    out = {k: torch.from_numpy(gw[i]) for i, k in enumerate("WPQRB")}
    out["T"] = torch.from_numpy(gt[0])
    if N * K > 1 << 22:
        ref = oracle.plsr(Xh, Yh, A)
        Bref = oracle.coefficients(ref["R"], ref["Q"])
        assert po.rel_fro(gw[4], Bref) < (1e-10 if dt == "f64" else 2e-5)
        rows = _rows_sample(N)
        assert po.rel_fro(gt[0][rows].astype(np.float64), Xh[rows] @ gw[3]) < (1e-11 if dt == "f64" else 1e-6)
    else:
        ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
        check_against(po, out, ref, Bref, ref["T"], col_err=cerr, **_tols(dt))


# ------------------------------------------------------------------------------------------------------------------------
# B = R[:, :c] Q[:, :c]^T (pls_hip_coefficients)
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("c", [0, 3, 6])
def test_coefficients_write_exactly_b(gpu, mem, c):
    from pls_amd import _lib as L
    torch = _torch()
    K, M, A = 301, 3, 6
    rng = np.random.default_rng(c)
    Rh = rng.standard_normal((K, A)); Qh = rng.standard_normal((M, A))
    dev = "numpy" if mem == "host" else "cuda"
    layout = "eigen" if c == 3 else "aligned"
    gi = Guarded([(K, A, K), (M, A, M)], np.float64 if dev == "numpy" else torch.float64, layout, dev)
    if dev == "numpy":
        gi[0][...] = Rh; gi[1][...] = Qh
    else:
        gi[0].copy_(torch.from_numpy(Rh)); gi[1].copy_(torch.from_numpy(Qh))
    ins = Inputs(R=gi[0], Q=gi[1])
    gb = Guarded([(K, M, K)], np.float64 if dev == "numpy" else torch.float64, layout, dev)
    with handle_with_env() as h:
        rc = L.lib().pls_hip_coefficients(h.h, gi.ptr(0), gi.ptr(1), K, M, A, c,
                                          L.MEM_HOST if mem == "host" else L.MEM_DEVICE, gb.ptr(0))
        L.check(rc, h.h)
        h.synchronize()
    gb.check(); gi.assert_untouched()
    ins.check()
    B = gb[0] if dev == "numpy" else gb[0].cpu().numpy()
    if c == 0:
        assert (B == 0.0).all() and not np.signbit(B).any()
    else:
        ref = Rh[:, :c] @ Qh[:, :c].T
        assert (np.abs(B - ref) <= 1e-14 * (np.abs(Rh[:, :c]) @ np.abs(Qh[:, :c]).T)).all()


# ------------------------------------------------------------------------------------------------------------------------
# column z-scores (pls_hip_colwise_z_scores): Z out of place, mean and sd in one flat buffer
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,dt,layout,want_z", [
    (1001, 37, "f64", "aligned", True),     # zscale_piece_kernel
    (4099, 20, "f32", "aligned", True),
    (1001, 37, "f64", "eigen", True),       # zscale_kernel<., 1, .>
    (2051, 33, "f32", "eigen", True),
    (70001, 17, "f64", "eigen", False),     # Z == NULL: the statistics only
])
def test_z_scores_write_exactly_z_mean_sd(gpu, oracle, N, K, dt, layout, want_z):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    rng = np.random.default_rng(N * 7 + K)
    Xh = oracle.synth_x(0, N, K) * rng.uniform(0.1, 30, K) + rng.uniform(-50, 50, K)
    if dt == "f32":
        Xh = Xh.astype(np.float32).astype(np.float64)
    gx, X = _place(Xh, tdt, layout)
    ins = Inputs(X=X)
    gz = Guarded([(N, K)], tdt, layout)
    gs = Guarded([(K, 1), (K, 1)], torch.float64, layout)
    with handle_with_env() as h:
        rc = L.lib().pls_hip_colwise_z_scores(h.h, gx.ptr(0), gx.ld(0), N, N, K, _code(tdt),
                                              gz.ptr(0) if want_z else None, gz.ld(0), gs.ptr(0), gs.ptr(1))
        L.check(rc, h.h)
        h.synchronize()
    gs.check()
    gz.assert_untouched()
    if want_z:
        gz.assert_written()
    else:
        gz.assert_prefilled(0)
    gx.assert_untouched()
    ins.check()
    xl = Xh.astype(np.longdouble)
    mr = xl.mean(0); sr = np.sqrt(((xl - mr) ** 2).sum(0) / (N - 1))
    assert np.allclose(gs[0].cpu().numpy()[:, 0], mr.astype(np.float64), rtol=1e-13, atol=1e-13)
    assert np.allclose(gs[1].cpu().numpy()[:, 0], sr.astype(np.float64), rtol=1e-12)
    if want_z:
        zr = ((xl - mr) / sr).astype(np.float64)
        assert np.abs(gz[0].cpu().numpy().astype(np.float64) - zr).max() < Z_BAR[dt]


# ------------------------------------------------------------------------------------------------------------------------
# SSE for every component count (pls_hip_sse_by_components, pls_hip_model_sse), ld M
# ------------------------------------------------------------------------------------------------------------------------

def _sse_reference(S, Y, Q):
    res = Y.astype(np.float64).copy()
    out = np.zeros((Y.shape[1], S.shape[1]))
    for c in range(S.shape[1]):
        res -= np.outer(S[:, c], Q[:, c])
        out[:, c] = (res ** 2).sum(0)
    return out


@pytest.mark.parametrize("N,A,M,dt,layout", [
    (2000, 400, 3, "f64", "aligned"),   # 341 component counts per range: two ranges
    (1001, 700, 2, "f32", "eigen"),     # 512 per range
])
def test_sse_by_components_writes_exactly_sse(gpu, N, A, M, dt, layout):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    npdt = np.float64 if dt == "f64" else np.float32
    rng = np.random.default_rng(A + M)
    Sh = (rng.standard_normal((N, A)) / np.sqrt(A)).astype(npdt)
    Yh = rng.standard_normal((N, M)).astype(npdt)
    Qh = rng.standard_normal((M, A))
    gsx, S = _place(Sh, tdt, layout)
    gy, Y = _place(Yh, tdt, layout)
    gq = Guarded([(M, A, M)], torch.float64, layout); gq[0].copy_(torch.from_numpy(Qh))
    ins = Inputs(S=S, Y=Y, Q=gq[0])
    go = Guarded([(M, A, M)], torch.float64, layout)
    with handle_with_env() as h:
        rc = L.lib().pls_hip_sse_by_components(h.h, gsx.ptr(0), gsx.ld(0), gy.ptr(0), gy.ld(0), N, A, M, gq.ptr(0),
                                               _code(tdt), go.ptr(0))
        L.check(rc, h.h)
        h.synchronize()
    go.check()
    gsx.assert_untouched(); gy.assert_untouched(); gq.assert_untouched()
    ins.check()
    ref = _sse_reference(Sh.astype(np.float64), Yh, Qh)
    assert np.abs(go[0].cpu().numpy() - ref).max() < SSE_BAR * np.abs(ref).max()


@pytest.mark.parametrize("mem", ["device", "host"])
def test_model_sse_writes_exactly_sse(gpu, oracle, mem):
    from pls_amd import _lib as L
    torch = _torch()
    N, K, M, A = 3001, 50, 3, 400
    rng = np.random.default_rng(9)
    Xh = oracle.synth_x(0, N, K); Yh = oracle.synth_y(0, N, M)
    Rh = rng.standard_normal((K, A)) / K; Qh = rng.standard_normal((M, A))
    dev = "numpy" if mem == "host" else "cuda"
    fdt = np.float64 if dev == "numpy" else torch.float64
    layout = "eigen" if mem == "host" else "aligned"
    gx, X = _place(Xh, fdt, layout, dev)
    gy, Y = _place(Yh, fdt, layout, dev)
    gm = Guarded([(K, A, K), (M, A, M)], fdt, layout, dev)
    if dev == "numpy":
        gm[0][...] = Rh; gm[1][...] = Qh
    else:
        gm[0].copy_(torch.from_numpy(Rh)); gm[1].copy_(torch.from_numpy(Qh))
    ins = Inputs(X=X, Y=Y, R=gm[0], Q=gm[1])
    go = Guarded([(M, A, M)], fdt, layout, dev)
    with handle_with_env() as h:
        rc = L.lib().pls_hip_model_sse(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A, gm.ptr(0), gm.ptr(1),
                                       L.F64, L.MEM_HOST if mem == "host" else L.MEM_DEVICE, go.ptr(0))
        L.check(rc, h.h)
        h.synchronize()
    go.check()
    gx.assert_untouched(); gy.assert_untouched(); gm.assert_untouched()
    ins.check()
    ref = _sse_reference(Xh @ Rh, Yh, Qh)
    got = go[0] if dev == "numpy" else go[0].cpu().numpy()
    assert np.abs(got - ref).max() < SSE_BAR * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------------------------------
# cross-validation folds (pls_hip_cv_folds): E, M matrices of nobs x A, held as one nobs x (M A) matrix
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,K,M,A,ts,nf,env,mem", [
    ("batched", 1500, 40, 2, 4, 25, 9, {}, "device"),          # cv_folds_kernel (X^T X downdates)
    ("batched-host", 1500, 40, 2, 4, 25, 9, {}, "host"),
    ("tiny-per-fold", 300, 24, 1, 5, 30, 6, {}, "device"),     # tiny_fit_kernel, one workgroup per fold
    ("tiny-m", 200, 24, 3, 5, 20, 7, {}, "device"),            # tiny_fit_m_kernel folds
    ("micro", 60, 24, 1, 6, 1, 60, {}, "host"),                # micro_fit_kernel folds (leave one out)
    ("refit", 301, 33, 2, 4, 17, 5, {"PLS_HIP_CV_REFIT": 1}, "device"),
    ("refit-m40", 150, 50, 40, 3, 30, 4, {}, "device"),        # M > 32: one refit per fold
])
def test_cv_folds_write_exactly_e(gpu, oracle, name, N, K, M, A, ts, nf, env, mem):
    from pls_amd import _lib as L
    torch = _torch()
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    rng = np.random.default_rng(N + nf)
    idx = np.arange(N)[:, None] if ts == 1 and nf == N else np.stack([rng.permutation(N)[:ts] for _ in range(nf)])
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    nobs = nf * ts
    dev = "numpy" if mem == "host" else "cuda"
    fdt = np.float64 if dev == "numpy" else torch.float64
    layout = "eigen" if name in ("batched-host", "tiny-m") else "aligned"
    gx, X = _place(Xh, fdt, layout, dev)
    gy, Y = _place(Yh, fdt, layout, dev)
    ins = Inputs(X=X, Y=Y, test_idx=idx)
    ge = Guarded([(nobs, M * A, nobs)], fdt, layout, dev)
    with handle_with_env(**env) as h:
        rc = L.lib().pls_hip_cv_folds(h.h, gx.ptr(0), gx.ld(0), gy.ptr(0), gy.ld(0), N, K, M, A,
                                      idx.ctypes.data_as(ctypes.c_void_p), ts, nf, L.F64,
                                      L.MEM_HOST if mem == "host" else L.MEM_DEVICE, ge.ptr(0))
        L.check(rc, h.h)
        h.synchronize()
    ge.check()
    gx.assert_untouched(); gy.assert_untouched()
    ins.check()
    ref = _fold_reference(oracle, Xh, Yh, A, idx)                 # (M, nobs, A)
    want = ref.transpose(1, 0, 2).reshape(nobs, M * A)            # E[m (nobs A) + i + c nobs] = column m A + c, row i
    got = ge[0] if dev == "numpy" else ge[0].cpu().numpy()
    assert np.abs(got - want).max() < CV_BAR * max(np.abs(ref).max(), 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# synthetic inputs (pls_hip_synth_x / _y) into row blocks of a padded matrix
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,row0,n,cols,dt,layout", [
    ("x", 777, 1001, 37, "f64", "aligned"), ("x", 5, 4099, 20, "f32", "eigen"),
    ("y", 1000, 3001, 3, "f64", "eigen"), ("y", 64, 515, 2, "f32", "aligned"),
])
def test_synth_writes_exactly_its_rows(gpu, which, row0, n, cols, dt, layout):
    from pls_amd import _lib as L
    torch = _torch()
    tdt = _dt(dt)
    g = Guarded([(n, cols)], tdt, layout)
    with handle_with_env() as h:
        fn = L.lib().pls_hip_synth_x if which == "x" else L.lib().pls_hip_synth_y
        L.check(fn(h.h, g.ptr(0), g.ld(0), row0, n, cols, 99, _code(tdt)), h.h)
        whole = (h.synth_x if which == "x" else h.synth_y)(0, row0 + n, cols, 99, dtype=tdt)
        h.synchronize()
    g.check()
    assert torch.equal(_bitsof(g[0]), _bitsof(whole[row0:]))


# ------------------------------------------------------------------------------------------------------------------------
# a group of two members on one GPU (host-synchronised exchange): host W/P/Q/R/B of a fit, a download into ld > N
# ------------------------------------------------------------------------------------------------------------------------

def test_group_fit_and_download_write_exactly_their_outputs(gpu, oracle, po):
    import pls_amd
    from pls_amd import _lib as L
    torch = _torch()
    N, K, M, A = 3001, 64, 2, 6
    Xh, Yh = oracle.synth_x(0, N, K), oracle.synth_y(0, N, M)
    g = pls_amd.Group([0, 0])
    try:
        assert g.exchange == "host"
        mx, my = g.upload(Xh), g.upload(Yh)
        T = g.alloc(N, A)
        gw = Guarded([(K, A, K), (K, A, K), (M, A, M), (K, A, K), (K, M, K)], np.float64, "eigen", "numpy")
        g._check(L.lib().pls_hip_group_fit(g.g, mx, my, A, L.KERNEL_TYPE1, gw.ptr(0), gw.ptr(1), gw.ptr(2), gw.ptr(3), T,
                                           gw.ptr(4)))
        gw.check()
        col0, ncols = 2, A - 3
        gd = Guarded([(N, ncols, N + 5)], np.float64, "aligned", "numpy")
        g._check(L.lib().pls_hip_group_download(g.g, T, col0, ncols, gd.ptr(0), gd.ld(0)))
        gd.check()
        ref, Bref, cerr = oracle_ref(oracle, po, Xh, Yh, A)
        out = {k: torch.from_numpy(gw[i]) for i, k in enumerate("WPQRB")}
        check_against(po, out, ref, Bref, None, col_err=cerr)
        Tref = Xh @ gw[3][:, col0:col0 + ncols]
        assert po.rel_fro(gd[0], Tref) < 1e-11
        g.free(T); g.free(mx); g.free(my)
    finally:
        g.close()
