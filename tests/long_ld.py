"""Matrices with LONG leading dimensions for the GPU tests: a few thousand rows, the columns tens or hundreds of MiB apart.

The header promises "any ld >= N" for every matrix argument, and the library is full of decisions that depend only on how far
apart two columns are (one 32-bit buffer descriptor per group of columns, per wave, or none: fit_route.hpp, xb_route.hpp, the
span checks of the launchers).  A kernel touches N rows of each column, so a test needs no 2^24-row data to reach them: the
matrix stays small, only its columns lie far apart inside ONE flat device allocation, the `Arena`.

  arena.begin(dtype, fill)                 every cell of the arena <- the gap pattern; no regions
  arena.place(a, dtype, ld, base_off)      an INPUT: the (rows, cols) view with strides (1, ld) holding the numpy matrix a
  arena.out(rows, cols, dtype, ld, base_off)   an OUTPUT: such a view over cells of a second pattern (the prefill)
  arena.check()                            after the call, with counting passes over the arena (no clone of it):
                                             every input is bit-identical to what was placed,
                                             exactly the rows x cols cells of the regions differ from the gap pattern,
                                             no cell holds the prefill any more.

Regions may share the pitch: X, Y and T with the same ld at different row windows (base_off) interleave their columns, so "all
arguments long at once" costs the memory of the widest matrix alone.

The gap pattern: a NaN of a payload no kernel produces for entry points on complete data -- a stray read poisons the result --
and a huge finite value (1e300; 3e38 in fp32, as test_gpu_missing_cv.Packed) for the missing-value entry points, where NaN
means "missing" and a stray read would be skipped silently.

No test may hold more than CAP_BYTES of device memory through torch, arena and the temporaries of the checks included:
asserted here, at construction and after every check.
"""
import numpy as np

CAP_BYTES = 20 << 30
# bit patterns by element size: the gap between the regions, the cells of an output region before the call
GAP_NAN = {8: 0x7FF4DEADBEEF0001, 4: 0x7FA5BEEF}
PREFILL = {8: 0x7FF4DEADBEEF0002, 4: 0x7FA5BEE2}
HUGE = {8: 1e300, 4: 3e38}
CHUNK = 1 << 27   # elements per counting pass: the comparison's temporary (one byte per element) stays at 128 MiB


def _torch():
    import torch
    return torch


def _signed(bits, es):
    return bits - (1 << (8 * es)) if bits >= 1 << (8 * es - 1) else bits


def gap_bits(fill, es):
    """the integer image of the gap pattern `fill` ("nan" or "huge") at element size es"""
    if fill == "nan":
        return GAP_NAN[es]
    assert fill == "huge", fill
    return int(np.array([HUGE[es]], dtype=np.float64 if es == 8 else np.float32).view(np.int64 if es == 8 else np.int32)[0])


class Arena:
    def __init__(self, nbytes, device="cuda"):
        torch = _torch()
        self.cuda = device == "cuda"   # (a CPU arena: the helper's own tests)
        assert nbytes % 16 == 0
        # (a counting pass holds one chunk's comparison and the library its workspaces: a few hundred MiB on top)
        assert nbytes + (1 << 30) <= CAP_BYTES, f"an arena of {nbytes} bytes leaves no room under the cap of {CAP_BYTES}"
        self.nbytes = nbytes
        self.raw = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        assert self.raw.data_ptr() % 16 == 0
        self.regions = []
        self.es = None

    def release(self):
        self.raw = None
        self.regions = []
        if self.cuda:
            _torch().cuda.empty_cache()

    # ---- layout ----------------------------------------------------------------------------------------------------------------
    def _ints(self):
        torch = _torch()
        return self.raw if self.es == 8 else self.raw.view(torch.int32)

    def begin(self, dtype, fill="nan"):
        torch = _torch()
        self.dtype = dtype
        self.es = torch.empty((), dtype=dtype).element_size()
        self.gap = gap_bits(fill, self.es)
        g = self.gap if self.es == 8 else (self.gap << 32) | self.gap
        self.raw.fill_(_signed(g, 8))
        self.regions = []
        if self.cuda:
            torch.cuda.reset_peak_memory_stats()

    def _claim(self, kind, rows, cols, ld, off, host):
        V = 16 // self.es
        assert rows >= 1 and cols >= 1 and ld >= rows and off >= 0
        assert off + (cols - 1) * ld + rows <= self.nbytes // self.es, \
            f"{rows} x {cols} at ld {ld}, offset {off}: {(off + (cols - 1) * ld + rows) * self.es} bytes, the arena has {self.nbytes}"
        for r in self.regions:   # disjoint: apart in memory, or the same pitch and disjoint row windows
            apart = off + (cols - 1) * ld + rows <= r["off"] or r["off"] + (r["cols"] - 1) * r["ld"] + r["rows"] <= off
            a0, b0 = off % ld, r["off"] % ld
            windows = r["ld"] == ld and off // ld == 0 and r["off"] // ld == 0 and (a0 + rows <= b0 or b0 + r["rows"] <= a0)
            assert apart or windows, "regions overlap"
        flat = self.raw.view(self.dtype)
        view = flat.as_strided((rows, cols), (1, ld), off)
        self.regions.append(dict(kind=kind, rows=rows, cols=cols, ld=ld, off=off, host=host, view=view, aligned=off % V == 0 and ld % V == 0))
        return view

    def place(self, a, dtype, ld, base_off=0, inout=False):
        """the numpy matrix a as an input of the call (inout: the call overwrites it in place)"""
        torch = _torch()
        assert dtype == self.dtype, "one storage type per case: begin() set it"
        a = np.asarray(a)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.raw.device)
        v = self._claim("inout" if inout else "in", a.shape[0], a.shape[1], ld, base_off, t)
        v.copy_(t)
        return v

    def out(self, rows, cols, dtype, ld, base_off=0):
        torch = _torch()
        assert dtype == self.dtype
        v = self._claim("out", rows, cols, ld, base_off, None)
        v.view(torch.int64 if self.es == 8 else torch.int32).fill_(_signed(PREFILL[self.es], self.es))
        return v

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def _bits(self, t):
        torch = _torch()
        return t.contiguous().view(torch.int64 if self.es == 8 else torch.int32)

    def check(self):
        torch = _torch()
        if self.cuda:
            torch.cuda.synchronize()
        for r in self.regions:
            if r["kind"] == "in":
                assert torch.equal(self._bits(r["view"]), self._bits(r["host"])), \
                    f"an input ({r['rows']} x {r['cols']}, ld {r['ld']}) was modified"
        ints = self._ints()
        gap, pre = _signed(self.gap, self.es), _signed(PREFILL[self.es], self.es)
        differ = left = 0
        for s in range(0, ints.numel(), CHUNK):
            c = ints[s:s + CHUNK]
            differ += int(torch.count_nonzero(c != gap))   # (count_nonzero: no widening of the mask to int64, 8 bytes per element)
            left += int(torch.count_nonzero(c == pre))
        want = sum(r["rows"] * r["cols"] for r in self.regions)
        assert left == 0, f"{left} cells of the output regions were never written"
        if differ != want:
            inside = sum(int(torch.count_nonzero(self._bits(r["view"]) != gap)) for r in self.regions)
            raise AssertionError(f"{differ} cells differ from the gap pattern, the regions hold {want}: {differ - inside} cells written "
                                 f"outside every region, {want - inside} of the regions' cells hold the gap pattern")
        peak = torch.cuda.max_memory_allocated() if self.cuda else 0
        assert peak <= CAP_BYTES, f"{peak} bytes of device memory held, the cap is {CAP_BYTES}"
