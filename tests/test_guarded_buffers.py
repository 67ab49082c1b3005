"""The guarded-matrix helper of test_gpu_bounds on the CPU: one changed guard cell, or one prefill cell left in a
region, must make its checks fail -- the GPU bounds tests are only as good as these two checks."""
import numpy as np
import pytest

from test_gpu_bounds import LEAD_BYTES, PREFILL, SENTINEL, TRAIL_BYTES, Guarded


def _backends():
    import torch
    return [("cpu", torch.float64), ("cpu", torch.float32), ("numpy", np.float64), ("numpy", np.float32)]


@pytest.mark.parametrize("layout", ["aligned", "eigen"])
@pytest.mark.parametrize("b", range(4))
def test_guarded_layout_and_checks(layout, b):
    device, dt = _backends()[b]
    specs = [(7, 3), (5, 2, 5), (1, 1)]
    g = Guarded(specs, dt, layout, device)
    es = g.es
    V = 16 // es
    for i, (s, off, ld) in enumerate(zip(g.specs, g.offs, g.lds)):
        rows, cols = s
        assert g[i].shape == (rows, cols)
        if len(specs[i]) == 2:
            assert ld == (rows if layout == "eigen" else -(-rows // V) * V + V)
        assert off % V == (1 if layout == "eigen" else 0)
        assert off * es >= LEAD_BYTES
        if i + 1 < len(g):
            assert g.offs[i + 1] - (off + ld * cols) >= max(4 * ld, TRAIL_BYTES // es)   # the gap to the next region
        # the view addresses the cells of the flat buffer it claims to
        strides = g[i].strides if device == "numpy" else tuple(x * es for x in g[i].stride())
        assert strides[0] == es and (cols == 1 or strides[1] == ld * es)
        assert g.ptr(i).value == (g.raw.ctypes.data if device == "numpy" else g.raw.data_ptr()) + off * es
    # freshly made: every guard untouched, every region still prefilled
    g.assert_untouched()
    for i in range(len(g)):
        g.assert_prefilled(i)
        with pytest.raises(AssertionError, match="never written"):
            g.assert_written(i)
    # a fully written buffer passes
    for i in range(len(g)):
        g[i][...] = 1.5
    g.check()
    # one prefill cell left (the last element of the middle region) fails, and is located
    g.bits(1)[4, 1] = PREFILL[es]
    with pytest.raises(AssertionError, match=r"region 1: 1 elements never written, first \(row, column\) \[\[4, 1\]\]"):
        g.assert_written()
    g.assert_written(1, cols=1)       # (outside the leading columns asked for)
    g[1][4, 1] = 2.0
    g.check()
    # one guard cell changed fails: just before a region, the padding row after a column, one past the region's end,
    # far into the trailing guard -- by one bit, or to a NaN of another payload
    ld = g.lds[0]
    for j, val in [(g.offs[0] - 1, SENTINEL[es] ^ 1), (g.offs[0] + 7, PREFILL[es]), (g.offs[0] + 3 * ld, 0),
                   (g.offs[2] + 1 + 100, SENTINEL[es] ^ (1 << 40 if es == 8 else 1 << 20))]:
        if layout == "eigen" and j == g.offs[0] + 7:
            j = g.offs[0] + 3 * ld + 1
        old = g.raw[j].item()
        g.raw[j] = val
        with pytest.raises(AssertionError, match="1 guard cells written"):
            g.assert_untouched()
        g.raw[j] = old
        g.assert_untouched()
    # refill puts every region back to the prefill and leaves the guards alone
    g.refill()
    g.assert_untouched()
    for i in range(len(g)):
        g.assert_prefilled(i)


def test_guarded_payloads_are_distinct_nans():
    for es, idt, fdt in [(8, np.int64, np.float64), (4, np.int32, np.float32)]:
        s, p = np.array([SENTINEL[es]], dtype=idt).view(fdt), np.array([PREFILL[es]], dtype=idt).view(fdt)
        assert np.isnan(s).all() and np.isnan(p).all() and SENTINEL[es] != PREFILL[es]
