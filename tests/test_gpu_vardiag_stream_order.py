"""pls_hip_var_diagnostics held to the order of the stream it was given: its cases of the stream-order catalogue.

tests/stream_order.py, the catalogue module, is left as it is; the cases of this entry point are registered here, when this module
is imported, with the catalogue's own add(): an fp64 and an fp32 case of the full call at 1001 x 37, A = 6, M = 2, and one
VIP-only case with tt given, all marked *enqueues* as the header's "Stream order" table says.  tests/test_stream_order_cover.py
holds the catalogue to the header when the suite is collected as a whole (a module of tests/ is imported before any test runs),
and the test below runs the cases through the catalogue's run_case: two synchronous baselines, the sandwich on the warm handle and
on a fresh one."""
import pytest

import stream_order as so

GROUP = "pls_hip_var_diagnostics"


def _register():
    if any(c.entry == GROUP for c in so.CASES):   # (imported twice, or the catalogue has them itself)
        return
    N, K, M, A = 1001, 37, 2, 6
    p, ld, cm = so.p, so.ld, so.cm

    def outs_vd(i):
        torch = so._torch()
        return {"ssxk": cm(K, A + 1, ld=K), "VIP": cm(K, A, ld=K), "sst": torch.empty(A, dtype=torch.float64, device="cuda")}

    def call_vd(h, i, o, seed):
        return so._lib().pls_hip_var_diagnostics(h.h, p(i["X"]), ld(i["X"]), N, K, M, A, p(i["W"]), p(i["R"]), p(i["P"]), p(i["Q"]), None,
                                                 so.dt_of(i["X"]), p(o["ssxk"]), ld(o["ssxk"]), p(o["VIP"]), ld(o["VIP"]), p(o["sst"]))
    for f32 in (False, True):
        def gen_vd(u, seed, f32=f32):
            return {"X": u.synth_x(0, N, K, seed, dtype=so._dt(f32)), "W": so.normal(seed, "vdW", K, A), "R": so.normal(seed, "vdR", K, A),
                    "P": so.normal(seed, "vdP", K, A), "Q": so.normal(seed, "vdQ", M, A)}
        so.add("var_diagnostics 1001x37 a6 m2", GROUP, "scores, one column sweep, VIP from the call's own sst", "default", so.ENQUEUES,
               gen_vd, outs_vd, call_vd, lambda l: so._check(l["xb"] >= 2, l), f32=f32)

    def gen_vip(u, seed):
        return {"W": so.normal(seed, "vdW", K, A), "Q": so.normal(seed, "vdQ", M, A), "tt": so.normal(seed, "vdtt", A).abs_().add_(1.0)}

    def call_vip(h, i, o, seed):
        return so._lib().pls_hip_var_diagnostics(h.h, None, 0, 0, K, M, A, p(i["W"]), None, None, p(i["Q"]), p(i["tt"]), 0, None, 0,
                                                 p(o["VIP"]), ld(o["VIP"]), None)
    so.add("var_diagnostics VIP alone, tt given", GROUP, "nothing N-sized is read", "default", so.ENQUEUES, gen_vip,
           lambda i: {"VIP": cm(K, A, ld=K)}, call_vip, lambda l: so._check(l["xb"] == 0 and l["fused"] == 0, l))


_register()


@pytest.fixture(scope="module")
def bench():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    b = so.Bench()
    yield b
    b.close()


def test_the_cases_are_in_the_catalogue():
    """without a GPU: three cases, one of them fp32, all *enqueues*, each answering to the entry's own row of the header's table"""
    mine = [c for c in so.CASES if c.entry == GROUP]
    assert len(mine) == 3 and sum(c.f32 for c in mine) == 1
    assert all(c.mark == so.ENQUEUES and c.row == GROUP and c.group == GROUP for c in mine)


@pytest.mark.gpu
def test_catalogue_cases(bench):
    cases = [c for c in so.CASES if c.group == GROUP]
    assert len(cases) == 3
    bad = []
    for c in cases:
        bad += so.run_case(bench, c)
    assert not bad, "\n".join(bad)
