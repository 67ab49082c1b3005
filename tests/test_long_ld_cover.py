"""Without a GPU: the cases of tests/test_gpu_long_ld.py really lie on the side of every guard they claim to cross, and the arena of
tests/long_ld.py really notices what it is there to notice.

Each guard is restated here from the line that holds it.  If a threshold moves, the restatement (or, for the two edge_level
thresholds of a fit, the plan that fit_plan itself makes: tests/cpp/fit_route.cpp) no longer agrees with the side a case claims,
and this test fails -- instead of the GPU case silently running on the other side."""
import numpy as np
import pytest

import test_gpu_long_ld as T
from test_fit_route import fit, planner  # noqa: F401  (the fixture that builds and runs tests/cpp/fit_route.cpp)
from test_xb_route import planner as xb_planner  # noqa: F401  (... tests/cpp/xb_route.cpp)


def tall_groups(K):
    return 8 if K <= 128 else 16 if K <= 256 else 32


TINY_KMAX, MICRO_K = 416, 32   # tiny_kernels.hpp: UPD_WAVES * TINY_RC, MICRO_K
# guard -> "the fast side holds" as a function of (ld in elements, es, K, A); ld is the long leading dimension of the case
GUARDS = {
    "fused-one-descriptor": lambda ld, es, K, A: tall_groups(K) * ld * es < 1 << 31,         # fit_route.hpp edge_level, cg_all
    "fused-per-wave": lambda ld, es, K, A: tall_groups(K) // 8 * ld * es < 1 << 31,          # ... cg_wave
    "defer": lambda ld, es, K, A: 32 * ld * es < 1 << 31,                                    # defer_kernels.hpp:164 (CG = 32)
    "xb4": lambda ld, es, K, A: 36 * ld * es < 1 << 31,                                      # xb_route.hpp:102,121,130
    "syrk-signed": lambda ld, es, K, A: 8 * ld * es < 1 << 31,                               # syrk_kernels.hpp:226,228,258: the int casts
    "syrk-dma": lambda ld, es, K, A: 8 * ld * es < (1 << 32) - 4096,                         # syrk_kernels.hpp:696
    "resident-gram": lambda ld, es, K, A: K * ld * es < 1 << 31,                             # resident_gram.hpp:77
    "resident": lambda ld, es, K, A: TINY_KMAX * ld * es < 1 << 31,                          # resident_kernels.hpp:37
    "tiny": lambda ld, es, K, A: TINY_KMAX * ld * es < 1 << 30,                              # tiny_kernels.hpp:83
    "micro": lambda ld, es, K, A: MICRO_K * ld * es < 1 << 31,                               # tiny_kernels.hpp:458
    "single-ldt": lambda ld, es, K, A: A * ld * es < 1 << 31,                                # plan_fit_single.hpp:196, on the output T
    "total": lambda ld, es, K, A: (K - 1) * ld <= 1 << 31,                                   # the last column begins within 2^31 elements
}
# guards the GPU cannot reach on both sides under the 20 GiB cap, held by the CPU rows of test_fit_route.py alone: "not addressable"
# for deflate_score_mode / wide_source_ok needs more than 1024 columns 512 MiB apart
BOTH_SIDES = [g for g in GUARDS if g != "total"]


def _claims():
    for c in T.FIT:
        yield "fit " + c["name"], c, c["K"]
    for c in T.XB_CASES:
        yield "xb " + c["name"], c, c["K"]


def test_every_case_lies_on_the_side_it_claims():
    n = 0
    for what, c, cols in _claims():
        ld, es = T.case_ld(c["pitch"], c["dt"], cols), T.ES[c["dt"]]
        assert ld % (16 // es) == 0 and (c["pitch"] == "total" or ld & (ld - 1)), (what, "aligned, no power of two")
        for g, side in c["guards"].items():
            assert side in ("below", "past"), (what, g)
            assert GUARDS[g](ld, es, c["K"], c["A"]) == (side == "below"), (what, g, side, ld)
            n += 1
    assert n > 100


def test_every_guard_has_a_case_on_both_sides():
    seen = {(g, side) for _, c, _ in _claims() for g, side in c["guards"].items()}
    for g in BOTH_SIDES:
        assert (g, "below") in seen and (g, "past") in seen, g
    assert ("total", "past") in seen


def test_every_entry_point_has_both_stresses_and_both_storage_types():
    """(a) a pitch rung and (b) the last column beyond 2^31 elements, in fp64 and in fp32 storage"""
    from test_dual_cv_ref import CASES as CV
    from test_dual_batch_ref import CASES as DB
    from test_dual_cvbatch_ref import CASES_B
    from test_missing_ref import CASES as MS
    from test_resample_ref import CASES as RS
    tables = {
        "fit": [(c["dt"], c["pitch"]) for c in T.FIT],
        "fit DUAL": [(c["dt"], c["pitch"]) for c in T.FIT if c["opts"].get("ALGO") == T.DUAL],
        "xb": [(c["dt"], c["pitch"]) for c in T.XB_CASES],
        "xty": [(c[3], c[4]) for c in T.XTY_CASES],
        "deflate": [(c[2], c[3]) for c in T.DEFLATE_CASES],
        "colwise_z_scores": [(c[2], c[3]) for c in T.ZSCORE_CASES],
        "sse_by_components": [(c[3], c[4]) for c in T.SSE_CASES],
        "model_sse": [(c[4], c[5]) for c in T.MODEL_SSE_CASES],
        "x_diagnostics": [(c[3], c[4]) for c in T.XDIAG_CASES],
        "synth": [(c[4], c[5]) for c in T.SYNTH_CASES],
        "cv_folds": [(c[7], c[8]) for c in T.CV_CASES],
        "cv_folds DUAL": [(CV[n][6], p) for n, p, _ in T.CV_DUAL_CASES],
        "fit_batch": [(c[6], c[7]) for c in T.BATCH_CASES if c[0] == "batched"],
        "fit_batch, one fit per problem": [(c[6], c[7]) for c in T.BATCH_CASES if c[0] != "batched"],
        "fit_batch DUAL": [(DB[n][5], p) for n, p, _ in T.BATCH_DUAL_CASES],
        "fit_resampled": [(RS[n][5], p) for n, p, _, _ in T.RESAMPLE_CASES],
        "cv_press_batch": [(CV[CASES_B[n][0]][6], p) for n, p, _, _ in T.CVBATCH_CASES],
        "fit_missing": [(MS[n][5], p) for n, p, _ in T.MISSING_FIT_CASES],
        "scores_missing": [(MS[n][5], p) for n, p, _ in T.MISSING_SCORES_CASES],
        "colwise_z_scores_missing": [(MS[n][5], p) for n, p, _ in T.MISSING_Z_CASES],
        "cv_folds_missing": [(MS[n][5], p) for n, p, _ in T.MISSING_CV_CASES],
    }
    for entry, rows in tables.items():
        assert {dt for dt, _ in rows} == {"f64", "f32"}, entry
        assert any(p == "total" for _, p in rows), entry
        assert any(p != "total" for _, p in rows) or entry.endswith("DUAL"), entry
    # the refits of fit_resampled's general route: both stresses in fp64 only -- they store the row-scaled copies in the type of X,
    # and no test of the entry point holds that route to a bar in fp32 storage
    refits = [p for _, p, _, dual in T.RESAMPLE_CASES if not dual]
    assert "total" in refits and any(p != "total" for p in refits)


def test_no_case_needs_more_than_the_arena():
    def need(rows, cols, dt, pitch, K=None):
        ld = T.case_ld(pitch, dt, K or cols)
        return ((cols - 1) * ld + 4 * (rows + 48) + 64) * T.ES[dt]
    widest = lambda c, names: max(c[n] for n, l in names.items() if l in c["long"])   # the widest of the matrices that are long
    worst = max([need(c["N"], widest(c, dict(K="X", M="Y", A="T")), c["dt"], c["pitch"], c["K"]) for c in T.FIT] +
                [need(c["N"], widest(c, dict(K="X", C="o")), c["dt"], c["pitch"], c["K"]) for c in T.XB_CASES] +
                [need(c[0], c[1], c[3], c[4]) for c in T.XTY_CASES] + [need(c[0], c[1], c[2], c[3]) for c in T.DEFLATE_CASES + T.ZSCORE_CASES])
    from long_ld import CAP_BYTES
    assert worst <= T.ARENA_BYTES and T.ARENA_BYTES + (1 << 30) <= CAP_BYTES


def test_the_plan_of_every_fit_case_is_on_the_claimed_side(planner):
    """fit_plan itself, on the case's shape and leading dimension: fused_mode 1 below one descriptor, 2 with a descriptor per wave,
    0 where not even a wave's groups fit"""
    rows, want = [], []
    for c in T.FIT:
        if "X" not in c["long"] or not ({T.ONE, T.WAVE_} & set(c["guards"])) or c["K"] > 1024 or not c["opts"].get("FUSE", 1):
            continue
        g = c["guards"]
        mode = 0 if g.get(T.WAVE_) == "past" else 2 if g.get(T.ONE) == "past" else 1
        algo = c["opts"].get("ALGO", 0)
        rows.append(fit(c["N"], c["K"], c["M"], c["A"], c["dt"], algo, method=c["method"], ldx=T.case_ld(c["pitch"], c["dt"], c["K"]),
                        layout=c["opts"].get("WORK_LAYOUT", 1), defer=c["opts"].get("DEFER", 1)))
        want.append((c["name"], mode, c["opts"].get("DEFER", 1) if g.get("defer") == "below" else 1))
    assert len(rows) >= 25
    for (name, mode, defer), got in zip(want, planner(rows)):
        assert got["fused_mode"] == mode and got["defer"] == defer, (name, got["fused_mode"], got["defer"])


def test_the_route_of_every_xb_case_is_on_the_claimed_side(xb_planner):
    """xb_next itself, on the case's shape and leading dimensions at 256 CUs: below the limit the call starts on a 4 x 4 x 4
    matrix-core kernel -- which also takes 32 MiB of X, a tile per CU and the windowed or resident form's own conditions, none of
    which the launch counts show -- and past it no step of the call is one.  (The 1-4 column form, xb4_few, needs a very tall
    matrix with K >= 128: beyond the arena at 48 MiB per column.  It has the rows of tests/test_xb_route.py only.)"""
    calls, sides = [], []
    for c in T.XB_CASES:
        if "xb4" not in c["guards"]:
            continue
        ld = T.case_ld(c["pitch"], c["dt"], c["K"])
        calls.append(((c["N"], c["K"], c["C"], c["dt"], ld if "X" in c["long"] else "aligned", ld if "o" in c["long"] else "aligned", None), 0))
        sides.append((c["name"], c["guards"]["xb4"]))
    assert sum(side == "below" for _, side in sides) >= 4 and sum(side == "past" for _, side in sides) >= 10
    for (name, side), steps in zip(sides, xb_planner(calls)):
        if side == "below":
            assert steps[0].startswith("xb_mfma4"), (name, steps)
        else:
            assert not any(st.startswith("xb_mfma4") for st in steps), (name, steps)


# ---- the arena notices ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def arena():
    torch = pytest.importorskip("torch")
    from long_ld import Arena
    return torch, Arena(1 << 16, device="cpu")


@pytest.mark.parametrize("dt,fill", [("f64", "nan"), ("f32", "nan"), ("f64", "huge"), ("f32", "huge")])
def test_arena_passes_a_clean_call_and_catches_a_dirty_one(arena, dt, fill):
    torch, a = arena
    tdt = torch.float64 if dt == "f64" else torch.float32
    Xh = np.arange(21 * 5, dtype=np.float64).reshape(21, 5) + 1.0

    def lay():
        a.begin(tdt, fill)
        return a.place(Xh, tdt, 400, 16), a.place(Xh[:, :2], tdt, 400, 64, inout=True), a.out(21, 3, tdt, 400, 128)
    X, Y, O = lay()
    assert X.stride() == (1, 400) and np.array_equal(X.numpy(), Xh.astype(X.numpy().dtype))
    O.copy_(X[:, :3]); Y.mul_(2.0)
    a.check()
    X, Y, O = lay(); O[:, :2] = 1.0                      # an output cell never written
    with pytest.raises(AssertionError, match="never written"):
        a.check()
    X, Y, O = lay(); O.fill_(1.0); X[3, 2] = -1.0        # an input modified
    with pytest.raises(AssertionError, match="was modified"):
        a.check()
    X, Y, O = lay(); O.fill_(1.0)
    a.raw.view(tdt)[128 + 21] = 0.0                      # a store one row past the output's first column
    with pytest.raises(AssertionError, match="1 cells written outside"):
        a.check()
    X, Y, O = lay(); O.fill_(1.0)
    a.raw.view(tdt)[16 + 4 * 400 + 399] = 5.0            # ... into the gap just before the next window's last column
    with pytest.raises(AssertionError, match="outside"):
        a.check()
    with pytest.raises(AssertionError, match="overlap"):
        a.place(Xh, tdt, 400, 30)


def test_arena_refuses_to_outgrow_the_cap():
    pytest.importorskip("torch")
    from long_ld import CAP_BYTES, Arena
    with pytest.raises(AssertionError, match="cap"):
        Arena(CAP_BYTES, device="meta")
