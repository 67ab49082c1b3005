"""The plan of a fit, checked without a GPU: fit_plan (pls_amd/csrc/fit_route.hpp) is a pure function of the shape, so which plan
a fit takes, when the tiled copy is made, which tile height it gets, whether component 1 writes half-height tiles and where AUTO
goes can be asserted on the CPU -- a GPU test sees these only through parity.  tests/cpp/fit_route.cpp, built with ASan + UBSan,
prints the plan.  The expected values are derived by hand from the thresholds (256 CUs, 16-byte aligned matrices with the leading
dimension N rounded up to 16 bytes unless a row says otherwise: what pls_amd.colmajor_empty makes)."""
import os
import subprocess

import pytest

from test_gpu_last_pass import AS, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CU = 256
KERNEL, NIPALS, GRAM, AUTO = 0, 1, 2, 3   # pls_hip_algo
TYPE1, TYPE2 = 0, 1                       # pls_hip_method
FIT_NO_COPY = 1                           # plsk::FIT_NO_COPY


def fit(N, K, M, A, dt, algo, **kw):
    """a row: the shape and the handle's settings (defaults: what a new handle has)"""
    d = dict(N=N, K=K, M=M, A=A, dt=dt, algo=algo, method=TYPE1, fuse=1, layout=1, defer=1, grid=0, reducer=0, pre=0, xep=0,
             ldx=None, xmod=0, denied=0)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


def pad(N, dt):
    V = 16 // (8 if dt == "f64" else 4)
    return -(-N // V) * V


def tiled(N, WR, K, dt):
    """bytes of a working copy in tiles of WR rows"""
    return -(-N // WR) * WR * K * (8 if dt == "f64" else 4)


def colmajor(N, K, dt):
    """bytes of a column-major working copy (rows up to a multiple of 4)"""
    return (N + 3) // 4 * 4 * K * (8 if dt == "f64" else 4)


# ---- NIPALS: the rows of test_gpu_last_pass.SHAPES, by their labels there ----------------------------------------------------------
# (N, K, storage) -> tile of the caller's matrix: column groups (8 up to 128 columns, 16 up to 256, else 32), rows (512 / groups
# lanes x 16 bytes); every one of these matrices is aligned and short enough for fused_mode 1 up to 1024 columns
TALL_TILE = {(4098, 512, "f64"): (32, 32), (4098, 512, "f32"): (32, 64), (3000, 96, "f64"): (8, 128), (3000, 96, "f32"): (8, 256),
             (1030, 700, "f64"): (32, 32), (2052, 1024, "f32"): (32, 64), (4097, 200, "f64"): (16, 64), (5003, 200, "f32"): (16, 128),
             (516, 2048, "f32"): (32, 64), (260, 4096, "f32"): (32, 64)}
SHORT_TILE = {2048: (128, 16), 4096: (256, 8)}   # K -> column groups, rows (fp32) of the short tiles of 1024 < K <= 4096


def nipals_expected(route, N, K, M, dt, layout, A):
    cg, TR = TALL_TILE[(N, K, dt)]
    e = dict(algo="NIPALS", tall_cg=cg, TR=TR, retile_fit=0, wide_only=0, defer=1, use_pre=0)
    if route in ("tall", "tall-ragged", "tailrows"):       # the tile-resident pass on the caller's matrix, a copy in the same tiles
        e.update(fused_mode=1, semi_fit=0, tiled_work=1, mid_cg=0, wide_cg=0, WR=TR, nip_copy=0, work=tiled(N, TR, K, dt), ldw=TR, tsw=TR * K)
    elif route in ("layout0", "tailrows-layout0"):         # ... a column-major copy
        e.update(fused_mode=1, semi_fit=0, tiled_work=0, mid_cg=0, wide_cg=0, WR=TR, nip_copy=0, work=colmajor(N, K, dt), ldw=pad(N, dt), tsw=TR)
    elif route == "half":                                  # 512 < K <= 1024: half-height tiles from the third component on
        WR = TR // 2 if A > 2 else TR
        e.update(fused_mode=1, semi_fit=0, tiled_work=1, mid_cg=64 if A > 2 else 0, wide_cg=0, WR=WR, nip_copy=0, work=tiled(N, WR, K, dt),
                 ldw=WR, tsw=WR * K)
    elif route == "short":                                 # 1024 < K <= 4096: short tiles, from three components on made by the X^T Y sweep
        wcg, WR = SHORT_TILE[K]
        e.update(fused_mode=0, wide_mode=1, semi_fit=1, tiled_work=1, mid_cg=0, wide_cg=wcg, WR=WR, nip_copy=int(A >= 3),
                 work=tiled(N, WR, K, dt), ldw=WR, tsw=WR * K)
    else:
        raise AssertionError(route)
    if A == 1:
        e["work"] = 0                                      # nothing is deflated
    return e


NIPALS_ROWS = [(f"{route} {N}x{K} M={M} {dt} layout={layout} A={A}", fit(N, K, M, A, dt, NIPALS, layout=layout),
                nipals_expected(route, N, K, M, dt, layout, A))
               for route, N, K, M, dt, layout in SHAPES for A in AS]

WIDE_ONLY = dict(algo="NIPALS", fused_mode=0, wide_mode=0, semi_fit=0)   # 6144 columns: beyond the semi-fused sweep's 4608
NIPALS_MORE = [
    ("wide_only", fit(3000, 6144, 1, 3, "f64", NIPALS),
     dict(WIDE_ONLY, wide_only=1, tiled_work=1, wide_cg=512, mid_cg=0, WR=2, nip_copy=1, work=3000 * 6144 * 8, ldw=2, tsw=2 * 6144)),
    ("wide_only shape, A=2", fit(3000, 6144, 1, 2, "f64", NIPALS),
     dict(WIDE_ONLY, wide_only=0, tiled_work=0, wide_cg=0, mid_cg=0, WR=32, nip_copy=0, work=3000 * 6144 * 8, ldw=3000, tsw=32)),
    ("opt_fuse=0", fit(4098, 512, 1, 3, "f64", NIPALS, fuse=0),
     dict(algo="NIPALS", fused_mode=0, wide_mode=0, semi_fit=0, tiled_work=0, wide_cg=0, mid_cg=0, WR=32, work=colmajor(4098, 512, "f64"),
          ldw=4098, tsw=32, nip_copy=0)),
    ("opt_defer=2, qualifies", fit(4098, 512, 1, 6, "f64", NIPALS, defer=2), dict(fused_mode=1, tall_cg=32, tiled_work=1, defer=2)),
    ("opt_defer=2, a 16-group tile", fit(4097, 200, 2, 6, "f64", NIPALS, defer=2), dict(fused_mode=1, tall_cg=16, tiled_work=1, defer=1)),
    ("opt_defer=2, an odd row count", fit(4097, 512, 1, 6, "f64", NIPALS, defer=2), dict(fused_mode=1, tall_cg=32, tiled_work=1, defer=1)),
    # test_last_pass_parity_unaligned_columns: X = big[:, 1:N + 1].t() of a (K, N + 3) buffer -- 8 bytes off the 16-byte grid
    ("unaligned columns f64", fit(1001, 37, 2, 3, "f64", NIPALS, ldx=1004, xmod=8),
     dict(fused_mode=2, tall_cg=8, TR=128, WR=128, tiled_work=1, wide_cg=0, mid_cg=0, defer=1, work=tiled(1001, 128, 37, "f64"))),
    ("unaligned columns f32", fit(1001, 37, 2, 2, "f32", NIPALS, ldx=1004, xmod=4),
     dict(fused_mode=2, tall_cg=8, TR=256, WR=256, tiled_work=1, work=tiled(1001, 256, 37, "f32"))),
    ("unaligned columns, odd ld", fit(1001, 37, 2, 3, "f64", NIPALS, ldx=1003, xmod=8), dict(fused_mode=2, defer=1)),
]

# ---- KERNEL: when the tiled copy is made -------------------------------------------------------------------------------------------
NO_COPY = dict(algo="KERNEL", retile_fit=0, wide_cg=0, work=0, tiled_work=0, nip_copy=0, mid_cg=0)


def copy(cg, WR, N, K, dt="f64"):
    return dict(algo="KERNEL", retile_fit=1, wide_cg=cg, WR=WR, work=tiled(N, WR, K, dt), ldw=WR, tsw=WR * K, tiled_work=0, nip_copy=0, mid_cg=0)


KERNEL_ROWS = [
    # aligned, K <= 512: from 10 components on, in the tiles of the caller's matrix
    ("aligned K=512 A=9", fit(20000, 512, 1, 9, "f64", KERNEL), dict(NO_COPY, fused_mode=1)),
    ("aligned K=512 A=10", fit(20000, 512, 1, 10, "f64", KERNEL), dict(copy(32, 32, 20000, 512), fused_mode=1)),
    # aligned, 512 < K <= 1024: from 32 on, in half-height tiles
    ("aligned K=1024 A=31", fit(20000, 1024, 1, 31, "f64", KERNEL), dict(NO_COPY, fused_mode=1)),
    ("aligned K=1024 A=32", fit(20000, 1024, 1, 32, "f64", KERNEL), dict(copy(64, 16, 20000, 1024), fused_mode=1)),
    # columns off the 16-byte grid: from 4 on
    ("unaligned K=512 A=3", fit(20000, 512, 1, 3, "f64", KERNEL, xmod=8), dict(NO_COPY, fused_mode=2)),
    ("unaligned K=512 A=4", fit(20000, 512, 1, 4, "f64", KERNEL, xmod=8), dict(copy(32, 32, 20000, 512), fused_mode=2)),
    # 1024 < K <= 4096: from 3 on, in short tiles
    ("K=2048 A=2", fit(10000, 2048, 1, 2, "f64", KERNEL), dict(NO_COPY, fused_mode=0, wide_mode=1)),
    ("K=2048 A=3", fit(10000, 2048, 1, 3, "f64", KERNEL), dict(copy(128, 8, 10000, 2048), fused_mode=0, wide_mode=1)),
    # beyond 8192 columns: row-pack tiles, only from 4096 rows on
    ("K=10000 N=3000", fit(3000, 10000, 1, 5, "f64", KERNEL), dict(NO_COPY, fused_mode=0, wide_mode=0)),
    ("K=10000 N=6000", fit(6000, 10000, 1, 5, "f64", KERNEL), dict(copy(512, 2, 6000, 10000), fused_mode=0, wide_mode=0)),
    # 9 responses: the copy of a wide matrix is still made (by a launch of its own: X^T Y rides only up to 8 responses), that of
    # a matrix the tile-resident pass covers is not
    ("K=2048 M=9", fit(10000, 2048, 9, 3, "f64", KERNEL), copy(128, 8, 10000, 2048)),
    ("aligned K=512 A=10 M=9", fit(20000, 512, 9, 10, "f64", KERNEL), dict(NO_COPY, fused_mode=1)),
    # refused its memory: planned again, no copy, the tall tile's geometry, no work buffer
    ("K=2048 A=3, copy refused", fit(10000, 2048, 1, 3, "f64", KERNEL, denied=FIT_NO_COPY), dict(NO_COPY, WR=32, ldw=10000, tsw=32)),
    ("aligned K=512 A=10, copy refused", fit(20000, 512, 1, 10, "f64", KERNEL, denied=FIT_NO_COPY), dict(NO_COPY, WR=32, fused_mode=1)),
]

# ---- AUTO, KERNEL_TYPE2, GRAM ------------------------------------------------------------------------------------------------------
C3 = (1048576, 512, 1)
C4 = (131072, 4096, 8, 50, "f32")
C5 = (16777216, 1024, 4, 20, "f64")   # all eight shards
PLAN_ROWS = [
    # config 3, 20 components: 21 passes of 0.72 ms + launches = 15.3 ms against SYRK 4.7 + T 0.9 + loop 0.4 = 6.1 ms
    ("AUTO config 3", fit(*C3, 20, "f64", AUTO), dict(algo="GRAM", use_pre=0, retile_fit=0, work=0, red=8 * 513 * 8, ssmax=4096, prow=2048)),
    ("AUTO config 3, A=1", fit(*C3, 1, "f64", AUTO), dict(algo="KERNEL", use_pre=0)),   # 1.4 ms against 5.7 ms
    ("AUTO config 3, a reducer", fit(*C3, 20, "f64", AUTO, reducer=1), dict(algo="KERNEL", xep_ok=0)),
    ("AUTO config 3, products uploaded", fit(*C3, 1, "f64", AUTO, pre=1), dict(algo="GRAM", use_pre=1)),
    ("AUTO K=4096", fit(131072, 4096, 1, 50, "f64", AUTO), dict(algo="KERNEL", retile_fit=1, wide_cg=256, WR=4)),
    ("NIPALS config 4", fit(*C4, NIPALS),
     dict(algo="NIPALS", fused_mode=0, wide_mode=1, semi_fit=1, wide_only=0, tiled_work=1, wide_cg=256, WR=8, nip_copy=1, retile_fit=0,
          work=131072 * 4096 * 4, part=2048 * 4096 * 8 * 8, ssmax=2048, red=8 * 4096 * 8 * 8)),
    ("KERNEL config 4", fit(*C4, KERNEL), dict(copy(256, 8, 131072, 4096, "f32"), fused_mode=0, wide_mode=1, semi_fit=0)),
    # config 5 unsharded: 32 column groups x 16,777,216 rows x 8 bytes do not fit one descriptor -- per-wave descriptors, mode 2
    ("NIPALS config 5", fit(*C5, NIPALS),
     dict(algo="NIPALS", fused_mode=2, tall_cg=32, tiled_work=1, mid_cg=64, wide_cg=0, WR=16, defer=1, work=16777216 * 1024 * 8,
          ssmax=262144, part=2048 * 4096 * 8)),
    ("KERNEL config 5", fit(*C5, KERNEL), dict(NO_COPY, fused_mode=2, WR=32)),   # 20 components: the copy pays from 32 on
    ("KERNEL_TYPE2", fit(20000, 512, 1, 10, "f64", KERNEL, method=TYPE2), dict(algo="TYPE2", use_pre=0, retile_fit=0, work=0)),
    ("KERNEL_TYPE2 under NIPALS, products uploaded", fit(20000, 512, 1, 10, "f64", NIPALS, method=TYPE2, pre=1),
     dict(algo="TYPE2", use_pre=1, tiled_work=0, work=0)),
    ("GRAM", fit(20000, 512, 1, 10, "f64", GRAM), dict(algo="GRAM", use_pre=0, retile_fit=0, work=0)),
    ("the device-side exchange", fit(20000, 512, 1, 5, "f64", NIPALS, reducer=1, xep=1), dict(algo="NIPALS", xep_ok=1)),
    ("... beyond one message piece", fit(1000, 70000, 1, 5, "f64", NIPALS, reducer=1, xep=1), dict(xep_ok=0)),
    ("... not attached", fit(20000, 512, 1, 5, "f64", NIPALS, reducer=1), dict(xep_ok=0)),
]

# ---- long leading dimensions: either side of every edge_level threshold ------------------------------------------------------------
# The tile that reads the caller's matrix has CG = 8 / 16 / 32 column groups (K <= 128 / <= 256 / beyond) behind ONE descriptor
# while CG ld es < 2^31 (fused_mode 1): 256 / 128 / 64 MiB per column.  From there on a descriptor per wave (CG / 8 groups:
# fused_mode 2) while (CG / 8) ld es < 2^31: 2 GiB / 1 GiB / 512 MiB per column, then the tile-resident pass is out (fused_mode 0).
# deflate_score_mode and wide_source_ok read with 32 groups, 4 per wave: one descriptor below 64 MiB (wide_mode 1), per wave
# below 512 MiB (wide_mode 2), not addressable from 512 MiB on (wide_mode 0, no short-tile copy: the one-product kernels).
MiB = 1 << 20
LD_N = 5000
ONE_DESCRIPTOR = {40: 256 * MiB, 200: 128 * MiB, 260: 64 * MiB}     # K -> bytes per column from which CG columns overflow 2^31
PER_WAVE = {9: 2048 * MiB, 200: 1024 * MiB, 260: 512 * MiB}        # K -> bytes per column from which a wave's groups do


def ld_at(nbytes, dt, below):
    """the leading dimension (elements) of `nbytes` per column, or the last 16-byte aligned one below it"""
    es = 8 if dt == "f64" else 4
    return nbytes // es - (16 // es if below else 0)


def _long_ld_rows():
    rows = []
    names = {KERNEL: "KERNEL", NIPALS: "NIPALS", GRAM: "GRAM", AUTO: "KERNEL"}   # (AUTO at 6 components of 5000 rows: KERNEL)
    for dt in ("f64", "f32"):
        for algo in (KERNEL, NIPALS, GRAM, AUTO):
            for K, nbytes in ONE_DESCRIPTOR.items():
                for below in (True, False):
                    want = dict(algo=names[algo], fused_mode=1 if below else 2, wide_mode=0, tall_cg=8 if K <= 128 else 16 if K <= 256 else 32)
                    if algo == NIPALS:   # the working copy is tiled on either side
                        want.update(tiled_work=1, semi_fit=0, defer=1)
                    rows.append((f"{names[algo]}/{algo} K={K} {dt} {'below' if below else 'at'} {nbytes // MiB} MiB",
                                 fit(LD_N, K, 1, 6, dt, algo, ldx=ld_at(nbytes, dt, below)), want))
            for K, nbytes in PER_WAVE.items():
                for below in (True, False):
                    want = dict(algo=names[algo], fused_mode=2 if below else 0, wide_mode=0)
                    if algo == NIPALS:   # past the limit: a column-major copy for the one-product kernels
                        want.update(tiled_work=int(below), semi_fit=0, wide_only=0, nip_copy=0, wide_cg=0)
                        if not below:
                            want.update(work=colmajor(LD_N, K, dt), ldw=pad(LD_N, dt))
                    if algo == KERNEL:   # (6 components: below the 10 from which the copy of an aligned matrix pays)
                        want.update(retile_fit=0, work=0)
                    rows.append((f"{names[algo]}/{algo} K={K} {dt} {'below' if below else 'at'} {nbytes // MiB} MiB (per wave)",
                                 fit(LD_N, K, 1, 6, dt, algo, ldx=ld_at(nbytes, dt, below)), want))
        # 1024 < K <= 4096: fused_mode 0 at any ld; the semi-fused sweep and the short-tile copy follow wide_mode
        for algo in (KERNEL, NIPALS):
            for nbytes, lo, hi in ((64 * MiB, 1, 2), (512 * MiB, 2, 0)):
                for below in (True, False):
                    wm = lo if below else hi
                    want = dict(fused_mode=0, wide_mode=wm, wide_cg=128 if wm else 0)
                    want.update(dict(semi_fit=int(wm != 0), tiled_work=int(wm != 0), nip_copy=int(wm != 0)) if algo == NIPALS
                                else dict(retile_fit=int(wm != 0)))
                    rows.append((f"algo {algo} K=2048 {dt} {'below' if below else 'at'} {nbytes // MiB} MiB",
                                 fit(LD_N, 2048, 1, 6, dt, algo, ldx=ld_at(nbytes, dt, below)), want))
        # 4096 < K <= 8192 under NIPALS: wide_only needs wide_source_ok -- gone from 512 MiB per column on
        for below in (True, False):
            rows.append((f"wide_only K=6144 {dt} {'below' if below else 'at'} 512 MiB",
                         fit(3000, 6144, 1, 3, dt, NIPALS, ldx=ld_at(512 * MiB, dt, below)),
                         dict(fused_mode=0, wide_mode=0, wide_only=int(below), wide_cg=512 if below else 0, tiled_work=int(below))))
    # the deferred write-back needs ONE descriptor for the 32 groups (fused_mode 1)
    rows.append(("opt_defer=2 below 64 MiB", fit(4098, 512, 1, 6, "f64", NIPALS, defer=2, ldx=ld_at(64 * MiB, "f64", True)),
                 dict(fused_mode=1, tall_cg=32, defer=2)))
    rows.append(("opt_defer=2 at 64 MiB", fit(4098, 512, 1, 6, "f64", NIPALS, defer=2, ldx=ld_at(64 * MiB, "f64", False)),
                 dict(fused_mode=2, tall_cg=32, defer=1)))
    # AUTO with 40 components of 5000 x 260 fp64: 41 passes of 1.73 us + 40 x 14 us = 0.631 ms against SYRK 12.8 us + T 2.3 us +
    # 40 x 13.7 us + 40 us = 0.602 ms -- GRAM, whatever the leading dimension is
    rows.append(("AUTO A=40 at 64 MiB", fit(LD_N, 260, 1, 40, "f64", AUTO, ldx=ld_at(64 * MiB, "f64", False)), dict(algo="GRAM", fused_mode=2)))
    return rows


LONG_LD_ROWS = _long_ld_rows()

ROWS = NIPALS_ROWS + NIPALS_MORE + KERNEL_ROWS + PLAN_ROWS + LONG_LD_ROWS


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_route") / "fit_route")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "fit_route.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def plan(fits):
        """fits: rows of fit() -> per row the plan as a dict (numbers as int)"""
        lines = []
        for d in fits:
            es = 8 if d["dt"] == "f64" else 4
            ld = pad(d["N"], d["dt"])
            tmod = 0 if d["method"] == TYPE1 else -1
            lines.append(f"{d['N']} {d['K']} {d['M']} {d['A']} {es} {d['ldx'] or ld} {ld} {ld} {d['xmod']} 0 {tmod} {NUM_CU} {d['method']} "
                         f"{d['algo']} {d['fuse']} {d['layout']} {d['defer']} {d['grid']} {d['reducer']} {d['pre']} {d['xep']} {d['denied']}")
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
        out = [{k: (v if k == "algo" else int(v)) for k, v in (kv.split("=") for kv in line.split())} for line in p.stdout.splitlines()]
        assert len(out) == len(fits)
        return out
    return plan


def test_every_row_gets_its_plan(planner):
    for (name, _, want), got in zip(ROWS, planner([d for _, d, _ in ROWS])):
        assert {k: got[k] for k in want} == want, name


def test_the_table_covers_every_last_pass_shape():
    assert len(NIPALS_ROWS) == len(SHAPES) * len(AS) and AS == [1, 2, 3, 6]
    assert {route for route, *_ in SHAPES} == {"tall", "tall-ragged", "layout0", "half", "short", "tailrows", "tailrows-layout0"}


def test_a_refused_copy_changes_only_what_follows_from_it(planner):
    """planned again under FIT_NO_COPY, a fit keeps its plan, its tall tile and every workspace but `work`"""
    rows = [d for _, d, want in KERNEL_ROWS if want.get("retile_fit") == 1]
    assert len(rows) >= 6
    for d, first, second in zip(rows, planner(rows), planner([dict(d, denied=FIT_NO_COPY) for d in rows])):
        assert first["retile_fit"] == 1 and first["work"] > 0, d
        changed = {k for k in first if first[k] != second[k]}
        assert {"retile_fit", "wide_cg", "work"} <= changed <= {"retile_fit", "wide_cg", "work", "WR", "ldw", "tsw"}, (d, changed)
        assert second["wide_cg"] == 0 and second["work"] == 0 and second["WR"] == second["TR"], d


def test_a_plan_without_a_copy_ignores_the_refusal(planner):
    rows = [d for _, d, want in ROWS if want.get("retile_fit") == 0 and not d["denied"]]
    assert planner(rows) == planner([dict(d, denied=FIT_NO_COPY) for d in rows])
