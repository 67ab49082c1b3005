"""xdiagmiss_geom_of (pls_amd/csrc/xdiagmiss_layout.hpp), the pure function that chooses the route, the tile, the K split and the
workspace of pls_hip_x_diagnostics_missing, checked without a GPU: the header is plain C++, tests/cpp/xdiagmiss_layout.cpp includes
it alone, is built with ASan + UBSan and run as a process of its own.  It holds every case of tests/test_xdiag_missing_ref.py to the
route and the tile rows the case claims, the tile to the on-chip budget, the workspace below 4 GB and the K split to covering K
exactly -- for the cases and for a sweep of shapes around the thresholds.  The same program holds the K split of the fit
(miss_geom_of) and of the streaming route to miss_row_split (pls_amd/csrc/miss_layout.hpp), the one copy of the rule."""
import os
import subprocess

import pytest

from test_missing_ref import TAILS as FIT_TAILS
from test_xdiag_missing_ref import CASES, RESIDENT, TAILS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geoms(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xdiagmiss_layout") / "xdiagmiss_layout")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "xdiagmiss_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = "".join(f"{n} {c[0]} {c[1]} {c[2]} {4 if c[4] == 'f32' else 8} {0 if c[5] == RESIDENT else 1} {c[6]}\n" for n, c in CASES.items())
    p = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    out = {}
    count = {"swept": 0, "split": 0}
    for l in p.stdout.splitlines():
        f = l.split()
        if f[0] in count:
            count[f[0]] = int(f[1])
        else:
            out[(f[0], int(f[1]))] = dict(route=int(f[2]), rt=int(f[3]), S=int(f[4]), kper=int(f[5]), ws=int(f[6]), split_S=int(f[7]),
                                          tail=(int(f[8]), int(f[9])))
    return out, count


def test_every_case_lies_on_the_route_it_claims(geoms):
    out, count = geoms
    assert len(out) == 2 * len(CASES) and count["swept"] > 1000
    for n, c in CASES.items():
        for al in (0, 1):
            g = out[(n, al)]
            assert g["route"] == (0 if c[5] == RESIDENT else 1) and g["rt"] == c[6], (n, g)
            assert g["ws"] < 4 << 30
            assert g["S"] * g["kper"] >= c[1] > (g["S"] - 1) * g["kper"]
    print({n: out[(n, 1)] for n in CASES})


def test_both_routes_and_both_storage_types_are_covered():
    kinds = {(c[5], c[4]) for c in CASES.values()}
    assert len(kinds) == 4, kinds
    assert {c[6] for c in CASES.values()} == {0, 8, 16, 32, 64}


def test_the_k_split_is_written_once(geoms):
    """the program held miss_geom_of and xdiagmiss_geom_of to miss_row_split, the ranges to covering K and a range to whole turns
    of the column lanes on every shape of its sweep: 81 row counts (1 .. 70, 255 .. 260, 511 .. 514, 5000) x 10 column counts x
    element sizes 4, 8 x rows per lane 1, 16 / es x 1, 64, 256 compute units"""
    assert geoms[1]["split"] == 81 * 10 * 2 * 2 * 3


def test_tail_cases_straddle_the_batches_of_the_lane_walk(geoms):
    """The cases that are in the tables for the batch tails of miss_row_walk have, in the aligned layout on 256 compute units, the
    columns per lane in the last K range that the tables claim (TAILS of the two files): U - 1, U and U + 1 for the fit's U = 8
    and for the diagnostics' U = 4, each with several column lanes per row and with one, the K split in several ranges."""
    out = geoms[0]
    for tails, U in ((FIT_TAILS, 8), (TAILS, 4)):
        several, one = set(), set()
        for n, claim in tails.items():
            g = out[(n, 1)]
            assert g["tail"] == claim and g["split_S"] > 1 and g["route"] == 1, (n, g)
            (several if claim[0] != claim[1] else one).update(claim)
        assert several == {U - 1, U, U + 1} and one == {U - 1, U, U + 1}, (U, several, one)
