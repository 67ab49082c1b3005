"""xdiagmiss_geom_of (pls_amd/csrc/xdiagmiss_layout.hpp), the pure function that chooses the route, the tile, the K split and the
workspace of pls_hip_x_diagnostics_missing, checked without a GPU: the header is plain C++, tests/cpp/xdiagmiss_layout.cpp includes
it alone, is built with ASan + UBSan and run as a process of its own.  It holds every case of tests/test_xdiag_missing_ref.py to the
route and the tile rows the case claims, the tile to the on-chip budget, the workspace below 4 GB and the K split to covering K
exactly -- for the cases and for a sweep of shapes around the thresholds."""
import os
import subprocess

import pytest

from test_xdiag_missing_ref import CASES, RESIDENT

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
    swept = 0
    for l in p.stdout.splitlines():
        f = l.split()
        if f[0] == "swept":
            swept = int(f[1])
        else:
            out[(f[0], int(f[1]))] = dict(route=int(f[2]), rt=int(f[3]), S=int(f[4]), kper=int(f[5]), ws=int(f[6]))
    return out, swept


def test_every_case_lies_on_the_route_it_claims(geoms):
    out, swept = geoms
    assert len(out) == 2 * len(CASES) and swept > 1000
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
