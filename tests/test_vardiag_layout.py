"""vardiag_geom_of (pls_amd/csrc/vardiag_layout.hpp), the pure function that chooses the tile, the row splits, the component ranges
and the workspace of pls_hip_var_diagnostics, checked without a GPU: the header is plain C++, tests/cpp/vardiag_layout.cpp includes it
alone, is built with ASan + UBSan and run as a process of its own.  For every shape of tests/test_gpu_vardiag.py and a sweep of
shapes around the tile's edges it holds that every (row tile, column block) has exactly one owner, that the partials of a range fill
the planned buffer cell by cell, and that the ranges cover 1..A."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (N, K, A, element size) -- the shapes of the GPU test and the three of the speed comparison
SHAPES = {"one-row": (1, 7, 3, 8), "small": (9, 7, 3, 8), "edge": (129, 65, 13, 8), "tails": (1031, 513, 12, 8),
          "split": (40000, 64, 13, 8), "wide": (60, 4000, 6, 8), "nir": (60, 401, 10, 8), "f32": (1031, 64, 10, 4),
          "a-eq-k": (1000, 7, 7, 8), "two-ranges": (300, 64, 30, 8), "config3": (1 << 20, 512, 20, 8),
          "config4-f32": (131072, 4096, 50, 4), "short-wide": (2000, 100000, 10, 8)}


@pytest.fixture(scope="module")
def geoms(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vardiag_layout") / "vardiag_layout")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "vardiag_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = "".join(f"{n} {s[0]} {s[1]} {s[2]} {s[3]}\n" for n, s in SHAPES.items())
    p = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    out, swept = {}, 0
    for l in p.stdout.splitlines():
        f = l.split()
        if f[0] == "swept":
            swept = int(f[1])
        else:
            out[(f[0], int(f[1]))] = dict(zip(("vec", "NT", "CB", "RS", "nranges", "AS", "part", "st", "msg", "one"), map(int, f[2:])))
    return out, swept


def geom_of(geoms, name, aligned=1):
    return geoms[0][(name, aligned)]


def test_every_tile_is_owned_once_and_the_partials_fill_their_buffer(geoms):
    """the program's own checks passed (its exit status) on every shape named here, aligned and not, and on its sweep"""
    out, swept = geoms
    assert len(out) == 2 * len(SHAPES) and swept > 5000, (len(out), swept)


def test_the_tile_and_the_splits_of_the_named_shapes(geoms):
    for n, (N, K, A, es) in SHAPES.items():
        for al in (0, 1):
            g = geom_of(geoms, n, al)
            assert g["NT"] == -(-N // 128) and g["CB"] == -(-K // 64), (n, g)
            assert g["vec"] == (16 // es if al else 1)
            assert g["nranges"] == -(-A // 24) and g["AS"] == -(-A // 4) * 4
            assert 1 <= g["RS"] <= g["NT"]
            assert g["part"] == g["RS"] * (min(A, 24) + 1) * K * 8
            assert g["msg"] == A + K * (A + 1) and g["one"] == 1
    assert geom_of(geoms, "split")["RS"] > 1          # 40,000 x 64: one column block, the rows are split
    assert geom_of(geoms, "config3")["RS"] == 64      # 8 column blocks x 64 splits = two workgroups per CU
    assert geom_of(geoms, "wide")["RS"] == 1 and geom_of(geoms, "short-wide")["RS"] == 1
    assert geom_of(geoms, "two-ranges")["nranges"] == 2 and geom_of(geoms, "config4-f32")["nranges"] == 3
