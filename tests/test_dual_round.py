"""The workspace slabs of the sample-space rounds, checked without a GPU: ItemLayout (pls_amd/csrc/dual_layout.hpp) is plain
C++, so the byte count that sizes a round and the addresses the kernels are given -- both derived from it -- can be compared
on the CPU with the closed forms and the pointer chains the four plans carried before they shared it.
tests/cpp/dual_round.cpp, built with ASan + UBSan, lays the slabs out and touches both ends of every field."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 1, 1, 1, 1), (37, 3, 4, 5, 3), (8192, 32, 64, 100, 7)]  # (N, M, A, ts, nround)

# bytes of one item: the closed forms of cv_dual_fold_bytes, batch_dual_problem_doubles, resample_item_doubles and
# cvbatch_item_doubles as the plans had them
BYTES = {
    "cv": lambda N, M, A, ts: (2 * N * M + N * A + 2 * A + N + ts * M) * 8 + N * 4,
    "batch": lambda N, M, A, ts: (2 * N * M + 2 * N * A + A * A + M * A + A + N + A) * 8,
    "resample": lambda N, M, A, ts: ((2 * N * M + 2 * N * A + A * A + M * A + A + N + A) + N + N * M) * 8,
    "cvbatch": lambda N, M, A, ts: (2 * N * M + N * A + A + N + A + 3 * ts * M + M * A + M) * 8,
}
# the fields in the order of the plans' pointer chains, with the bytes of one item's share
_BATCH = [("Ya", lambda N, M, A, ts: N * M * 8), ("Z", lambda N, M, A, ts: N * M * 8), ("T", lambda N, M, A, ts: N * A * 8),
          ("U", lambda N, M, A, ts: N * A * 8), ("C", lambda N, M, A, ts: A * A * 8), ("Q", lambda N, M, A, ts: M * A * 8),
          ("tt", lambda N, M, A, ts: A * 8), ("scr", lambda N, M, A, ts: (N + A) * 8)]
_CV = [("Ya", lambda N, M, A, ts: N * M * 8), ("Z", lambda N, M, A, ts: N * M * 8), ("T", lambda N, M, A, ts: N * A * 8),
       ("tt", lambda N, M, A, ts: A * 8), ("scr", lambda N, M, A, ts: (N + A) * 8), ("pred", lambda N, M, A, ts: ts * M * 8)]
FIELDS = {
    "cv": _CV + [("pos", lambda N, M, A, ts: N * 4)],
    "batch": _BATCH,
    "resample": _BATCH + [("s", lambda N, M, A, ts: N * 8), ("Yin", lambda N, M, A, ts: N * M * 8)],
    "cvbatch": _CV + [("yte", lambda N, M, A, ts: ts * M * 8), ("escr", lambda N, M, A, ts: ts * M * 8),
                      ("press", lambda N, M, A, ts: M * A * 8), ("ssy", lambda N, M, A, ts: M * 8)],
}


@pytest.fixture(scope="module")
def slabs(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dual_round") / "dual_round")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "dual_round.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], input="".join(" ".join(map(str, c)) + "\n" for c in CASES), capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = [l.split() for l in p.stdout.splitlines()]
    assert len(lines) == 4 * len(CASES)
    out = {}
    for i, l in enumerate(lines):
        out[(CASES[i // 4], l[0])] = (int(l[1]), [(f.split(":")[0], int(f.split(":")[1])) for f in l[2:]])
    return out


@pytest.mark.parametrize("layout", sorted(FIELDS))
@pytest.mark.parametrize("case", CASES)
def test_bytes_per_item_is_the_closed_form(slabs, case, layout):
    assert slabs[(case, layout)][0] == BYTES[layout](*case[:4])


@pytest.mark.parametrize("layout", sorted(FIELDS))
@pytest.mark.parametrize("case", CASES)
def test_fields_keep_their_order_and_tile_the_slab(slabs, case, layout):
    per_item, got = slabs[(case, layout)]
    nround = case[4]
    assert [n for n, _ in got] == [n for n, _ in FIELDS[layout]]  # the order of the pointer chains
    at = 0  # contiguous from the base: every field begins where the one before it ends, so no two overlap
    for (name, off), (_, size) in zip(got, FIELDS[layout]):
        assert off == at, (name, off, at)
        assert size(*case[:4]) > 0
        at += nround * size(*case[:4])
    assert at == nround * per_item  # ... and the last one ends with the slab
