"""Without a GPU: the catalogue of tests/stream_order.py covers every compute entry point that include/pls_hip.h declares, and its
*enqueues* / *completes* marks are the ones of the header's "Stream order" table -- the mark follows the header, never the other way
round."""
import os
import re

import stream_order as so
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "pls_hip.h")).read()
DECLARED = re.findall(r"^PLS_HIP_API\s+[^;(]*?\b(pls_hip_\w+)\s*\(", HEADER, re.M)

# declared, and deliberately not in the catalogue
EXEMPT = {
    "pls_hip_abi_version": "lifetime: no handle, no stream",
    "pls_hip_create": "lifetime: takes the stream",
    "pls_hip_destroy": "lifetime: test_close_with_work_pending",
    "pls_hip_set_stream": "lifetime: test_set_stream_with_work_pending",
    "pls_hip_set_option": "options: host state only",
    "pls_hip_get_option": "options: host state only",
    "pls_hip_set_reducer": "reducer setter: row-sharded handles are a later change",
    "pls_hip_get_reducer": "reducer setter: host state only",
    "pls_hip_set_reduce_buffer": "reducer setter: row-sharded handles are a later change",
    "pls_hip_synchronize": "lifetime: the synchronisation itself, called behind every sandwich",
    "pls_hip_last_error": "host state only",
    "pls_hip_get_timing": "reads the events of profiled launches: synchronises by design, used by every baseline",
    "pls_hip_matrix_shape": "group family: a later change",
    "pls_hip_matrix_block": "group family: a later change",
}
EXEMPT_FAMILIES = {"pls_hip_xchg_": "the cross-process exchange: a later change",
                   "pls_hip_group_": "groups run member streams and host threads of their own: a later change"}


def _exempt(name):
    return name in EXEMPT or any(name.startswith(f) for f in EXEMPT_FAMILIES)


def test_the_header_parses():
    assert len(DECLARED) >= 55 and len(set(DECLARED)) == len(DECLARED), len(DECLARED)
    assert "pls_hip_fit" in DECLARED and "pls_hip_colwise_z_scores_missing" in DECLARED and "pls_hip_group_cv_folds" in DECLARED


def test_every_declared_entry_point_is_in_the_catalogue_or_exempt():
    covered = {c.entry for c in so.CASES}
    assert covered <= set(DECLARED), covered - set(DECLARED)
    for name in DECLARED:
        assert (name in covered) != _exempt(name), f"{name}: {'both covered and exempt' if name in covered else 'neither in the catalogue nor exempt'}"
    assert all(e in DECLARED for e in EXEMPT), [e for e in EXEMPT if e not in DECLARED]


def test_every_mark_is_the_headers():
    table = so.header_table(HEADER)
    assert len(table) >= 22, sorted(table)
    rows = {c.row for c in so.CASES}
    assert rows == set(table), (rows ^ set(table))
    for c in so.CASES:
        assert c.mark == table[c.row][0], (c.name, c.mark, table[c.row])
        assert c.row.split(",")[0] == c.entry, c.name
    # host memory: every call completes; "-" exactly where the entry has no `mem` argument
    for row, (dev, host) in table.items():
        entry = row.split(",")[0]
        decl = re.search(rf"PLS_HIP_API\s+int\s+{entry}\s*\(([^;]*)\)\s*;", HEADER).group(1)
        assert (host == "-") == (re.search(r"\bint\s+mem\b", decl) is None), row
        assert host in ("completes", "-"), row


def test_every_entry_point_with_a_storage_type_has_an_fp32_case():
    for entry in {c.entry for c in so.CASES}:
        decl = re.search(rf"PLS_HIP_API\s+int\s+{entry}\s*\(([^;]*)\)\s*;", HEADER).group(1)
        if re.search(r"\bint\s+dtype\b", decl):
            assert any(c.f32 for c in so.CASES if c.entry == entry), f"{entry} takes a storage type and has no fp32 case"
        else:
            assert not any(c.f32 for c in so.CASES if c.entry == entry), entry


def test_the_catalogue_names_its_cases_once_and_groups_them_by_entry_point():
    names = [c.name for c in so.CASES]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    for c in so.CASES:
        assert c.group.split(":")[0] == c.entry and c.kind in so.KIND_NAMES, c.name
    # the host-memory test lists exactly the entries that take `mem`
    import test_gpu_stream_order as T
    with_mem = [e for e in DECLARED if not _exempt(e) and
                re.search(r"\bint\s+mem\b", re.search(rf"PLS_HIP_API\s+int\s+{e}\s*\(([^;]*)\)\s*;", HEADER).group(1))]
    assert sorted(T.HOST_ENTRIES) == sorted(with_mem)
