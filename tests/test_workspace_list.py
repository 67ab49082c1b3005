"""The handle's workspaces are ONE list (pls_amd/csrc/ctx.hpp, PLS_HIP_WORKSPACES): pls_hip_destroy frees from it and the testing
build's pls_hip_test_poison_workspace fills from it.  A DevBuf member added to pls_hip_context and left out of the list would be
leaked by the one and never poisoned by the other (tests/test_gpu_history.py would then not see a stale read of it), so the struct
and the list are held to each other here, from the text of the header: no compiler, no GPU."""
import os
import re

from conftest import ROOT

CTX = os.path.join(ROOT, "pls_amd", "csrc", "ctx.hpp")


def parse(path=CTX):
    """(members, entries): the DevBuf members of pls_hip_context in order of declaration, and the list's entries as
    (name, kind, keep, reason) with kind "scratch" / "stateful" (keep and reason None for scratch)"""
    text = open(path).read()
    m = re.search(r"^struct pls_hip_context \{\n(.*?)^\};", text, re.S | re.M)
    assert m, "struct pls_hip_context not found"
    members = []
    for decl in re.findall(r"^\s*DevBuf\s+([^;()]+);", m.group(1), re.M):
        members += [n.strip() for n in decl.split(",")]
    assert all(re.fullmatch(r"\w+", n) for n in members), members
    m = re.search(r"^#define PLS_HIP_WORKSPACES\(SCRATCH, STATEFUL\)(.*?[^\\])\n", text, re.S | re.M)
    assert m, "PLS_HIP_WORKSPACES not found"
    body = m.group(1)
    entries = []
    for e in re.finditer(r'\b(SCRATCH|STATEFUL)\(\s*(\w+)\s*(?:,(.*?),\s*"((?:[^"\\]|\\.)*)"\s*)?\)', body):
        kind, name, keep, reason = e.groups()
        if kind == "SCRATCH":
            assert keep is None, f"SCRATCH({name}) takes the name alone"
            entries.append((name, "scratch", None, None))
        else:
            assert keep is not None, f"STATEFUL({name}) needs (name, keep, \"reason\")"
            entries.append((name, "stateful", keep.strip(), reason))
    # nothing in the list's text that the pattern above did not take for an entry
    assert len(re.findall(r"\b(?:SCRATCH|STATEFUL)\(", body)) == len(entries), "an entry of PLS_HIP_WORKSPACES did not parse"
    return members, entries


def check(path=CTX):
    members, entries = parse(path)
    assert len(members) >= 90 and len(set(members)) == len(members), members
    names = [e[0] for e in entries]
    missing = [n for n in members if n not in names]
    extra = [n for n in names if n not in members]
    twice = sorted({n for n in names if names.count(n) > 1})
    assert not missing, f"DevBuf members of pls_hip_context missing from PLS_HIP_WORKSPACES (never freed, never poisoned): {missing}"
    assert not extra, f"PLS_HIP_WORKSPACES names no DevBuf member of pls_hip_context: {extra}"
    assert not twice, f"listed more than once (freed twice): {twice}"
    return members, entries


def test_every_devbuf_member_is_listed_exactly_once():
    check()


def test_every_stateful_mark_has_a_reason():
    _, entries = check()
    stateful = [e for e in entries if e[1] == "stateful"]
    assert stateful, "no stateful entry at all: zeros, the resident counters and the epoch words are"
    for name, _, keep, reason in stateful:
        assert keep, name
        assert reason and len(reason.split()) >= 8, f"STATEFUL({name}): the reason is missing or says nothing: {reason!r}"
    print(f"{len(entries) - len(stateful)} scratch, {len(stateful)} stateful: {[e[0] for e in stateful]}")


def test_destroy_and_the_poisoner_walk_the_list():
    """no second, hand-written array of the buffers beside the list"""
    src = open(os.path.join(ROOT, "pls_amd", "csrc", "pls_hip.hip")).read()
    destroy = src[src.index("int pls_hip_destroy("):src.index("int pls_hip_set_stream(")]
    assert "for_each_workspace(" in destroy and "DevBuf *bufs[]" not in destroy
    poison = src[src.index("pls_hip_test_poison_workspace("):src.index("int pls_hip_create(")]
    assert "for_each_workspace(" in poison
    # ... and the poisoner is in the testing build only, outside the public header
    assert src.index("#ifdef PLS_HIP_TESTING") < src.index("pls_hip_test_poison_workspace(") < src.index("#endif")
    assert "pls_hip_test_" not in open(os.path.join(ROOT, "include", "pls_hip.h")).read()


def test_the_check_notices_a_member_left_out(tmp_path):
    """a copy of the header with one entry taken out of the list fails the check (the buffer that would leak is named)"""
    import pytest
    text = open(CTX).read()
    assert text.count("SCRATCH(valhist) ") == 1
    broken = tmp_path / "ctx.hpp"
    broken.write_text(text.replace("SCRATCH(valhist) ", ""))
    with pytest.raises(AssertionError, match="valhist"):
        check(str(broken))
