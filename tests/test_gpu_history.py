"""A handle's results do not depend on what it ran before (include/pls_hip.h, "History").

tools/history_probe.py, one child process per group of handles -- default, general (PLS_HIP_TINY=0), dual (ALGO_DUAL), host --
on pls_amd/csrc/testing/libpls_hip.so, which PLS_AMD_LIBRARY names when pls_amd is imported (so not in the suite's own process).
Every probe of its catalogue (the 14 routes of test_gpu_hard_data.py on its four shapes, three of them in fp32 storage as well;
the wider fit plans of test_gpu_edge.py; every other entry point once per route) asserts the route it took and is run
  * on a fresh handle: the SHA-256 of all its outputs and its launch counts are the baseline;
  * on ONE long-lived handle per kind, after pls_hip_test_poison_workspace has filled every scratch workspace -- and has every
    later allocation filled -- with 0xFF, 0x7F and 0x01 in turn, the probes in catalogue order and then in reverse;
  * (group "host", no poison) after options toggled and restored, graph capture and replay, X^T X taken during an upload, a
    changed stream, every refused call of test_bad_arguments_every_entry_point, the resident fits three times in a row and in
    turn, two handles on two streams taking turns.
Bit for bit: digest and launch counts equal the baseline's, no tolerance anywhere.  The driver also holds that no probe is
skipped, that something was poisoned before every probe but a handle's first, and that the poisoned byte count of a handle never
shrinks; it prints every probe with its route, baseline digest and the bytes poisoned before it (shown when the test fails, or
with pytest -s).

Nothing is cut: three bytes x two orders for every probe.
Single GPU only: sharded handles, groups and the cross-process exchange have recovery tests of their own (test_gpu_dist*.py);
the same treatment of their workspaces (the exchange's inboxes and flags are no DevBuf) is left to a later change.

The children run one after another, each under its own time limit; a child that ends abnormally (a signal, a time limit, an
exception) ends the test there -- the next one is not started."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GROUPS = ("default", "general", "dual", "host")
PROBES = {"default": 39, "general": 44, "dual": 17, "host": 0}   # the catalogue, by group: 100 probes


def test_results_do_not_depend_on_the_history_of_the_handle():
    env = dict(os.environ, PLS_AMD_LIBRARY=os.path.join(ROOT, "pls_amd", "csrc", "testing", "libpls_hip.so"))
    differ = []
    for group in GROUPS:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "history_probe.py"), group], env=env, capture_output=True, text=True,
                           timeout=240)
        print(r.stdout)
        tail = r.stdout[-3000:] + r.stderr[-3000:]
        assert r.returncode in (0, 1), f"group {group} ended abnormally ({r.returncode}):\n{tail}"   # (stop here: start nothing more)
        m = re.search(rf"^done: {group}: (\d+) probes, (\d+) runs, (\d+) differ$", r.stdout, re.M)
        assert m, f"group {group} did not finish:\n{tail}"
        nprobes, runs, bad = map(int, m.groups())
        assert nprobes == PROBES[group], (group, nprobes)
        if group != "host":   # baseline + 3 bytes x 2 orders of every probe, none skipped
            assert runs == 7 * nprobes, (group, runs)
            assert len(re.findall(r"^poison \[", r.stdout, re.M)) == 6 * nprobes, group
        else:
            assert runs >= 100, runs
        assert (bad == 0) == (r.returncode == 0), (group, bad, r.returncode)
        differ += re.findall(r"^DIFFERS.*$", r.stdout, re.M)
    assert not differ, "\n".join(differ)
