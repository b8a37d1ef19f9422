"""The Take batcher's threading on the CPU (no GPU needed).

oracle/batcher_check links the product's phip_batcher.cpp and phip_host.cpp
against a model engine (the oracle behind phip_apply_mixed and
phip_apply_mixed_egress, with a log of every call) and drives the batcher from
native threads: arrival order against the oracle, max_batch against a 10 s
window, an engine error reaching exactly its batch's callers, close with
callers blocked, the egress ring's numbering, reuse, backpressure, several
drainers and misuse of egress_done, close with the ring full.  What each
scenario asserts is stated at its function in oracle/batcher_check.cpp.

Only the plain build runs here.  The ThreadSanitizer and ASan + UBSan builds of
the same program (oracle/Makefile) are run by hand on the CPU.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "oracle", "batcher_check")

SCENARIOS = ["order", "max_batch", "engine_error", "close_blocked", "egress_order",
             "zero_datagrams", "backpressure", "drainers", "done_misuse", "close_ring_full"]


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-s", "-C", os.path.dirname(CHECK), "batcher_check"], check=True)
    return CHECK


def test_every_scenario_is_run(check):
    p = subprocess.run([check, "list"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.split() == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_scenario(check, scenario):
    # the timeout is a hang guard, not a measurement: the program bounds what it times itself
    p = subprocess.run([check, scenario], capture_output=True, text=True, timeout=60)
    print(p.stdout.strip())
    assert p.returncode == 0, (p.stdout, p.stderr[-3000:])
    J = json.loads(p.stdout)
    assert J["scenario"] == scenario and J["ok"] is True and J["failures"] == 0, J
    assert J["requests"] > 0 and J["engine_calls"] > 0, J
