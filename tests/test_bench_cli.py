"""bench.py as a command: a plain run at a small size with --dump-outputs.

One run (a 10k-bucket table, 100k messages per step) whose 9 steps do not
fit its 3-batch pool, so the batches are recycled twice:
* the line carries the fields a driver reads, `steps` is the number asked
  for, and a plain run carries none of --full's objects;
* the dump is float32/float64 .npy files of at most 64 MB;
* every status is "merged", and the hottest bucket (id 0, named in every
  batch) holds a state of the last step: replica_states() draws step j's
  taken from [j * 2e6, j * 2e6 + 1e6) and its elapsed from
  [j * 2^40, (j + 1) * 2^40), so a recycled batch that was not moved up, or
  a last step that did not run, leaves an earlier step's range there.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, STEPS, WARMUP, POOL = 100_000, 10_000, 7, 2, 3


def _bench(*more):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--keys", str(K), "--messages", str(N), "--log2-slots", "15",
           "--pool-bytes", str(POOL * 24 * N), *more]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    return _bench("--dump-outputs", str(out)), out


def test_full_owner_routed_recycles_too():
    """--full with more steps than batches fit: the owner_routed object (the
    one extra leg that runs --steps steps) recycles its pool as the headline
    does, and the run exits 0.  The other objects have fixed sizes of their
    own and are left out here."""
    d = _bench("--full", "--no-cpu", "--no-variants", "--no-c3", "--no-c4", "--no-ae")
    assert d["config"]["full"] is True and d["steps"] == STEPS
    o = d["owner_routed"]
    assert "error" not in o, o
    assert o["ms_per_step"] > 0 and o["messages_per_step_total"] == N
    assert o["value"] == pytest.approx(N / (o["ms_per_step"] / 1e3), rel=1e-9)
    assert 0 < o["merged_per_step_total"] <= N


def test_plain_line(run):
    d, _ = run
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["config"]["batches_in_hbm"] == POOL and d["config"]["full"] is False
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert d["roofline"]["launches_per_step"] == 1.0     # every step's kernels were counted
    assert d.get("cpu_baseline") is None
    for key in ("owner_routed", "c2_variants", "c3", "c4", "anti_entropy"):
        assert key not in d


def test_dump(run):
    _, out = run
    files = sorted(os.listdir(out))
    assert files == sorted(f"{n}.npy" for n in ("status", "status_index", "status_counts",
                                                "bucket_ids", "added", "taken", "elapsed"))
    arr = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    assert np.array_equal(arr["status_index"], np.arange(N))
    assert (arr["status"] == 1).all()                     # PHIP_ST_MERGED
    assert arr["status_counts"][1] == N and arr["status_counts"].sum() == N
    assert np.array_equal(arr["bucket_ids"], np.arange(K))
    last = WARMUP + STEPS - 1
    assert last * 2e6 <= arr["taken"][0] < last * 2e6 + 1e6
    assert arr["taken"][0] <= arr["added"][0] <= arr["taken"][0] + 100.0 + 1e6
    assert last * 2.0**40 <= arr["elapsed"][0] < (last + 1) * 2.0**40
    # no bucket is ahead of the last step, and added >= taken wherever a message landed
    assert arr["taken"].max() < last * 2e6 + 1e6 and arr["elapsed"].max() < (last + 1) * 2.0**40
    assert (arr["added"] >= arr["taken"]).all()
