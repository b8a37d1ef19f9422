"""The hot-bucket block fold's arithmetic on the CPU (no GPU needed).

oracle/fold_model is built from the kernel header itself: the pure functions
k_fold_block runs (step_sop, window_quiet, window_absorbable, join_state,
state_grew, ...) compiled for the host.  Here
  * its `sweep` checks the two window predicates against the sequential fold
    over random windows and the constructed family at the absorbing bound;
  * its `replay` of every directed stream (tests/_fold_cases.py) equals the
    oracle bit for bit -- the kernel's per-op code under the oracle -- and
    its JSON shows that the stream still reaches the path it was written for;
  * the constants the stream builders use equal the header's.
This says nothing about gfx950's own NaN behaviour: tests/test_fold_directed.py
runs the same streams on the GPU.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import _fold_cases as F
from tests import _gen

# the committed sweep: N windows, seed (about 3 s; `make -C oracle` builds the binary)
SWEEP_N, SWEEP_SEED = 2_000_000, 1


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(F.MODEL):
        subprocess.run(["make", "-s", "-C", os.path.dirname(F.MODEL), "fold_model"], check=True)
    return F.MODEL


def test_sweep_predicates_sound_and_not_vacuous(model):
    p = subprocess.run([model, "sweep", str(SWEEP_N), str(SWEEP_SEED)], capture_output=True,
                       text=True)
    assert p.returncode == 0, (p.stdout, p.stderr[-3000:])
    J = json.loads(p.stdout)
    print(J)
    assert J["violations"] == 0 and J["samples"] == SWEEP_N and J["family"] > 1000
    # the floors, on windows that hold Takes (the others are absorbable trivially)
    assert J["absorbable_with_takes"] * 10 >= SWEEP_N, J
    assert J["quiet_with_takes"] * 100 >= SWEEP_N, J
    assert J["absorbable_only_raised"] * 100 >= SWEEP_N, J


def test_builder_constants_match_the_header():
    with open(os.path.join(F.ROOT, "patrol_amd", "csrc", "phip_kernels.hpp")) as f:
        src = f.read()

    def macro(name):
        return int(re.search(r"^#define %s (\d+)\b" % name, src, re.M).group(1))

    def const(name):
        return int(re.search(r"^constexpr u32 %s = (\d+);" % name, src, re.M).group(1))

    assert macro("PHIP_HUGE_SEG") == F.HUGE_SEG
    assert macro("PHIP_FOLD_THREADS") == F.FOLD_THREADS
    assert macro("PHIP_FOLD_PER") == F.FOLD_PER
    assert macro("PHIP_HUGE_FIRST") == F.HUGE_FIRST
    assert const("kBurstQuiet") == F.BURST_QUIET
    assert const("kLongSeg") == F.LONG_SEG
    # what the builders derive from them
    assert re.search(r"^constexpr u32 kFoldWin = kFoldThreads \* kFoldPer;", src, re.M)
    assert re.search(r"^constexpr u32 kSumChunk = kFoldThreads;", src, re.M)
    assert F.SUM_CHUNK_OPS == 262144 and F.FOLD_WIN == 512


def check_replay_vs_oracle(model, tmp_path, case, ref, dump, k):
    """The k-th hot bucket of the case: replay == oracle on every output."""
    name, idx = case.hot[k]
    seed, cols = F.segment_of(case, k)
    J, out = F.replay(tmp_path, seed, cols, "seg%d" % k)
    assert J["violations"] == 0 and J["window"] == F.FOLD_WIN, J
    assert np.array_equal(out["status"], ref["status"][idx]), name
    assert np.array_equal(out["remaining"], ref["remaining"][idx]), name
    take = cols[0] == F.TAKE
    assert np.array_equal(out["have"][take], ref["have"][idx][take]), name
    rep = out["has_reply"].astype(bool)
    st = ref["status"][idx] & 0x7F
    assert np.array_equal(rep, take | (cols[0] == F.UPSERT) | (st == 2) | (st == 3)), name
    for f in ("reply_added", "reply_taken", "reply_elapsed", "reply_created"):
        assert np.array_equal(out[f][rep], ref[f][idx][rep]), (name, f)
    assert out["existed"] == 1 and tuple(int(x) for x in out["final"]) == dump[name], name
    return J, out


def run_case(model, tmp_path, case):
    o = O.Repo()
    case.seed_into(o)
    ref = o.apply_mixed(*case.args)
    dump = o.dump()
    first = None
    for k in range(len(case.hot)):
        J, out = check_replay_vs_oracle(model, tmp_path, case, ref, dump, k)
        if k == 0:
            first = (J, out)
    J, out = first
    print(case.name, json.dumps(J))
    case.check(J, out["status"])
    return J


@pytest.mark.parametrize("cid", list(F.CASES))
def test_directed_stream_replay_equals_oracle_and_shows_its_property(model, tmp_path, cid):
    run_case(model, tmp_path, F.CASES[cid]())


@pytest.mark.parametrize("h", F.COUNTS)
def test_segment_count_streams_replay_equals_oracle(model, tmp_path, h):
    case = F.case_count(h)
    assert [len(idx) for _, idx in case.hot] == [F.HUGE_SEG + 1 + F.FOLD_WIN * i for i in range(h)]
    run_case(model, tmp_path, case)


def test_bound_edge_classification_differs(model, tmp_path):
    """bound + 1 is absorbed, bound and bound - 1 are folded with the Take granted."""
    got = {}
    for d in (-1, 0, 1):
        case = F.case_bound(d)
        seed, cols = F.segment_of(case)
        J, out = F.replay(tmp_path, seed, cols, "b%d" % (d + 1))
        got[d] = (J["classes"][case.marks["window"]], int(out["status"][case.marks["take"]]))
    assert got == {-1: ("F", F.ST_TAKE_OK), 0: ("F", F.ST_TAKE_OK), 1: ("A", F.ST_TAKE_DENIED)}, got


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_dirty_states_stream_replay_equals_oracle(model, tmp_path, seed):
    """One bucket, every op kind, _gen.dirty_states replicas (-0.0, NaN, Inf,
    negatives, incasts), odd rates: the per-op code against the oracle."""
    rng = np.random.default_rng(900 + seed)
    n = 20000
    kind = rng.choice(np.array([0, 1, 2], np.uint8), n, p=[0.5, 0.4, 0.1])
    now = _gen.T0 + np.arange(n, dtype=np.int64) * 20_000 + rng.integers(-10**6, 10**6, n)
    freq = np.full(n, 100, np.int64)
    per = np.full(n, _gen.SEC, np.int64)
    odd = rng.random(n) < 0.05
    freq[odd] = rng.choice([0, 3, 7, -5, 1 << 40], int(odd.sum()))
    per[odd] = rng.choice([_gen.SEC, 1, 0, 60 * _gen.SEC], int(odd.sum()))
    cnt = np.ones(n, np.uint64)
    cnt[rng.random(n) < 0.05] = 3
    a, t, e = _gen.dirty_states(rng, n, 0.02 * seed)
    if seed == 3:      # keep tokens in play, as _mixed_stream does
        a = (a.view(np.float64) / 1e4).view(np.uint64).copy()
        t = (t.view(np.float64) / 1e4).view(np.uint64).copy()
        e = e >> 12
    names = [b"one"] * n
    o = O.Repo()
    ref = o.apply_mixed(kind, names, now, freq, per, cnt, a, t, e)

    class C:
        hot = [(b"one", np.arange(n))]
        seeds = {b"one": None}
        args = [kind, names, now, freq, per, cnt, a, t, e]
    J, _ = check_replay_vs_oracle(model, tmp_path, C, ref, o.dump(), 0)
    assert J["exact"]["why"] != "never" and J["take_ok"] > 0 and J["incast_reply"] > 0, J
