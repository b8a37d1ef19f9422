"""The ordered path's launch list, pinned (patrol_amd/csrc/phip_engine.hip,
the schedule above ordered()).

GPURepo.timings() lists one call's launches in host issue order.  Every case
pins the first name and the whole list from "radix_sort_pairs" on (the resolve
and insert launches between them depend on the table), for one class of batch
each: thread folds only, long segments, one huge chain, the split onto the
third stream, and the egress or the change-set marks behind the folds, in the
mixed-kind and the uniform form.  Every case also compares its results with
the oracle, as tests/test_fold_directed.py does.
"""
import collections
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _egress_cases as EC  # noqa: E402
from tests import _fold_cases as F  # noqa: E402
from tests.test_fold_directed import assert_replies, check_case, first_diff  # noqa: E402

FIRST = "k_pack_ops"
THREAD = ["radix_sort_pairs", "segments", "k_fold_thread"]
LONG = THREAD + ["k_fold_wave"]
EGRESS = ["k_egress_count", "k_egress_scan", "k_egress_write"]
HUGE = ["radix_sort_pairs", "segments", "k_gather_huge", "k_fold_block", "k_huge_outputs"]
HUGE2 = ["k_gather_huge2", "k_fold_block2", "k_huge_outputs2"]
REST = ["k_fold_thread", "k_fold_wave"]


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def assert_launches(launched, tail):
    print("launched:", launched)
    assert launched[0] == FIRST
    assert launched.count("radix_sort_pairs") == 1
    assert launched[launched.index("radix_sort_pairs"):] == tail


@functools.lru_cache(maxsize=None)
def batch(which):
    """-> (ops, the oracle's results, its dump afterwards), computed once."""
    if which == "distinct":     # 300 Takes on 300 names: no segment over kLongSeg ops
        ops = EC.gen_ops(np.random.default_rng(300), 300, [b"d%d" % i for i in range(300)],
                         all_take=True)
        ops["names"] = [b"d%d" % i for i in np.random.default_rng(301).permutation(300)]
    else:                       # 3000 ops on 20 names: several long segments, none huge
        ops = EC.gen_ops(np.random.default_rng(3000), 3000, EC.name_pool(20),
                         all_take=which == "takes")
    o = O.Repo()
    ref = EC.call(o, ops)
    return ops, ref, o.dump()


def run_ops(pa, which, mode):
    """The batch on a fresh handle, as a host batch on the large path; mode:
    plain, egress, or tracked (a handle that keeps a change set)."""
    ops, ref, dump = batch(which)
    g = pa.GPURepo(log2_slots=12, small=False, track_changes=mode == "tracked")
    try:
        g.set_timing(True)
        out = g.apply_mixed(ops["kind"], ops["names"], ops["now"], ops["freq"], ops["per"],
                            ops["count"], ops["added"], ops["taken"], ops["elapsed"],
                            egress=mode == "egress")
        launched = [name for name, _ in g.timings()]
        g.set_timing(False)
        assert first_diff(out["status"], ref["status"]) is None
        assert first_diff(out["remaining"], ref["remaining"]) is None
        take = ops["kind"] == F.TAKE
        assert first_diff(out["have"][take], ref["have"][take]) is None
        assert assert_replies(out, ref, ops["kind"]) > 0
        gd = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}
        assert len(g) == len(gd) and gd == dump
        if mode != "plain":
            # the batch's datagrams, leaving with it or drained from the change set
            eg = out["egress"] if mode == "egress" else g.export_changed(1 << 12)
            assert mode == "egress" or eg["done"]
            want_req, want_st = EC.expected_datagrams(ops, ref, dump)
            assert eg["n_incast"] == len(want_req) and eg["n"] == len(want_req) + len(want_st)
            assert EC.sections(eg) == (want_req, want_st)
        return ops, launched
    finally:
        g.close()


def long_segments(ops):
    """Buckets with more than kLongSeg ops (more than one: the partition runs)."""
    return sum(c > F.LONG_SEG for c in collections.Counter(ops["names"]).values())


def test_thread_folds_only(pa):
    ops, launched = run_ops(pa, "distinct", "plain")
    assert len(set(ops["names"])) == 300
    assert_launches(launched, THREAD)


BEHIND = {"plain": [], "egress": EGRESS, "tracked": ["k_changes_mark"]}


@pytest.mark.parametrize("mode", ["plain", "egress", "tracked"])
def test_long_segments_mixed_kinds(pa, mode):
    """Mixed kinds meet segments over kLongSeg ops: k_egress_wants runs in
    front of what runs behind the folds."""
    ops, launched = run_ops(pa, "mixed", mode)
    assert long_segments(ops) > 1 and len(set(ops["kind"])) == 3
    assert_launches(launched, LONG + (["k_egress_wants"] if mode != "plain" else []) + BEHIND[mode])


@pytest.mark.parametrize("mode", ["egress", "tracked"])
def test_long_segments_all_takes(pa, mode):
    """A host batch of one kind takes the uniform form: no k_egress_wants."""
    ops, launched = run_ops(pa, "takes", mode)
    assert long_segments(ops) > 1 and set(ops["kind"]) == {F.TAKE}
    assert_launches(launched, LONG + BEHIND[mode])


@pytest.mark.parametrize("h", [1, F.HUGE_FIRST + 1])
def test_huge_chains(pa, h):
    """One huge segment: one chain on the second stream; PHIP_HUGE_FIRST + 1:
    the chain of the rest, on the third stream, is issued right behind it."""
    _, launched = check_case(pa, F.case_count(h), timing=True)
    assert_launches(launched, HUGE + (HUGE2 if h > F.HUGE_FIRST else []) + REST)
