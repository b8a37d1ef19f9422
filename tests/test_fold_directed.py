"""Directed parity tests of the hot-bucket block fold on cuda:0.

Every stream of tests/_fold_cases.py (segment lengths on the fold's
thresholds, 1 / 8 / 9 / 17 hot segments, and windows built to land on each
decision k_fold_block makes) through GPURepo.apply_mixed (host arrays, the
large path) against the oracle from the same seeded buckets: status,
remaining, have on Takes, every reply state and the whole table, bit for bit.
tests/test_fold_model.py shows on the CPU that each stream reaches the path it
was written for.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _fold_cases as F  # noqa: E402


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def reply_mask(kind, status):
    """Ops whose reply state is written (include/patrolhip.h): Takes, Upserts
    and incast requests."""
    st = np.asarray(status) & 0x7F
    kind = np.asarray(kind)
    return (kind == F.TAKE) | (kind == F.UPSERT) | (st == F.ST_INCAST_REPLY) | \
        (st == F.ST_INCAST_NOREPLY)


def assert_replies(out, ref, kind):
    rep = reply_mask(kind, ref["status"])
    r = out["reply"][rep]
    for f, k in (("a", "reply_added"), ("t", "reply_taken"), ("e", "reply_elapsed"),
                 ("c", "reply_created")):
        bad = np.nonzero(r[f] != ref[k][rep])[0]
        assert bad.size == 0, (f, int(np.nonzero(rep)[0][bad[0]]), bad.size)
    return int(rep.sum())


def first_diff(x, y):
    bad = np.nonzero(np.asarray(x) != np.asarray(y))[0]
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


def check_case(pa, case, log2_slots=12, timing=False):
    g = pa.GPURepo(log2_slots=log2_slots)
    o = O.Repo()
    case.seed_into(g)
    case.seed_into(o)
    if timing:
        g.set_timing(True)
    out = g.apply_mixed(*case.args)
    launched = [name for name, _ in g.timings()] if timing else None
    ref = o.apply_mixed(*case.args)
    kind = case.args[0]
    assert first_diff(out["status"], ref["status"]) is None
    assert first_diff(out["remaining"], ref["remaining"]) is None
    take = kind == F.TAKE
    assert first_diff(out["have"][take], ref["have"][take]) is None
    assert assert_replies(out, ref, kind) > 0
    gd = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}
    od = o.dump()
    assert len(g) == len(gd) == len(od)
    bad = [k for k in od if gd.get(k) != od[k]]
    assert not bad, [(k, gd.get(k), od[k]) for k in bad[:5]]
    g.close()
    return ref, launched


@pytest.mark.parametrize("cid", list(F.CASES))
def test_directed_stream_vs_oracle(pa, cid):
    case = F.CASES[cid]()
    ref, _ = check_case(pa, case)
    if cid == "absorbed":      # incast replies there carry the joined state (compared above)
        _, idx = case.hot[0]
        assert ((ref["status"][idx] & 0x7F) == F.ST_INCAST_REPLY).sum() > 100


@pytest.mark.parametrize("h", F.COUNTS)
def test_segment_count_second_stream_vs_oracle(pa, h):
    """1, PHIP_HUGE_FIRST, PHIP_HUGE_FIRST + 1 and 17 huge segments of distinct
    lengths, the longest last in name order: past PHIP_HUGE_FIRST the rest
    fold on a second stream (k_huge_order, k_fold_block2, k_huge_outputs2)."""
    case = F.case_count(h)
    _, launched = check_case(pa, case, timing=True)
    assert "k_fold_block" in launched and "k_huge_outputs" in launched, launched
    split = h > F.HUGE_FIRST
    assert ("k_fold_block2" in launched) == split, launched
    assert ("k_huge_outputs2" in launched) == split, launched
