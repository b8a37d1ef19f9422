#!/usr/bin/env python3
"""The launches of the fast Receive path, scenario by scenario: for fixed
seeds, the timings() kernel-name list of each scenario as one JSON line.

Evidence for a change to the receive orchestration that must launch what the
parent launched: run once per library (PATROLHIP_LIB selects the .so, as in
tools/ab.sh) and compare the two outputs byte for byte.

Every scenario: 2^17 messages on a fresh 2^17-slot handle seeded with 20000
buckets (tests/test_receive_optimistic.py's shapes and its Batch helper).
Usage: python3 tools/receive_launches.py > OUT
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import patrol_amd as pa  # noqa: E402
from tests import _gen  # noqa: E402
from tests.test_receive_batches import wire  # noqa: E402
from tests.test_receive_optimistic import K, N, SEC, Batch, raising_states  # noqa: E402


def handle(rng, **kw):
    g = pa.GPURepo(log2_slots=17, isolate=kw.pop("isolate", False), **kw)
    a, t, e = _gen.clean_states(rng, K)
    g.seed(_gen.key_names(np.arange(K)), a, t, e, _gen.T0 - rng.integers(0, SEC, K))
    g.set_timing(True, accumulate=True)
    return g


def clean(rng, step, k=K):
    return Batch(_gen.zipf_ids(rng, N, k), *raising_states(rng, N, step), _gen.T0 + step * SEC)


def incast_cold(rng, step):
    """A clean batch with one incast, on a bucket the batch names once more."""
    b_ids = _gen.zipf_ids(rng, N, K)
    a, t, e = raising_states(rng, N, step)
    at = N // 3
    b_ids[at] = int(np.nonzero(np.bincount(b_ids, minlength=K) == 1)[0][0])
    a[at], t[at], e[at] = 0, 0, 0
    return Batch(b_ids, a, t, e, _gen.T0 + step * SEC)


def new_names(rng, step, count):
    """A clean batch `count` of whose messages name distinct new buckets."""
    ids = _gen.zipf_ids(rng, N, K)
    ids[rng.choice(N, count, replace=False)] = K + np.arange(count)
    return Batch(ids, *raising_states(rng, N, step), _gen.T0 + step * SEC)


def three_dirty(rng, step):
    ids = _gen.zipf_ids(rng, N, K)
    a, t, e = raising_states(rng, N, step)
    pos = rng.choice(N, 3, replace=False)
    a[pos], t[pos], e[pos] = 0, 0, 0
    return Batch(ids, a, t, e, _gen.T0 + step * SEC)


def uniform_raising(rng):
    """Uniform ids, every message above whatever its bucket held: the
    optimistic pass's log overflows (test_log_overflow)."""
    up = np.arange(N, dtype=np.float64)
    return Batch(rng.integers(0, K, N), (2e6 + up + 0.5).view(np.uint64).copy(),
                 (2e6 + up).view(np.uint64).copy(), (1 << 40) + np.arange(N, dtype=np.int64),
                 _gen.T0 + SEC)


def soa(g, batches, queue=False):
    keep = [b.run(g, queue) for b in batches]   # (a queued batch's tensors stay alive)
    g.flush()
    return keep


def datagrams(g, b, short_at=None):
    dgs = wire(b.names, b.a, b.t, b.e)
    if short_at is not None:
        dgs[short_at] = dgs[short_at][:20]
    g.receive_datagrams(dgs, b.now)


def bad_offsets_queued(g, rng):
    """Checked names with a non-monotone entry in the second of three queued
    batches (test_checked_names_non_monotone_entry)."""
    bs = [clean(rng, 1), clean(rng, 2, K + 100), clean(rng, 3)]
    bs[1].offs[70001] = bs[1].offs[70000] - 1
    try:
        soa(g, bs, queue=True)
    except pa.PatrolHipError as err:
        assert err.code == -1, err
    g.flush()


SCENARIOS = [
    ("clean_sync", {}, lambda g, r: soa(g, [clean(r, 1)])),
    ("clean_queued_x3", {}, lambda g, r: soa(g, [clean(r, s) for s in (1, 2, 3)], True)),
    ("incast_cold_sync", {}, lambda g, r: soa(g, [incast_cold(r, 1)])),
    ("incast_cold_queued_between_clean", {},
     lambda g, r: soa(g, [clean(r, 1), incast_cold(r, 2), clean(r, 3)], True)),
    ("new_names_1000", {}, lambda g, r: soa(g, [new_names(r, 1, 1000)])),
    ("new_names_65536", {}, lambda g, r: soa(g, [new_names(r, 1, 1 << 16)])),
    ("isolate_3_dirty", dict(isolate=True), lambda g, r: soa(g, [three_dirty(r, 1)])),
    ("classify_first", dict(classify_first=True), lambda g, r: soa(g, [clean(r, 1)])),
    ("log_overflow_then_backoff", {}, lambda g, r: soa(g, [uniform_raising(r), clean(r, 2)])),
    ("wire_clean", {}, lambda g, r: datagrams(g, clean(r, 1))),
    ("wire_short_in_middle", {}, lambda g, r: datagrams(g, clean(r, 1), N // 2)),
    ("checked_names_bad_entry_queued", {}, bad_offsets_queued),
]


def main():
    for k, (name, cfg, run) in enumerate(SCENARIOS):
        rng = np.random.default_rng(900 + k)
        g = handle(rng, **cfg)
        run(g, rng)
        print(json.dumps({"scenario": name, "kernels": [nm for nm, _ in g.timings()]}), flush=True)
        g.close()


if __name__ == "__main__":
    main()
