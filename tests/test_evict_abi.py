"""phip_evict_idle without a GPU: the binding's constants and struct match
include/patrolhip.h, and the local property the sweep's safety rests on
(idle_ns >= per: the first Take on a recreated bucket answers as the evicted
one would have) holds for the inputs tests/test_evict.py reuses on the GPU,
checked with the oracle alone."""
import ctypes as C
import os
import re

import pytest

from patrol_amd import _lib
from oracle import oracle as O
from tests import _evict_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evict_flag_constants_match_header():
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    defs = {m.group(1): int(m.group(2), 16)
            for m in re.finditer(r"#define PHIP_([A-Z_0-9]+)\s+(0x[0-9a-fA-F]+)u", src)}
    assert defs["EVICT_SHRINK"] == 0x40 and defs["EVICT_DRY_RUN"] == 0x80
    for name in ("EVICT_SHRINK", "EVICT_DRY_RUN"):
        assert getattr(_lib, name) == defs[name], name
    # no call flag shares a bit with them
    others = [v for k, v in defs.items() if not k.startswith(("CFG_", "EVICT_"))]
    assert all(v & 0xC0 == 0 for v in others), defs


def test_evict_stats_struct_layout():
    assert C.sizeof(_lib.phip_evict_stats) == 48
    assert [f for f, _ in _lib.phip_evict_stats._fields_] == \
        ["idle", "evicted", "buckets", "slots", "arena_used", "arena_freed"]
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    body = re.search(r"typedef struct phip_evict_stats \{(.*?)\} phip_evict_stats;", src, re.S)
    fields = re.findall(r"uint64_t (\w+);", body.group(1))
    assert fields == [f for f, _ in _lib.phip_evict_stats._fields_]
    assert "phip_evict_idle" in _lib.EXPORTS and "phip_group_evict_idle" in _lib.EXPORTS


@pytest.mark.parametrize("rate", EC.RATES)
def test_take_on_recreated_bucket_equals_take_on_idle_bucket(rate):
    """dt >= per: Tokens(dt) >= Freq, the refill clamps to capacity - tokens
    (bucket.go:210-213), have == capacity either way."""
    freq, per, count = rate
    assert per >= freq > 0
    bs = EC.buckets(rate)
    assert len(bs) == len(EC.STATES) * 3
    for name, a, t, e, created in bs:
        assert a == int(a) and t == int(t) and 0 <= t <= a < 2**53
        assert EC.NOW - (created + e) in EC.dts(per)
        old = O.take_fields([a, t, e], created, EC.NOW, freq, per, count)
        new = O.take_fields([0.0, 0.0, 0], EC.NOW, EC.NOW, freq, per, count)
        assert old[:2] == new[:2], (name, rate, old, new)
        assert new[:2] == ((freq - count, True) if count <= freq else (freq, False))
