"""The owner-routed peek without a GPU: phip_group_peek is exported and bound,
its flag has the header's value, a NULL group is refused before any HIP call,
and the inputs of the GPU tests (tests/test_group_peek.py) meet their
conditions, computed from the reference alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from patrol_amd import _lib
from tests import _group_ops as GO
from tests import _group_peek as GP
from tests import _peek_cases as PC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "patrolhip.h")


def test_symbol_exported_and_bound():
    L = _lib.load()
    assert "phip_group_peek" in _lib.EXPORTS
    assert hasattr(L, "phip_group_peek")
    assert len(L.phip_group_peek.argtypes) == 6
    assert L.phip_abi_version() == 3


def test_peek_state_flag_is_the_headers():
    text = open(HEADER).read()
    m = re.search(r"#define\s+PHIP_GROUP_PEEK_STATE\s+0x([0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == _lib.GROUP_PEEK_STATE
    # a bit of its own among the call flags
    others = (_lib.DEVICE_PTRS, _lib.ROUTE_COMBINE, _lib.GROUP_RCCL_SELF, _lib.GROUP_SMALL_CHUNKS,
              _lib.RECV_ASYNC, _lib.RECV_CLASSIFY, _lib.EVICT_SHRINK, _lib.EVICT_DRY_RUN,
              _lib.SWEEP_COUNT)
    assert bin(_lib.GROUP_PEEK_STATE).count("1") == 1 and _lib.GROUP_PEEK_STATE not in others


def test_null_group_is_invalid():
    L = _lib.load()
    ops = _lib.phip_ops()
    res = _lib.phip_peek_results()
    for flags in (_lib.DEVICE_PTRS, _lib.DEVICE_PTRS | _lib.GROUP_PEEK_STATE):
        assert L.phip_group_peek(None, C.byref(ops), C.byref(res), None, None, flags) == -1


@pytest.fixture(scope="module")
def tab():
    return GP.table()


@pytest.mark.parametrize("world,sizes", GP.SHARED_CASES + [GP.ROUNDS_CASE])
def test_gpu_inputs_meet_their_conditions(tab, world, sizes):
    """Every member's batch holds the case mix (PC.check_mix: >= 20% granted,
    >= 20% denied-finite, >= 10% never, >= 10% absent) and every (source,
    owner) pair at least MIN_PAIR queries, so that every segment of the
    exchange is exercised and a misrouted query cannot hide."""
    o = GP.seeded_oracle(tab)
    for i, queries in enumerate(GP.member_queries(tab, world, sizes)):
        assert len(queries) == sizes[i]
        if not queries:
            continue
        k, absent = PC.check_mix(GP.references(o.get, queries))
        own = np.bincount(GO.owners([q[0] for q in queries], world), minlength=world)
        assert own.min() >= GP.MIN_PAIR, (i, own)
        print("world %d member %d: %s, %d absent, owners %s" % (world, i, k, absent, own.tolist()))


def test_table_is_spread_over_the_owners(tab):
    """Buckets per owner: no shard of the seeded table is empty or near it."""
    for world in (2, 3):
        per = np.bincount(GO.owners(tab["names"], world), minlength=world)
        assert per.sum() == GP.TABLE_BUCKETS and per.min() >= GP.TABLE_BUCKETS // (2 * world), per
