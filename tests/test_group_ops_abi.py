"""The owner-routed op path without a GPU: the two entry points are exported
and bound, reject a NULL handle / group before touching HIP, and the order
rule the GPU tests compare against (tests/_group_ops.py) is pinned on a
hand-written example."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from patrol_amd import _lib
from tests import _gen
from tests import _group_ops as GO


def test_symbols_exported_and_bound():
    L = _lib.load()
    for name in ("phip_route_pack_ops", "phip_group_apply_mixed"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert len(L.phip_route_pack_ops.argtypes) == 14
    assert len(L.phip_group_apply_mixed.argtypes) == 6
    assert L.phip_abi_version() == 3


def test_null_handle_and_group_are_invalid():
    L = _lib.load()
    ops = _lib.phip_ops()
    res = _lib.phip_results()
    assert L.phip_route_pack_ops(None, C.byref(ops), 2, None, None, None, None, None, None, None,
                                 None, None, None, _lib.DEVICE_PTRS) == -1
    assert L.phip_group_apply_mixed(None, C.byref(ops), C.byref(res), None, None,
                                    _lib.DEVICE_PTRS) == -1


def test_order_rule_on_a_hand_written_example():
    """Two members, three ops each, chunk 2: two rounds.  Round 0 holds ops 0-1
    of member 0 then of member 1, round 1 op 2 of member 0 then of member 1.
    All six are Takes of 1 on one bucket at 3:1h with equal `now` (no refill):
    the first three in order are granted, so WHICH three says which order ran."""
    order = GO.apply_order([3, 3], chunk=2)
    assert order == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (1, 2)]
    assert GO.apply_order([3, 3], chunk=4) == GO.rank_order([3, 3])
    assert GO.apply_order([1, 0, 5], chunk=2) == [(0, 0), (2, 0), (2, 1), (2, 2), (2, 3), (2, 4)]

    def batch():
        n = 3
        return dict(names=[b"hot"] * n, kind=np.zeros(n, np.uint8), now=np.full(n, _gen.T0, np.int64),
                    freq=np.full(n, 3, np.int64), per=np.full(n, 3600 * _gen.SEC, np.int64),
                    count=np.ones(n, np.uint64), added=np.zeros(n, np.uint64),
                    taken=np.zeros(n, np.uint64), elapsed=np.zeros(n, np.int64))
    bs = [batch(), batch()]
    OK, DENIED, CREATED = _lib.ST_TAKE_OK, _lib.ST_TAKE_DENIED, _lib.ST_CREATED
    got = GO.oracle_results(O.Repo(), bs, order)
    assert got[0]["status"].tolist() == [OK | CREATED, OK, DENIED]
    assert got[1]["status"].tolist() == [OK, DENIED, DENIED]
    assert got[0]["remaining"].tolist() == [2, 1, 0]
    assert got[1]["remaining"].tolist() == [0, 0, 0]
    # every Take has a reply state, created at the first op's `now`
    assert all(int(r[3]) == _gen.T0 for g in got for r in g["reply"])
    # the order without rounds grants member 0's three instead
    other = GO.oracle_results(O.Repo(), bs, GO.rank_order([3, 3]))
    assert other[0]["status"].tolist() == [OK | CREATED, OK, OK]
    assert other[1]["status"].tolist() == [DENIED] * 3
