"""The change set without a GPU: the C ABI as declared, exported and bound
(include/patrolhip.h "Change set"), and the model of tests/_changes_cases.py
checked on oracle repos alone: what drains at arbitrary batch boundaries must
contain, and that a peer which merges them in order ends where the
reference's per-op broadcasts would leave it."""
import ctypes as C
import os
import re

import numpy as np

from oracle import oracle as O
from patrol_amd import _lib
from tests import _changes_cases as CC
from tests import _egress_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_change_set_abi():
    src = header()
    assert re.search(r"#define PHIP_CFG_TRACK_CHANGES 0x20u\b", src)
    assert re.search(r"typedef struct phip_changes_stats \{[^}]*\} phip_changes_stats;", src)
    assert re.search(r"\bint\s+phip_export_changed\s*\(", src)
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", src)


def test_exported_and_bound():
    L = _lib.load()
    assert "phip_export_changed" in _lib.EXPORTS and hasattr(L, "phip_export_changed")
    assert _lib.CFG_TRACK_CHANGES == 0x20
    assert L.phip_abi_version() == 3
    # no handle, no stats: refused before anything is touched
    assert L.phip_export_changed(None, None, 0, None, 0, None, 0) == -1


def test_struct_layout():
    s = _lib.phip_changes_stats
    assert [getattr(s, f).offset for f in ("n", "bytes", "n_incast", "done", "pending")] == \
        [0, 8, 16, 20, 24]
    assert C.sizeof(s) == 32


def peer_after(datagrams, now, peer=None):
    p = O.Repo() if peer is None else peer   # (an empty Repo is falsy: it has a length)
    if datagrams:
        assert p.receive(datagrams, now)[4] == len(datagrams)
    return p


def test_drains_at_batch_boundaries_equal_per_op_broadcasts():
    """monotone_takes in several batches, a drain after some of them: first the
    premise (each bucket's post-op states never decrease, from the oracle's
    replies alone), then the claim: a peer that merges every drain's model
    datagrams in order equals one that received every per-op broadcast."""
    rng = np.random.default_rng(111)
    ops = EC.monotone_takes(rng, 20000, 2000)
    whole = EC.call(O.Repo(), ops)
    EC.assert_monotone(ops, whole)
    now = int(ops["now"][-1]) + 1
    want = peer_after(EC.per_op_broadcasts(ops, whole), now).dump()
    for cuts, drain_after in (([5000, 5001, 9000, 16000], {0, 2, 3, 4}),
                              ([1, 19999], {0, 1, 2}),
                              ([7000, 14000], {2})):
        m = CC.Model(O.Repo())
        peer = O.Repo()
        sent = requests = 0
        for k, b in enumerate(CC.split(ops, cuts)):
            m.batch(b)
            if k in drain_after:
                req, st = m.expected()
                assert m.pending() == len(m.req) + len(m.touched)
                dgs = m.datagrams()
                peer_after(dgs, now, peer)
                sent += len(dgs)
                requests += len(req)
                m.drained()
        assert m.pending() == 0
        assert peer.dump() == want, cuts
        distinct = len(set(ops["names"]))
        assert requests == distinct                 # every bucket is created once, by a take
        assert sent <= 20000 + distinct             # never more than one datagram per take
    # one drain at the end is the egress of the whole stream as one batch
    m = CC.Model(O.Repo())
    for b in CC.split(ops, [3000, 11000]):
        m.batch(b)
    o = O.Repo()
    ref = EC.call(o, ops)
    assert m.expected() == EC.expected_datagrams(ops, ref, o.dump())


def test_mixed_model_against_the_dump():
    """gen_ops' mix in three batches with a RECEIVE-only batch between them:
    the model's states are the dump's final states of exactly the buckets a
    TAKE or UPSERT named since the drain, and its requests the buckets a TAKE
    created; a bucket named only by RECEIVE ops appears in neither."""
    rng = np.random.default_rng(113)
    pool = EC.name_pool(60)
    o = O.Repo()
    m = CC.Model(o)
    named, first_kind = set(), {}
    t0 = None
    for k in range(3):
        ops = EC.gen_ops(rng, 1500, pool) if t0 is None else EC.gen_ops(rng, 1500, pool, t0=t0)
        t0 = int(ops["now"][-1])
        for nm, kd in zip(ops["names"], ops["kind"]):
            first_kind.setdefault(nm, int(kd))
            if kd in (CC.TAKE, CC.UPSERT):
                named.add(nm)
        m.batch(ops)
        extra = [b"only-received-%d" % i for i in range(5)]
        a = np.full(5, np.float64(3.0 + k).view(np.uint64), np.uint64)
        m.receive_soa(extra, a, a.copy(), np.full(5, 7 + k, np.int64), t0)
        for nm in extra:
            first_kind.setdefault(nm, CC.RECEIVE)
    dump = o.dump()
    req, st = m.expected()
    assert set(st) <= named and not any(nm.startswith(b"only-received") for nm in set(st) | set(req))
    for nm in named:
        if nm in st:
            assert st[nm] == EC.marshal(nm, *dump[nm][:3])
        else:
            assert EC.is_zero(*dump[nm][:3]) or len(nm) > CC.MAX_NAME
    assert set(req) == {nm for nm, kd in first_kind.items() if kd == CC.TAKE}
    assert any(kd != CC.TAKE for kd in first_kind.values())
    assert m.pending() == len(named) + len(req)
    m.evict(list(named)[:10])
    req2, st2 = m.expected()
    assert not (set(list(named)[:10]) & (set(req2) | set(st2)))
    m.drained()
    assert m.expected() == ({}, {}) and m.pending() == 0
