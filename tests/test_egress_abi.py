"""Coalesced egress without a GPU: the C ABI as declared, exported and bound
(include/patrolhip.h "Coalesced egress"), phip_egress_caps' arithmetic, and
the model of tests/_egress_cases.py checked on oracle repos alone: what a
batch's egress must contain, and when a peer that merges it ends where the
reference's per-op broadcasts would leave it."""
import ctypes as C
import os
import re

import numpy as np

from oracle import oracle as O
from patrol_amd import _lib
from tests import _egress_cases as EC
from tests import _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["phip_egress_caps", "phip_apply_mixed_egress", "phip_batcher_open_egress",
         "phip_batcher_egress_next", "phip_batcher_egress_done"]


def header():
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_egress_abi():
    src = header()
    for f in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, src), f
    for s in ("phip_egress", "phip_egress_batch"):
        assert re.search(r"typedef struct %s \{[^}]*\} %s;" % (s, s), src), s
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", src)


def test_exported_and_bound():
    L = _lib.load()
    for f in FUNCS:
        assert f in _lib.EXPORTS and hasattr(L, f), f
    assert L.phip_abi_version() == 3


def test_struct_layouts():
    e = _lib.phip_egress
    assert [getattr(e, f).offset for f in ("out", "out_cap", "offs", "max_msgs", "n_incast", "n",
                                           "reserved", "bytes")] == [0, 8, 16, 24, 28, 32, 36, 40]
    assert C.sizeof(e) == 48
    b = _lib.phip_egress_batch
    assert [getattr(b, f).offset for f in ("bytes", "offs", "n", "n_incast", "batch", "first_seq",
                                           "requests", "reserved")] == [0, 8, 16, 20, 24, 32, 40, 44]
    assert C.sizeof(b) == 48


def test_caps_formula():
    L = _lib.load()
    for n in (0, 1, 1024, 1 << 30):
        for nb in (0, 7 * n, 231 * n):
            for dev in (False, True):
                m, c = C.c_uint32(), C.c_uint64()
                assert L.phip_egress_caps(n, nb, _lib.DEVICE_PTRS if dev else 0, C.byref(m),
                                          C.byref(c)) == 0
                want = 2 * (25 * n + nb)
                if dev:
                    want = (want + 7) // 8 * 8 + 8
                    assert c.value % 8 == 0
                assert (m.value, c.value) == (2 * n, want), (n, nb, dev)
    m, c = C.c_uint32(), C.c_uint64()
    assert L.phip_egress_caps((1 << 30) + 1, 0, 0, C.byref(m), C.byref(c)) == -1
    assert L.phip_egress_caps(1, 1, 0x20, C.byref(m), C.byref(c)) == -1   # unknown flag


def peer_after(datagrams, now):
    p = O.Repo()
    if datagrams:
        st, _, _, _, stop = p.receive(datagrams, now)
        assert stop == len(datagrams)
    return p.dump()


def test_monotone_takes_coalesce_exactly():
    """TAKE-only, one rate per bucket, a non-decreasing clock: first the
    premise, from the oracle's replies alone (each bucket's post-op states
    never decrease in any field; if the reference did not satisfy it this
    fails here, by name), then the claim: a peer that receives the model's
    coalesced datagrams equals one that received every per-op broadcast."""
    rng = np.random.default_rng(11)
    ops = EC.monotone_takes(rng, 20000, 2000)
    o = O.Repo()
    ref = EC.call(o, ops)
    EC.assert_monotone(ops, ref)
    dump = o.dump()
    req, st = EC.expected_datagrams(ops, ref, dump)
    per_op = EC.per_op_broadcasts(ops, ref)
    now = int(ops["now"][-1]) + 1
    assert peer_after(list(req.values()) + list(st.values()), now) == peer_after(per_op, now)
    distinct = len(set(ops["names"]))
    created = sum(1 for s in ref["status"] if s & EC.CREATED)
    assert created == distinct == len(req)        # a fresh repo: every bucket's first take
    assert len(req) + len(st) <= distinct + created
    assert len(per_op) == 20000 + created


def test_second_batch_on_existing_buckets():
    """A later batch creates only the buckets the first did not name."""
    rng = np.random.default_rng(12)
    o = O.Repo()
    first = EC.monotone_takes(rng, 3000, 300)
    EC.call(o, first)
    ops = EC.monotone_takes(rng, 3000, 600, t0=int(first["now"][-1]))
    ref = EC.call(o, ops)
    incast, states = EC.expected(ops, ref, o.dump())
    assert set(incast) == set(ops["names"]) - set(first["names"])
    assert set(states) <= set(ops["names"])


def test_mixed_batch_model_against_the_dump():
    """gen_ops' mix (TAKE at two rates per bucket, RECEIVE, incasts, UPSERT):
    the model's states are the dump's final states of exactly the buckets a
    TAKE or UPSERT named.  Peer equivalence with the per-op broadcasts is not
    asserted here: with two rates on a bucket a take at the smaller capacity
    lowers `added` (bucket.go:210-213), and an UPSERT stores any state, so a
    peer that saw an intermediate state keeps a higher field than the final
    one -- the limit patrolhip.h states."""
    rng = np.random.default_rng(13)
    pool = EC.name_pool(40)
    ops = EC.gen_ops(rng, 3000, pool)
    o = O.Repo()
    ref = EC.call(o, ops)
    dump = o.dump()
    incast, states = EC.expected(ops, ref, dump)
    named = {nm for nm, k in zip(ops["names"], ops["kind"]) if k in (EC.TAKE, EC.UPSERT)}
    assert set(states) <= named
    for nm in named:
        if nm in states:
            assert states[nm] == dump[nm][:3]
        else:
            assert EC.is_zero(*dump[nm][:3])
    firsts = {}
    for i, nm in enumerate(ops["names"]):
        firsts.setdefault(nm, i)
    for nm in incast:
        assert ops["kind"][firsts[nm]] == EC.TAKE and dump[nm][3] == ops["now"][firsts[nm]]
    # buckets a RECEIVE or UPSERT created send no request
    assert any(ops["kind"][i] != EC.TAKE for i in firsts.values())
    assert all(ops["kind"][firsts[nm]] == EC.TAKE for nm in incast)
    assert len(set(incast)) == len(incast)
    # where a bucket's last op is a TAKE or UPSERT, the reference's last
    # broadcast of it carries the state the model sends (a later RECEIVE
    # changes the state and broadcasts nothing)
    last, last_kind = {}, {}
    for i, nm in enumerate(ops["names"]):
        last_kind[nm] = ops["kind"][i]
        if ops["kind"][i] in (EC.TAKE, EC.UPSERT):
            last[nm] = EC.marshal(nm, ref["reply_added"][i], ref["reply_taken"][i],
                                  ref["reply_elapsed"][i])
    checked = 0
    for nm, s in states.items():
        if last_kind[nm] != EC.RECEIVE:
            assert last[nm] == EC.marshal(nm, *s)
            checked += 1
    assert checked
    assert _gen.T0 <= int(ops["now"][0])
