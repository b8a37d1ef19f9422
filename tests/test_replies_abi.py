"""Incast reply egress without a GPU: the C ABI as declared, exported and
bound (include/patrolhip.h "Incast reply egress"), phip_reply_peers, and the
model of tests/_replies_cases.py pinned against the host phip_incast_replies
on the oracle's columns."""
import ctypes as C
import os
import re

import numpy as np

import patrol_amd as pa
from oracle import oracle as O
from patrol_amd import _lib
from tests import _replies_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["phip_receive_soa_replies", "phip_receive_datagrams_replies",
         "phip_ring_receive_replies", "phip_reply_peers"]


def header():
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_reply_abi():
    src = header()
    for f in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, src), f
    assert re.search(r"typedef struct phip_reply_egress \{[^}]*\} phip_reply_egress;", src)
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", src)
    assert re.search(r"\bint\s+phip_incast_replies\s*\(", src)   # stays


def test_exported_and_bound():
    L = _lib.load()
    for f in FUNCS:
        assert f in _lib.EXPORTS and hasattr(L, f), f
    assert L.phip_abi_version() == 3
    for f in ("receive_soa_replies", "receive_soa_replies_device", "receive_datagrams_replies",
              "receive_datagrams_replies_device"):
        assert callable(getattr(pa.GPURepo, f))
    assert callable(pa.Ring.receive_replies) and callable(pa.reply_peers)


def test_struct_layout():
    e = _lib.phip_reply_egress
    fields = ("out", "out_cap", "offs", "src", "max_msgs", "n", "replies", "skipped", "bytes")
    assert [getattr(e, f).offset for f in fields] == [0, 8, 16, 24, 32, 36, 40, 44, 48]
    assert C.sizeof(e) == 56


def test_reply_peers_is_a_gather():
    rng = np.random.default_rng(5)
    peers = rng.integers(0, 256, (300, _lib.PEER_BYTES), dtype=np.uint8)
    src = np.sort(rng.choice(300, 70, replace=False)).astype(np.uint32)
    assert np.array_equal(pa.reply_peers(peers, src), peers[src])
    assert pa.reply_peers(peers, src[:0]).shape == (0, _lib.PEER_BYTES)
    L = _lib.load()
    out = np.zeros((70, _lib.PEER_BYTES), np.uint8)
    assert L.phip_reply_peers(None, None, 0, None) == 0
    assert L.phip_reply_peers(None, src.ctypes.data, 70, out.ctypes.data) == -1
    assert L.phip_reply_peers(peers.ctypes.data, None, 70, out.ctypes.data) == -1
    assert L.phip_reply_peers(peers.ctypes.data, src.ctypes.data, 70, None) == -1


def oracle_case(c, as_wire):
    o = O.Repo()
    o.seed(*c["seed"])
    if as_wire:
        st, ra, rt, re, stop = o.receive(RC.wire(c["names"], c["a"], c["t"], c["e"]), RC.NOW)
        assert stop == len(c["names"])
    else:
        st, ra, rt, re = o.receive_soa(c["names"], c["a"], c["t"], c["e"], RC.NOW)
    return st, ra, rt, re


def test_model_equals_the_host_incast_replies():
    """The model's datagrams are, byte for byte, what phip_incast_replies
    makes of the oracle's full status and reply columns; the case holds every
    kind of request the GPU tests rely on."""
    c = RC.make_case(7, 4000, K=500, long=6)
    st, ra, rt, re = oracle_case(c, True)
    RC.check_case(c, st, ra, rt, re, replies=50, absent=5, zero=5, negzero=3, twice=5, long=5)
    assert np.array_equal(st, oracle_case(c, False)[0])
    e = RC.expected(c["names"], st, ra, rt, re)
    assert e["n"] == e["replies"] >= 50 and e["skipped"] == 0
    dgs = RC.wire(c["names"], c["a"], c["t"], c["e"])
    offs = np.zeros(len(dgs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in dgs])
    blob = np.frombuffer(b"".join(dgs), np.uint8).copy()
    reply = np.zeros(len(dgs), dtype=[("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
    reply["a"], reply["t"], reply["e"] = ra, rt, re
    peers = np.random.default_rng(1).integers(0, 256, (len(dgs), _lib.PEER_BYTES), dtype=np.uint8)
    data, oo, op = pa.incast_replies(blob, offs, st, reply, peers)
    assert bytes(data) == e["data"] and np.array_equal(oo, e["offs"])
    assert np.array_equal(op, pa.reply_peers(peers, e["src"]))
    # each datagram decodes to the reply state under the request's name
    for k, d in enumerate(RC.datagrams_of(e)):
        i = int(e["src"][k])
        assert d[25:] == c["names"][i] and d[24] == len(c["names"][i])
        assert int.from_bytes(d[:8], "big") == int(ra[i])


def test_model_cuts_at_a_record():
    c = RC.make_case(8, 3000, K=300)
    st, ra, rt, re = oracle_case(c, False)
    full = RC.expected(c["names"], st, ra, rt, re)
    m = RC.expected(c["names"], st, ra, rt, re, max_msgs=10)
    assert m["n"] == 10 and m["replies"] == full["replies"]
    assert m["data"] == full["data"][:int(full["offs"][10])]
    budget = int(full["offs"][20]) + 3
    b = RC.expected(c["names"], st, ra, rt, re, budget=budget)
    assert b["n"] == 20 and b["bytes"] == int(full["offs"][20]) and b["replies"] == full["replies"]
    assert np.array_equal(b["src"], full["src"][:20])
