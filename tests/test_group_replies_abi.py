"""Group reply egress without a GPU: the four symbols are exported with the
header's signatures and bound, refused arguments (NULL group, NULL batches,
NULL rq, flags without PHIP_DEVICE_PTRS, unknown flag bits) return
PHIP_ERR_INVALID before any device call -- the group pointer below is a dummy
that the library must not follow -- and the cases of tests/test_group_replies.py
hold what they are for, from the oracle's columns alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from patrol_amd import _lib
from tests import _group_replies_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECEIVE = ("phip_group_receive_datagrams_replies", "phip_group_receive_replies",
           "phip_group_ring_receive_replies")
NAMES = RECEIVE + ("phip_group_reply_stats",)
ALLOWED = _lib.DEVICE_PTRS | _lib.ROUTE_COMBINE | _lib.GROUP_RCCL_SELF | _lib.GROUP_SMALL_CHUNKS


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return "ptr"
    return {"uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "int": C.c_int}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported_with_the_headers_signature(name):
    L = _lib.load()
    assert name in _lib.EXPORTS and hasattr(L, name)
    params = _prototype(name)
    argtypes = getattr(L, name).argtypes
    assert len(argtypes) == len(params)
    for p, a in zip(params, argtypes):
        want = _ctype_of(p)
        if want == "ptr":
            assert a is C.c_void_p or issubclass(a, C._Pointer), (p, a)
        else:
            assert a is want, (p, a)
    if name in RECEIVE:
        assert params[-1] == "uint32_t flags" and params[-2] == "phip_reply_egress* rq"


def test_abi_version_unchanged():
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    assert re.search(r"#define\s+PHIP_ABI_VERSION\s+3\b", src)


def _dummy():
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


def _calls():
    """name -> call(g, batches, rq, flags) over dummy pointers."""
    L = _lib.load()
    rings = (C.c_void_p * 1)()
    slots = (C.c_uint32 * 1)()
    return {
        "wire": (lambda g, b, rq, f: L.phip_group_receive_datagrams_replies(g, b, 0, None, None, None, rq, f),
                 (_lib.phip_wire * 1)()),
        "msgs": (lambda g, b, rq, f: L.phip_group_receive_replies(g, b, 0, None, None, rq, f),
                 (_lib.phip_msgs * 1)()),
        "ring": (lambda g, b, rq, f: L.phip_group_ring_receive_replies(g, b, slots, 0, None, None, None, rq, f),
                 rings),
    }


@pytest.mark.parametrize("form", ["wire", "msgs", "ring"])
def test_receive_forms_refuse_before_any_device_call(form):
    call, batches = _calls()[form]
    keep, g = _dummy()
    rq = (_lib.phip_reply_egress * 1)()
    D = _lib.DEVICE_PTRS
    assert call(None, batches, rq, D) == -1
    assert call(g, None, rq, D) == -1
    assert call(g, batches, None, D) == -1
    assert call(g, batches, rq, 0) == -1
    assert call(g, batches, rq, _lib.ROUTE_COMBINE) == -1
    for bit in (0x10, 0x20, 0x100, 0x8000_0000):
        assert not bit & ALLOWED
        assert call(g, batches, rq, D | bit) == -1


def test_ring_form_refuses_null_slots():
    L = _lib.load()
    keep, g = _dummy()
    rings = (C.c_void_p * 1)()
    rq = (_lib.phip_reply_egress * 1)()
    assert L.phip_group_ring_receive_replies(g, rings, None, 0, None, None, None, rq,
                                             _lib.DEVICE_PTRS) == -1


def test_reply_stats_refuses_null():
    L = _lib.load()
    out = (C.c_uint64 * 4)()
    assert L.phip_group_reply_stats(None, 0, out, 4) == 0


# ------------------------------------------------------------ the model --
@pytest.mark.parametrize("world,sizes", [(2, (9000, 4097)), (3, (9000, 4097, 1)), (3, (9000, 0, 4097)),
                                         (1, (9000,))])
def test_pipelined_cases_hold_what_they_are_for(world, sizes):
    b = GC.build(world, sizes, 9100 + world)
    GC.check_group_case(b["case"], b["cols"], edge_own=2, edge_other=2 if world > 1 else 0,
                        shared=world > 1 and sizes[1] >= 3, again=True)
    ex = GC.expected(b["case"]["names"], b["cols"], world)
    # (every large member plants 40 requests to warm buckets beside the tagged ones)
    assert sum(e["n"] for e in ex) >= 40 * sum(n >= 1000 for n in sizes)
    assert all(e["n"] == e["replies"] for e in ex)
    for e, n in zip(ex, sizes):
        assert np.all(np.diff(e["src"].astype(np.int64)) > 0) and (n or e["n"] == 0)
    # answers in both rounds of the first member, on both sides of the boundary
    assert (ex[0]["src"] < GC.CHUNK).any() and (ex[0]["src"] >= GC.CHUNK).any()


def test_model_order_is_round_then_rank():
    """Member 1's request in round 0 sees what member 0 merged in round 0, not
    what it merges in round 1."""
    from oracle import oracle as O
    from tests import _replies_cases as RC
    up = lambda v: np.float64(v).view(np.uint64)   # noqa: E731
    n0 = [b"x"] * (GC.CHUNK + 1)
    a0 = np.full(GC.CHUNK + 1, up(5.0), np.uint64)
    a0[-1] = up(9.0)
    per = [RC.wire(n0, a0, a0, np.ones(GC.CHUNK + 1, np.int64)),
           RC.wire([b"x"], np.zeros(1, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.int64))]
    cols = GC.model(O.Repo(), per, GC.NOW, GC.CHUNK)
    assert cols[1][0][0] & 0x7F == GC.REPLY and cols[1][1][0] == up(5.0)


def test_long_names_count_at_their_owner():
    b = GC.build(2, (3000, 3000), 9200, long_names=6)
    GC.check_group_case(b["case"], b["cols"], long=12)
    ex = GC.expected(b["case"]["names"], b["cols"], 2)
    assert sum(e["skipped"] for e in ex) >= 12
    for e, names in zip(ex, b["case"]["names"]):
        assert all(len(names[int(i)]) <= 231 for i in e["src"]) and e["n"] == e["replies"]
