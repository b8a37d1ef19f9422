"""The group's wire path without a GPU: phip_route_pack_datagrams,
phip_group_receive_datagrams and phip_group_ring_receive are exported with the
header's signatures and bound, phip_wire is laid out as the header says, and
refused arguments (NULL group, NULL batches, flags without PHIP_DEVICE_PTRS,
unknown flag bits) return PHIP_ERR_INVALID before any device call: the group
and handle pointers below are dummies that the library must not follow."""
import ctypes as C
import os
import re

import pytest

from patrol_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phip_route_pack_datagrams", "phip_group_receive_datagrams", "phip_group_ring_receive")
ALLOWED = _lib.DEVICE_PTRS | _lib.ROUTE_COMBINE | _lib.GROUP_RCCL_SELF | _lib.GROUP_SMALL_CHUNKS


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    """The ctypes kind a header parameter binds to: pointers, and the scalars by width."""
    if "*" in param:
        return "ptr"
    return {"uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}[param.split()[0]]


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
    assert params[-1] == "uint32_t flags"


def test_phip_wire_layout():
    """n, reserved, bytes, offs, bytes_len: 32 bytes, as the header's struct."""
    assert C.sizeof(_lib.phip_wire) == 32
    assert [f[0] for f in _lib.phip_wire._fields_] == ["n", "reserved", "bytes", "offs", "bytes_len"]
    assert _lib.phip_wire.n.offset == 0 and _lib.phip_wire.reserved.offset == 4
    assert _lib.phip_wire.bytes.offset == 8 and _lib.phip_wire.offs.offset == 16
    assert _lib.phip_wire.bytes_len.offset == 24
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    body = re.search(r"typedef struct phip_wire \{(.*?)\} phip_wire;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(x.split()) for x in body.split(";") if x.strip()]
    assert fields == ["uint32_t n", "uint32_t reserved", "const uint8_t* bytes",
                      "const uint64_t* offs", "uint64_t bytes_len"]


def _dummy():
    """A non-NULL pointer to zeroed host bytes: a group / handle / ring that
    must be refused before it is looked at."""
    buf = C.create_string_buffer(4096)
    return buf, C.cast(buf, C.c_void_p)


def test_group_receive_datagrams_refuses_before_any_device_call():
    L = _lib.load()
    keep, g = _dummy()
    w = (_lib.phip_wire * 1)()
    D = _lib.DEVICE_PTRS
    assert L.phip_group_receive_datagrams(None, w, 0, None, None, None, D) == -1
    assert L.phip_group_receive_datagrams(g, None, 0, None, None, None, D) == -1
    assert L.phip_group_receive_datagrams(g, w, 0, None, None, None, 0) == -1
    assert L.phip_group_receive_datagrams(g, w, 0, None, None, None, _lib.ROUTE_COMBINE) == -1
    for bit in (0x10, 0x20, 0x100, 0x8000_0000):
        assert not bit & ALLOWED
        assert L.phip_group_receive_datagrams(g, w, 0, None, None, None, D | bit) == -1


def test_group_ring_receive_refuses_before_any_device_call():
    L = _lib.load()
    keep, g = _dummy()
    rings = (C.c_void_p * 1)()
    slots = (C.c_uint32 * 1)()
    D = _lib.DEVICE_PTRS
    assert L.phip_group_ring_receive(None, rings, slots, 0, None, None, None, D) == -1
    assert L.phip_group_ring_receive(g, None, slots, 0, None, None, None, D) == -1
    assert L.phip_group_ring_receive(g, rings, None, 0, None, None, None, D) == -1
    assert L.phip_group_ring_receive(g, rings, slots, 0, None, None, None, 0) == -1
    assert L.phip_group_ring_receive(g, rings, slots, 0, None, None, None, D | 0x40) == -1


def test_route_pack_datagrams_refuses_before_any_device_call():
    L = _lib.load()
    keep, h = _dummy()
    w = _lib.phip_wire()
    cnt = (C.c_uint64 * 64)()
    D = _lib.DEVICE_PTRS
    a = C.addressof(cnt)

    def call(h, w, world, flags, counts=a, nbytes=a):
        return L.phip_route_pack_datagrams(h, w, world, None, None, None, None, None, counts, nbytes,
                                           None, flags)
    assert call(None, C.byref(w), 2, D) == -1
    assert call(h, None, 2, D) == -1
    assert call(h, C.byref(w), 2, 0) == -1
    assert call(h, C.byref(w), 2, D | _lib.GROUP_RCCL_SELF) == -1
    assert call(h, C.byref(w), 2, D | 0x100) == -1
    assert call(h, C.byref(w), 0, D) == -1
    assert call(h, C.byref(w), 65, D) == -1
    assert call(h, C.byref(w), 2, D, counts=None) == -1
    assert call(h, C.byref(w), 2, D, nbytes=None) == -1
