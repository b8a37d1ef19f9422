"""CPU checks of tests/_columns.py: the op streams against the oracle (every
column shows enough default and enough non-default entries, over each fold
class too, so that no GPU case can pass vacuously), the poison byte against
the status list, the thresholds against the kernel header, and the helper
against itself (a write one byte outside a column, and an unwritten entry, are
each caught)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import _columns as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def reference(stream):
    o = O.Repo()
    stream.seed_into(o)
    return RC.expected_mixed(stream.kind, o.apply_mixed(*stream.args))


# ------------------------------------------------------------------ constants --
def test_poison_is_no_status():
    vals = {name: int(v, 0) for name, v in
            re.findall(r"PHIP_ST_(\w+) = (0x[0-9A-Fa-f]+|\d+)", read("include", "patrolhip.h"))}
    assert len(vals) >= 10 and vals["MERGED"] == RC.ST_MERGED and vals["CREATED"] == RC.ST_CREATED
    flags = vals["CREATED"] | vals["ABSENT"]
    codes = {v for k, v in vals.items() if k not in ("CREATED", "ABSENT")}
    assert RC.POISON not in codes and (RC.POISON & ~flags) not in codes
    # nor a plausible result: as a float64 the pattern is a huge negative number
    word = np.frombuffer(bytes([RC.POISON]) * 8, np.uint64)[0]
    assert word.view(np.float64) < -1e-100 and int(word) > 1 << 63


def test_thresholds_are_the_kernels():
    src = read("patrol_amd", "csrc", "phip_kernels.hpp")
    assert int(re.search(r"constexpr u32 kSmallMax = (\d+);", src).group(1)) == RC.SMALL_MAX
    assert int(re.search(r"constexpr u32 kLongSeg = (\d+);", src).group(1)) == RC.LONG_SEG
    assert int(re.search(r"#define PHIP_HUGE_SEG (\d+)", src).group(1)) == RC.HUGE_SEG
    bits = re.search(r"kOutStatus = (\d+), kOutRem = (\d+), kOutHave = (\d+), kOutReply = (\d+);", src)
    assert tuple(int(x) for x in bits.groups()) == tuple(RC.BIT[c] for c in RC.COLUMNS)


# -------------------------------------------------------------------- streams --
def test_small_stream_shows_both_halves_of_every_column():
    s = RC.small_stream()
    assert s.n < RC.SMALL_MAX and s.cls.max() > RC.LONG_SEG
    want = reference(s)
    RC.assert_shares(RC.shares(s.kind, want), "small stream")
    st = want["status"]
    # the kinds the issue lists, and buckets the batch itself creates
    assert {RC.TAKE, RC.RECEIVE, RC.UPSERT} == set(s.kind.tolist())
    assert ((st & 0x7F) == RC.ST_INCAST_REPLY).sum() >= 4
    assert ((s.kind == RC.RECEIVE) & (s.added == RC.NEG_ZERO)).sum() >= 4
    assert ((st & RC.ST_CREATED) != 0).sum() >= 64
    # the wave fold's own ops
    RC.assert_shares(RC.shares(s.kind, want, s.cls > RC.LONG_SEG), "small stream, long buckets")


def test_large_stream_shows_both_halves_in_every_fold_class():
    s = RC.large_stream()
    want = reference(s)
    RC.assert_shares(RC.shares(s.kind, want), "large stream")
    sizes = set(s.cls.tolist())
    assert set(RC.WAVE_SIZES) <= sizes and max(sizes) > RC.HUGE_SEG
    for label, m in s.classes().items():
        RC.assert_shares(RC.shares(s.kind, want, m), "large stream, %s fold" % label)
    # the hot bucket's Takes denied with nothing to have: the drained runs
    hot = s.classes()["block"] & (s.kind == RC.TAKE)
    assert ((want["status"][hot] == RC.ST_TAKE_DENIED) & (want["have"][hot] == 0)).sum() >= 64


def test_medium_stream_shows_both_halves_without_a_huge_bucket():
    s = RC.medium_stream()
    assert s.n > RC.SMALL_MAX and RC.LONG_SEG < s.cls.max() <= RC.HUGE_SEG
    want = reference(s)
    RC.assert_shares(RC.shares(s.kind, want), "medium stream")
    cl = s.classes()
    assert not cl["block"].any()
    for label in ("thread", "wave"):
        RC.assert_shares(RC.shares(s.kind, want, cl[label]), "medium stream, %s fold" % label)


def test_stain_is_non_default_everywhere():
    ops = RC.stain_ops(3000)
    want = RC.expected_mixed(ops[0], O.Repo().apply_mixed(*ops))
    for c in RC.COLUMNS:
        assert not RC.is_default(c, want[c]).any(), c


def test_receive_expectation_stops():
    names = [b"a", b"b", b"a", b"c"]
    a = np.array([RC.f2b(3), 0, 0, RC.f2b(1)], np.uint64)
    t = np.array([RC.f2b(1), 0, 0, RC.f2b(1)], np.uint64)
    e = np.array([5, 0, 0, 7], np.int64)
    want = RC.expected_receive(O.Repo(), names, a, t, e, 99, stop=3)
    assert want["status"].tolist() == [RC.ST_MERGED | RC.ST_CREATED,
                                       RC.ST_INCAST_NOREPLY | RC.ST_CREATED,
                                       RC.ST_INCAST_REPLY, RC.ST_SHORT]
    assert want["reply"][2].tolist() == (RC.f2b(3), RC.f2b(1), 5, 99)
    assert RC.is_default("reply", want["reply"]).tolist() == [True, False, False, True]
    assert not want["remaining"].any() and not want["have"].any()


# --------------------------------------------------------------------- helper --
@pytest.mark.parametrize("misaligned", [True, False])
@pytest.mark.parametrize("name", RC.COLUMNS)
def test_layout(name, misaligned):
    col = RC.Column(name, 7, "host", misaligned)
    size = RC.DTYPE[name].itemsize
    assert col.off >= RC.GUARD and len(col.bytes()) - col.off - 7 * size == RC.GUARD
    assert col.ptr % min(size, 8) == 0
    nxt = {"status": 2, "remaining": 16, "have": 16, "reply": 32}[name]
    assert (col.ptr % nxt != 0) == misaligned
    assert (col.check().view(np.uint8) == RC.POISON).all()


def fill(col, value=0):
    C.memset(col.ptr, value, col.nbytes)


@pytest.mark.parametrize("name", RC.COLUMNS)
def test_a_write_outside_the_column_is_caught(name):
    for where in (-1, None):
        col = RC.Column(name, 5, "host")
        fill(col)
        col.check()
        addr = col.ptr - 1 if where == -1 else col.ptr + col.nbytes
        C.memset(addr, 0, 1)
        with pytest.raises(AssertionError, match="before" if where == -1 else "after"):
            col.check()


@pytest.mark.parametrize("name", RC.COLUMNS)
def test_an_unwritten_entry_is_caught(name):
    """Every entry written with the right (all-default) values but one."""
    n = 9
    res = RC.Results(n, RC.BIT[name], "host")
    col = res.cols[name]
    want = {name: np.zeros(n, RC.DTYPE[name])}
    if name == "status":
        want[name][:] = RC.ST_MERGED
    size = col.dtype.itemsize
    raw = want[name].view(np.uint8)
    C.memmove(col.ptr, raw.ctypes.data, 4 * size)
    C.memmove(col.ptr + 5 * size, raw.ctypes.data + 5 * size, 4 * size)
    with pytest.raises(AssertionError, match="entry 4"):
        RC.compare(res.check(), want)
    C.memmove(col.ptr + 4 * size, raw.ctypes.data + 4 * size, size)
    RC.compare(res.check(), want)


def test_results_builder_passes_null_for_absent_columns():
    for mask in range(16):
        res = RC.Results(3, mask, "host")
        for c in RC.COLUMNS:
            p = getattr(res.struct, c)
            assert (p is not None) == bool(mask & RC.BIT[c])
            if p is not None:
                assert p == res.cols[c].ptr
