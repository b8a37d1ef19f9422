"""Peek without a GPU (include/patrolhip.h "Peek"): the new symbols and
constants, and phip_peek_eval -- the host build of the function k_peek calls --
against tests/_peek_cases.py's reference: status, remaining and have bit-exact,
retry_at by its definition, the least-t claim by brute force, and the
monotonicity premise the bisection rests on.  No device calls."""
import ctypes as C
import os
import random
import re

import pytest

import patrol_amd
from patrol_amd import _lib
from oracle import go_semantics as G
from tests import _peek_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def peek_eval(q):
    return patrol_amd.peek_eval(*q)


def test_exports_and_constants():
    L = _lib.load()
    for name in ("phip_peek", "phip_peek_eval", "phip_api_peek"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert C.sizeof(_lib.phip_peek_results) == 40
    src = open(os.path.join(ROOT, "include", "patrolhip.h")).read()
    assert re.search(r"#define PHIP_PEEK_NEVER INT64_MIN\b", src)
    assert int(re.search(r"PHIP_ST_ABSENT = (0x[0-9a-fA-F]+)", src).group(1), 16) == _lib.ST_ABSENT == \
        PC.ABSENT == 0x40
    assert _lib.PEEK_NEVER == PC.NEVER == -(1 << 63)
    assert (_lib.ST_TAKE_OK, _lib.ST_TAKE_DENIED) == (PC.OK, PC.DENIED)
    assert re.search(r"#define PHIP_ABI_VERSION 3\b", src) and L.phip_abi_version() == 3


@pytest.fixture(scope="module")
def mixed():
    """20 000 mixed cases, their references, and the mix's conditions (asserted
    from the reference alone, before anything is compared)."""
    cases = PC.mixed_cases(20240611, 20000)
    refs = [PC.reference(*q) for q in cases]
    k, absent = PC.check_mix(refs)
    print("mix: %s, %d absent of %d" % (k, absent, len(cases)))
    return cases, refs


def test_peek_eval_matches_reference(mixed):
    cases, refs = mixed
    for q, ref in zip(cases, refs):
        st, rem, have, at = peek_eval(q)
        # (phip_peek_eval has no table: the absent flag is the caller's)
        assert (st, rem, have) == (ref["status"] & ~PC.ABSENT, ref["remaining"], ref["have"]), (q, ref)
        PC.check_retry(ref, q, at)


def test_retry_at_is_the_least_reading_brute_force():
    """Rates whose interval is 1-7 ns, counts <= 50: the first granted reading
    of a scan now .. now + 2000 is retry_at."""
    rng = random.Random(77)
    scanned = found = 0
    while scanned < 300:
        iv = rng.randrange(1, 8)
        freq = rng.randrange(1, 60)
        per = freq * iv + rng.randrange(0, freq)
        assert per // freq == iv
        count = rng.randrange(1, 51)
        tokens = rng.choice([0, 0.5, float(rng.randrange(0, 50))])
        added = float(freq + rng.randrange(0, 100))
        state = (G.f2b(added), G.f2b(added - tokens), rng.randrange(0, 10**6), PC.T0)
        now = state[2] + state[3] + rng.randrange(0, 20)
        q = (state, now, freq, per, count)
        ref = PC.reference(*q)
        if ref["klass"] == "ok":
            continue
        scanned += 1
        at = peek_eval(q)[3]
        first = next((t for t in range(now, now + 2001) if PC.ok_at(state, t, freq, per, count)), None)
        if first is None:
            assert at == PC.NEVER or at > now + 2000, (q, at)
        else:
            found += 1
            assert at == first, (q, at, first)
    assert found >= 150, found


def test_ok_is_monotone_from_a_denial(mixed):
    """The premise: over sorted sample readings >= now, ok() of a denied query
    never goes from true back to false."""
    cases, refs = mixed
    rng = random.Random(5)
    denied = [(q, r) for q, r in zip(cases, refs) if r["klass"] != "ok"][:5000]
    assert len(denied) == 5000
    turned = 0
    for q, ref in denied:
        _, now, freq, per, count = q
        s = ref["s"]
        iv = abs(per // freq) if freq and per else 1
        ts = {now, PC.I64_MAX}
        room = PC.I64_MAX - now
        for _ in range(200):   # (24 readings; fewer when now leaves no room for them)
            if len(ts) >= min(24, room + 1):
                break
            r = rng.random()
            if r < 0.4:
                d = rng.randrange(0, 1 << rng.randrange(1, 64))
            elif r < 0.8:
                d = rng.randrange(0, 400) * max(iv, 1) + rng.randrange(-2, 3)
            else:
                d = rng.randrange(0, 1 << 20)
            t = now + d
            if now <= t <= PC.I64_MAX:
                ts.add(t)
        seen = False
        for t in sorted(ts):
            ok = PC.ok_at(s, t, freq, per, count)
            assert ok or not seen, (q, t)
            seen = seen or ok
        turned += seen
    assert turned > 500, turned


def test_null_arguments():
    L = _lib.load()
    q = _lib.phip_ops()
    assert L.phip_peek(None, C.byref(q), None, 0) == -1
    rem, have, at = C.c_uint64(), C.c_uint64(), C.c_int64()
    assert L.phip_peek_eval(None, 0, 1, 1, 1, C.byref(rem), C.byref(have), None) == -1
    assert L.phip_peek_eval(None, 0, 1, 1, 1, None, C.byref(have), C.byref(at)) == -1
    # an absent bucket, one token a nanosecond, capacity 1: granted, nothing left
    assert L.phip_peek_eval(None, 5, 1, 1, 1, C.byref(rem), C.byref(have), C.byref(at)) == PC.OK
    assert (rem.value, have.value, at.value) == (0, 0, 5)


def test_api_peek_name_too_large_needs_no_handle():
    L = _lib.load()
    body, bl, after = C.create_string_buffer(64), C.c_uint32(), C.c_int64(-7)
    name = b"A" * 232
    code = L.phip_api_peek(None, name, len(name), b"1:s", 3, b"1", 1, PC.T0, body, C.byref(bl),
                           C.byref(after))
    assert (code, body.raw[:bl.value].decode()) == G.api_take(G.LocalRepo(), "A" * 232, "1:s", "1", PC.T0)
    assert code == 400 and after.value == -7
    assert L.phip_api_peek(None, b"a", 1, b"1:s", 3, b"1", 1, PC.T0, body, C.byref(bl), None) == -1
