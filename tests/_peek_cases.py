"""Peek (include/patrolhip.h "Peek"): the reference and the seeded case mix
shared by tests/test_peek_abi.py (CPU) and tests/test_peek.py (GPU).

Reference.  A query (state or None, now, freq, per, count) is evaluated by the
C++ oracle's pure Take (oracle.take_fields) on a copy of the state; an absent
bucket (None) is the zero state with created = now, what GetBucket would have
created (repo.go:189-211).  status, remaining and have are compared on bit
patterns.  retry_at has no formula here: it is checked by its definition, with
ok(t) = the same evaluation at the clock reading t:
    granted            retry_at == now
    a finite answer    retry_at > now, ok(retry_at), not ok(retry_at - 1)
    PEEK_NEVER         not ok(INT64_MAX)
(the least such t, given that from a denial ok() turns true at most once:
test_peek_abi.py checks that premise itself, and the least-t claim by brute
force where the answer is near).
"""
from __future__ import annotations

import random

import numpy as np

from oracle import go_semantics as G
from oracle import oracle as O

OK, DENIED, ABSENT = 6, 7, 0x40
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
NEVER = I64_MIN
T0, SEC = 1_700_000_000_000_000_000, 10**9


# ------------------------------------------------------------- reference ----
def evaluated(state, now):
    """The state a query is evaluated on."""
    return (0, 0, 0, now) if state is None else tuple(int(x) for x in state)


def take_at(s, t, freq, per, count):
    """Take on a copy of s at the reading t -> (remaining, ok, have bits)."""
    rem, ok, have = O.take_fields([G.b2f(s[0]), G.b2f(s[1]), s[2]], s[3], t, freq, per, count)
    return rem, ok, G.f2b(have)


def ok_at(s, t, freq, per, count):
    return take_at(s, t, freq, per, count)[1]


def reference(state, now, freq, per, count):
    """-> dict(status, remaining, have, klass, s): klass is "ok", "finite" (denied,
    some later reading grants) or "never"."""
    s = evaluated(state, now)
    rem, ok, have = take_at(s, now, freq, per, count)
    klass = "ok" if ok else ("finite" if ok_at(s, I64_MAX, freq, per, count) else "never")
    return dict(status=(OK if ok else DENIED) | (ABSENT if state is None else 0), remaining=rem,
                have=have, klass=klass, s=s)


def check_retry(ref, q, retry_at):
    """retry_at against its definition."""
    _, now, freq, per, count = q
    s, klass = ref["s"], ref["klass"]
    if klass == "ok":
        assert retry_at == now, (q, retry_at)
    elif klass == "never":
        assert retry_at == NEVER, (q, retry_at)
    else:
        assert now < retry_at <= I64_MAX, (q, retry_at)
        assert ok_at(s, retry_at, freq, per, count), (q, retry_at)
        assert not ok_at(s, retry_at - 1, freq, per, count), (q, retry_at)


def check_one(q, got):
    """got = (status, remaining, have bits, retry_at) of the query q."""
    ref = reference(*q)
    assert (int(got[0]), int(got[1]), int(got[2])) == (ref["status"], ref["remaining"], ref["have"]), \
        (q, got, ref)
    check_retry(ref, q, int(got[3]))
    return ref


def check_mix(refs):
    """The conditions on a case mix, from the reference alone."""
    n = len(refs)
    k = {c: sum(r["klass"] == c for r in refs) for c in ("ok", "finite", "never")}
    absent = sum(bool(r["status"] & ABSENT) for r in refs)
    assert k["ok"] >= 0.2 * n and k["finite"] >= 0.2 * n and k["never"] >= 0.1 * n, (k, n)
    assert absent >= 0.1 * n, (absent, n)
    return k, absent


# ------------------------------------------------------------------ cases ----
F64_EDGES = [0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000001,   # NaNs
             0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
             G.f2b(-1.0), G.f2b(-1e300), G.f2b(2.0**53), G.f2b(2.0**53 + 2), 0x1,
             0x8000000000000001, 0x000FFFFFFFFFFFFF, G.f2b(1.0), G.f2b(0.5), G.f2b(100.0),
             G.f2b(1e18), G.f2b(2.0**63), G.f2b(2.0**64), G.f2b(-3.0)]
I64_EDGES = [0, 1, -1, I64_MAX, I64_MIN, I64_MAX - 1, I64_MIN + 1, 1 << 62, -(1 << 62), T0,
             T0 + SEC, -T0]
RATE_EDGES = [(0, SEC), (5, 0), (0, 0), (-3, SEC), (3, -SEC), (-3, -SEC), (10, 3), (-1, I64_MIN),
              (1, I64_MAX), (I64_MAX, I64_MAX), (1, 1), (2, 7), (I64_MIN, I64_MIN), (100, SEC),
              (3, SEC), (30, 60 * SEC)]
COUNT_EDGES = [0, 1, 2, 5, 101, 1 << 63, (1 << 64) - 1, (1 << 53) + 1]
PLAIN_RATES = [(100, SEC), (3, SEC), (30, 60 * SEC)]


def _clamp(v):
    return max(I64_MIN, min(I64_MAX, v))


def extreme_state(rng):
    def f():
        if rng.random() < 0.6:
            return rng.choice(F64_EDGES)
        return G.f2b(float(rng.choice([rng.randrange(0, 200), rng.random() * 100,
                                       -rng.randrange(0, 50)])))

    def i(base):
        if rng.random() < 0.5:
            return rng.choice(I64_EDGES)
        return _clamp(base + rng.randrange(-(1 << 40), 1 << 40))
    return (f(), f(), i(0), i(T0))


def plain_state(rng, rate=None):
    """A partly drained bucket of one of the plain rates -> (state, rate)."""
    freq, per = rate or rng.choice(PLAIN_RATES)
    refilled = rng.randrange(0, 3 * freq)
    tokens = rng.choice([0, 0, 1, rng.randrange(0, freq + 1)])
    added = float(freq + refilled)
    elapsed = refilled * (per // freq) + rng.randrange(0, per)
    return (G.f2b(added), G.f2b(added - tokens), elapsed, T0 - rng.randrange(0, 100 * SEC)), \
        (freq, per)


def extreme_query(rng, state):
    """(now, freq, per, count) drawn against `state` (None: absent)."""
    freq, per = rng.choice(RATE_EDGES) if rng.random() < 0.7 else \
        (rng.randrange(1, 1000), rng.randrange(1, 10 * SEC))
    count = rng.choice(COUNT_EDGES) if rng.random() < 0.6 else rng.randrange(0, 300)
    last = T0 if state is None else _clamp(state[2] + state[3])
    r = rng.random()
    if r < 0.3:
        now = rng.choice(I64_EDGES)
    elif r < 0.45:
        now = _clamp(last - rng.randrange(1, 1 << 30))      # before `last`
    elif r < 0.55:
        now = -rng.randrange(1, 1 << 62)
    else:
        now = _clamp(last + rng.randrange(0, 1 << rng.randrange(1, 50)))
    return now, freq, per, count


def plain_query(rng, state, rate):
    freq, per = rate
    last = T0 if state is None else _clamp(state[2] + state[3])
    iv = per // freq
    now = _clamp(last + rng.choice([0, rng.randrange(0, iv), rng.randrange(0, 3 * iv),
                                    rng.randrange(0, 2 * per)]))
    count = rng.choice([1, 2, 2, 3, 5, rng.randrange(1, freq + 1), freq, freq + 1, 3 * freq])
    return now, freq, per, count


def mixed_cases(seed, n, p_absent=0.15):
    """n queries (state or None, now, freq, per, count): half from the edge
    lists, half plain."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        absent = rng.random() < p_absent
        if k & 1:
            state, rate = plain_state(rng)
            state = None if absent else state
            out.append((state,) + plain_query(rng, state, rate))
        else:
            state = None if absent else extreme_state(rng)
            out.append((state,) + extreme_query(rng, state))
    return out


# ---------------------------------------------------------------- a table ----
def table_names(rng, n):
    """n distinct present names over the name classes, and absent names that
    share prefixes (and, on a handle with debug_tag_bits, tags) with them."""
    classes = [(0, 0), (1, 14), (15, 22), (23, 40), (200, 231)]
    present, seen = [], set()
    for draw in range(100 * n):   # (the classes in turn; the empty name is taken once)
        if len(present) == n:
            break
        lo, hi = classes[draw % len(classes)]
        nm = bytes(rng.randrange(97, 123) for _ in range(rng.randrange(lo, hi + 1)))
        if nm not in seen:
            seen.add(nm)
            present.append(nm)
    absent = []
    for nm in present:
        for cand in (nm + b"x", nm[:-1], nm[:16] + b"#" + nm[17:], nm[:-1] + b"~"):
            if cand not in seen and len(cand) <= 231:
                seen.add(cand)
                absent.append(cand)
                break
    return present, absent


def table_case(seed, n_buckets=600):
    """Seeded buckets (names, a, t, e, c arrays, per-bucket rate or None) for a
    table: half extreme states, half plain."""
    rng = random.Random(seed)
    present, absent = table_names(rng, n_buckets)
    states, rates = [], []
    for k in range(n_buckets):
        if k & 1:
            s, r = plain_state(rng)
        else:
            s, r = extreme_state(rng), None
        states.append(s)
        rates.append(r)
    cols = [np.array([s[j] for s in states], np.uint64 if j < 2 else np.int64) for j in range(4)]
    return dict(names=present, absent=absent, states=states, rates=rates, cols=cols)


def table_queries(seed, tab, n, p_absent=0.15):
    """n queries over a table_case -> list of (name, now, freq, per, count)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        if rng.random() < p_absent:
            name, state, rate = rng.choice(tab["absent"]), None, None
        else:
            k = rng.randrange(len(tab["names"]))
            name, state, rate = tab["names"][k], tab["states"][k], tab["rates"][k]
        if rate is None and rng.random() < 0.5:
            q = extreme_query(rng, state)
        else:
            q = plain_query(rng, state, rate or rng.choice(PLAIN_RATES))
        out.append((name,) + q)
    return out


def columns(queries):
    """(name, now, freq, per, count) rows -> names list and numpy columns."""
    names = [q[0] for q in queries]
    now, freq, per = (np.array([q[j] for q in queries], np.int64) for j in (1, 2, 3))
    count = np.array([q[4] for q in queries], np.uint64)
    return names, now, freq, per, count
