"""The top-talkers model (include/patrolhip.h "Top talkers"), shared by
tests/test_top_abi.py (CPU) and tests/test_top.py (GPU).  Nothing here calls
the library.

The contract, restated over the rows of a dump, {name: (added bits, taken
bits, elapsed, created)}.  A bucket qualifies iff its name is at most 231
bytes, it starts with the prefix (tests/_throttled_cases.match with one rule),
with idle_ns > 0 it is not idle at `now` -- idle = now - (created + elapsed) in
exact integers, 0 when negative, saturating at INT64_MAX; idle iff idle >=
idle_ns -- and its taken bits t satisfy 0 < t <= 0x7FF0000000000000.  The list
is by t descending; equal t falls in slot order, which a dump does not show,
so a result is checked by check(): the sequence of keys, every entry true of
the dump, distinct names, the exact set above the last key, a subset of the
right size at it.

merge(): phip_top_merge restated -- one entry per name (the larger taken; equal
taken: the earlier list, then position), then by taken descending, list, position.
"""
from __future__ import annotations

import random

import numpy as np

from tests import _throttled_cases as TC

MAX_NAME = 231
TOP_MAX = 4096
INF = 0x7FF0000000000000
SIGN = 1 << 63
I64_MAX = (1 << 63) - 1
T0, SEC = TC.T0, TC.SEC
ONE = 0x3FF0000000000000   # 1.0


def f2b(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def idle_of(created, elapsed, now):
    last = created + elapsed
    if now < last:
        return 0
    return min(now - last, I64_MAX)


def qualifies(name, st, prefix=b"", now=0, idle_ns=0):
    a, t, e, c = st
    if len(name) > MAX_NAME or TC.match([(prefix,)], name) < 0:
        return False
    if idle_ns > 0 and idle_of(c, e, now) >= idle_ns:
        return False
    return 0 < t <= INF


def reference(rows, prefix=b"", now=0, idle_ns=0):
    """-> {name: taken bits} of the buckets that qualify."""
    return {nm: st[1] for nm, st in rows.items() if qualifies(nm, st, prefix, now, idle_ns)}


def rows_of(dump):
    return {k: (v.added, v.taken, v.elapsed, v.created) for k, v in dump.items()}


def entries(d):
    """A result dict -> [(name, taken, state tuple or None)]."""
    out = []
    for i, nm in enumerate(d["names"]):
        s = None
        if d.get("state") is not None:
            r = d["state"][i]
            s = (int(r["a"]), int(r["t"]), int(r["e"]), int(r["c"]))
        out.append((nm, int(d["taken"][i]), s))
    return out


def check(d, rows, k, prefix=b"", now=0, idle_ns=0, cut=False):
    """The set conditions on one result.  cut: names_cap may have ended the
    list early (then n is whatever was reported, and truncated says so)."""
    ref = reference(rows, prefix, now, idle_ns)
    keys = sorted(ref.values(), reverse=True)
    want = min(k, len(ref))
    n = d["n"]
    assert d["population"] == len(ref), (d["population"], len(ref))
    if cut:
        assert n <= want and d["truncated"] == int(n < want), (n, want, d["truncated"])
    else:
        assert n == want and d["truncated"] == 0, (n, want, d["truncated"])
    got = entries(d)
    assert len(got) == n == len(d["taken"])
    assert d["bytes"] == sum(len(e[0]) for e in got)
    assert [e[1] for e in got] == keys[:n]
    names = [e[0] for e in got]
    assert len(set(names)) == n, "a bucket was reported twice"
    for nm, t, s in got:
        assert nm in ref and ref[nm] == t, (nm, t)
        if s is not None:
            assert s == tuple(rows[nm]), (nm, s, rows[nm])
    if n:
        last = got[-1][1]
        assert {nm for nm, t, _ in got if t > last} == {nm for nm, t in ref.items() if t > last}
        assert {nm for nm, t, _ in got if t == last} <= {nm for nm, t in ref.items() if t == last}
    return got


# ------------------------------------------------------------- tables ----
def name_classes(rng, n):
    """n distinct names over the throttled recipe's classes: the empty name,
    inline names, 23..231-byte names."""
    return TC.make_names(rng, n)


def distinct_table(seed=7, n=600):
    """-> (names, cols, rows): distinct positive taken values, plain states."""
    rng = random.Random(seed)
    names = name_classes(rng, n)
    vals = rng.sample(range(1, 50 * n), n)
    t = np.array([f2b(float(v) / 4) for v in vals], np.uint64)
    a = np.array([f2b(float(v) / 4 + rng.randrange(1, 100)) for v in vals], np.uint64)
    e = np.array([rng.randrange(0, 1 << 40) for _ in range(n)], np.int64)
    c = np.array([T0 + rng.randrange(-1000, 1000) * SEC for _ in range(n)], np.int64)
    cols = [a, t, e, c]
    rows = {nm: (int(a[i]), int(t[i]), int(e[i]), int(c[i])) for i, nm in enumerate(names)}
    return names, cols, rows


BASE = 0x4000000000000000
SHIFTS = [0, 7, 8, 10, 11, 12, 15, 16, 31, 32, 47, 52]
NON_RANKING = [0, SIGN, f2b(-1.0), SIGN | INF, INF + 1, SIGN | (INF + 12345), 0x7FF8000000000000,
               0xFFF8000000000001]


def boundary_table(s):
    """8 buckets with taken bits BASE + (i << s), i = 1..8, +Inf, the smallest
    denormal, and the values that never rank.  -> (names, cols, rows)."""
    t = [BASE + (i << s) for i in range(1, 9)] + [INF, 1] + NON_RANKING
    names = [b"fam-%d" % i for i in range(1, 9)] + [b"inf", b"denormal"] + \
        [b"never-%d" % i for i in range(len(NON_RANKING))]
    n = len(t)
    a = np.full(n, f2b(5.0), np.uint64)
    cols = [a, np.array(t, np.uint64), np.full(n, 1, np.int64), np.full(n, T0, np.int64)]
    rows = {nm: (f2b(5.0), t[i], 1, T0) for i, nm in enumerate(names)}
    return names, cols, rows


# -------------------------------------------------------------- merge ----
def merge(lists, k):
    """lists: [[(name, taken, state)]] -> the first k of the merged order."""
    best = {}
    for li, lst in enumerate(lists):
        for pos, (nm, t, s) in enumerate(lst):
            key = (-t, li, pos)
            if nm not in best or key < best[nm][0]:
                best[nm] = (key, (nm, t, s))
    return [e for _, e in sorted(best.values(), key=lambda x: x[0])][:k]


def merge_cases():
    """-> [(label, lists, k)] with lists of (name, taken bits, state tuple)."""
    rng = random.Random(23)

    def lst(names, takens):
        rows = [(nm, t, (t + 7, t, rng.randrange(1 << 30), T0 + rng.randrange(1000)))
                for nm, t in zip(names, takens)]
        return sorted(rows, key=lambda r: -r[1])

    def tk(v):
        return f2b(float(v))
    cases = []
    a = lst([b"a%d" % i for i in range(40)], [tk(rng.randrange(1, 10 ** 6)) for _ in range(40)])
    b = lst([b"b%d" % i + b"x" * (i * 5) for i in range(40)], [tk(rng.randrange(1, 10 ** 6)) for _ in range(40)])
    c = lst([b"", b"c"], [tk(5), tk(10 ** 7)])
    cases.append(("disjoint", [a, b, c], 30))
    cases.append(("k above the total", [a, b, c], 4096))
    cases.append(("one list", [a], 7))
    cases.append(("an empty list among them", [a, [], c], 50))
    cases.append(("only empty lists", [[], []], 5))
    # a name in two lists with different taken, and with equal taken
    d1 = lst([b"shared", b"d1", b"same"], [tk(100), tk(50), tk(70)])
    d2 = lst([b"shared", b"d2", b"same"], [tk(300), tk(60), tk(70)])
    cases.append(("a name in two lists", [d1, d2], 10))
    cases.append(("a name in two lists, reversed", [d2, d1], 10))
    cases.append(("a name in two lists, cut", [d1, d2], 2))
    # ties across lists fall by list index, then position
    t1 = lst([b"t1-%d" % i for i in range(6)], [tk(9)] * 6)
    t2 = lst([b"t2-%d" % i for i in range(6)], [tk(9)] * 4 + [tk(11)] * 2)
    cases.append(("ties across lists", [t1, t2], 5))
    cases.append(("ties across lists, all", [t1, t2], 12))
    cases.append(("+Inf and a denormal", [lst([b"inf", b"tiny"], [INF, 1]), lst([b"one"], [ONE])], 3))
    return cases
