"""The windowed top-talkers model (include/patrolhip.h "Windowed top
talkers"), shared by tests/test_usage_abi.py (CPU) and tests/test_usage.py
(GPU).  Nothing here calls the library.

The contract, restated over two dumps, the rows at the mark and the rows now,
each {name: (added bits, taken bits, elapsed, created)}.  A bucket's key is
bits(float64(taken now) - float64(base)), one IEEE subtraction (numpy's), with
base = +0.0 for a name the rows at the mark do not hold.  It ranks iff it
passes every test of tests/_top_cases.qualifies except the one on `taken`
itself, and 0 < key <= 0x7FF0000000000000.  The list is by key descending;
equal keys fall in slot order, which a dump does not show, so a result is
checked by check(): the key sequence, every entry true of the model, distinct
names, the exact set above the last key, a subset at it, and state equal to
the current row.

plan(): the activity recipe, a deterministic list of steps over the 600 names
of _top_cases.distinct_table(7, 600), and run_model(), the same steps through
the Go restatement (oracle/go_semantics.py), so that the classes the recipe
promises are asserted without a GPU.

edge_table(): (base, taken) pairs whose differences round, vanish, overflow the
range test or sit on the radix select's digit boundaries.
"""
from __future__ import annotations

import numpy as np

from oracle import go_semantics as G
from tests import _top_cases as TP

INF, SIGN, ONE = TP.INF, TP.SIGN, TP.ONE
T0, SEC = TP.T0, TP.SEC
f2b = TP.f2b


def b2f(b):
    return np.array([b], np.uint64).view(np.float64)[0]


def delta_bits(taken_bits, base_bits=0):
    """bits(taken - base): one float64 subtraction, round to nearest."""
    with np.errstate(all="ignore"):
        return int(np.array([b2f(taken_bits) - b2f(base_bits)], np.float64).view(np.uint64)[0])


def passes_filters(name, st, prefix=b"", now=0, idle_ns=0):
    """Every test of metric 0 except the one on `taken` itself."""
    a, _, e, c = st
    return TP.qualifies(name, (a, ONE, e, c), prefix, now, idle_ns)


def reference(rows_mark, rows_now, prefix=b"", now=0, idle_ns=0):
    """-> {name: key bits} of the buckets that rank since the mark."""
    out = {}
    for nm, st in rows_now.items():
        if not passes_filters(nm, st, prefix, now, idle_ns):
            continue
        d = delta_bits(st[1], rows_mark[nm][1] if nm in rows_mark else 0)
        if 0 < d <= INF:
            out[nm] = d
    return out


def active(rows_mark, rows_now):
    """phip_usage_stats.active of a mark taken now: names of any length."""
    return sum(0 < delta_bits(st[1], rows_mark[nm][1] if nm in rows_mark else 0) <= INF
               for nm, st in rows_now.items())


def check(d, rows_mark, rows_now, k, prefix=b"", now=0, idle_ns=0, cut=False):
    """TP.check for metric 1: `taken` holds the key, `state` the current row."""
    ref = reference(rows_mark, rows_now, prefix, now, idle_ns)
    keys = sorted(ref.values(), reverse=True)
    want = min(k, len(ref))
    n = d["n"]
    assert d["population"] == len(ref), (d["population"], len(ref))
    if cut:
        assert n <= want and d["truncated"] == int(n < want), (n, want, d["truncated"])
    else:
        assert n == want and d["truncated"] == 0, (n, want, d["truncated"])
    got = TP.entries(d)
    assert len(got) == n == len(d["taken"])
    assert d["bytes"] == sum(len(e[0]) for e in got)
    assert [e[1] for e in got] == keys[:n]
    assert len(set(e[0] for e in got)) == n, "a bucket was reported twice"
    for nm, t, s in got:
        assert nm in ref and ref[nm] == t, (nm, t)
        if s is not None:
            assert s == tuple(rows_now[nm]), (nm, s, rows_now[nm])
    if n:
        last = got[-1][1]
        assert {nm for nm, t, _ in got if t > last} == {nm for nm, t in ref.items() if t > last}
        assert {nm for nm, t, _ in got if t == last} <= {nm for nm, t in ref.items() if t == last}
    return got


# ----------------------------------------------------- the activity recipe ----
N_SEED = 600
MERGED = slice(0, 150)        # raised by receive merges, distinct differences
TOOK_ONE = slice(150, 200)    # raised by take(count = 1): one difference, 50 buckets
GROUPS = slice(200, 240)      # ten groups of four, take(count = 2 + g) through apply_mixed
UNTOUCHED = slice(240, 600)
N_NEW_TAKE, N_NEW_RECV = 25, 25
TAKE_NOW = T0 + 5000 * SEC    # past every seeded bucket's created + elapsed
FREQ, PER = 1000, SEC         # a full bucket of 1000 tokens by then: every take below is granted


def plan(seed=7):
    """-> (names, cols, rows, steps).  steps: [(call, args)] with call one of
    "receive" (names, added, taken, elapsed, now), "take" (names, now, freq,
    per, count) and "mixed" (kind, names, now, freq, per, count, added, taken,
    elapsed) -- the arguments of GPURepo.receive_soa / take / apply_mixed."""
    names, cols, rows = TP.distinct_table(seed, N_SEED)
    a, t, e, _ = cols
    steps = []
    # receive merges: taken raised by 2000.5 + i / 2 (all exact: multiples of 1/4 below 2^20)
    idx = range(*MERGED.indices(N_SEED))
    up = np.array([b2f(int(t[i])) + 2000.5 + i / 2 for i in idx], np.float64).view(np.uint64)
    steps.append(("receive", ([names[i] for i in idx], a[MERGED].copy(), up.copy(),
                              e[MERGED].copy(), TAKE_NOW)))
    # plain takes of one token
    idx = list(range(*TOOK_ONE.indices(N_SEED)))
    m = len(idx)
    steps.append(("take", ([names[i] for i in idx], np.full(m, TAKE_NOW, np.int64),
                           np.full(m, FREQ, np.int64), np.full(m, PER, np.int64),
                           np.ones(m, np.uint64))))
    # new names created by takes of 3 tokens (tied with group 1 below)
    new_t = [b"usage-new-take-%d" % i for i in range(N_NEW_TAKE)]
    steps.append(("take", (new_t, np.full(N_NEW_TAKE, TAKE_NOW, np.int64),
                           np.full(N_NEW_TAKE, FREQ, np.int64), np.full(N_NEW_TAKE, PER, np.int64),
                           np.full(N_NEW_TAKE, 3, np.uint64))))
    # one mixed batch: the groups' takes, and new names created by receives
    idx = list(range(*GROUPS.indices(N_SEED)))
    new_r = [b"org:usage-new-recv-%d" % i + b"r" * (i * 7) for i in range(N_NEW_RECV)]
    kind = np.array([0] * len(idx) + [1] * N_NEW_RECV, np.uint8)
    m = len(kind)
    cnt = np.array([2 + j // 4 for j in range(len(idx))] + [0] * N_NEW_RECV, np.uint64)
    rt = np.array([0.0] * len(idx) + [7.5 + i for i in range(N_NEW_RECV)], np.float64)
    steps.append(("mixed", (kind, [names[i] for i in idx] + new_r, np.full(m, TAKE_NOW + 1, np.int64),
                            np.full(m, FREQ, np.int64), np.full(m, PER, np.int64), cnt,
                            (rt + 50).view(np.uint64).copy(), rt.view(np.uint64).copy(),
                            np.ones(m, np.int64))))
    return names, cols, rows, steps


def run_model(rows, steps):
    """The steps through the Go restatement -> the rows after them."""
    repo = G.LocalRepo(*[G.Bucket(name=nm, added=b2f(s[0]), taken=b2f(s[1]), elapsed=s[2],
                                  created=s[3]) for nm, s in rows.items()])
    for call, args in steps:
        if call == "receive":
            nm, a, t, e, now = args
            for i, x in enumerate(nm):
                repo.receive_one(G.Bucket(name=x, added=b2f(a[i]), taken=b2f(t[i]),
                                          elapsed=int(e[i])), now)
        elif call == "take":
            nm, now, freq, per, cnt = args
            for i, x in enumerate(nm):
                st, _, _ = repo.take(x, int(now[i]), G.Rate(int(freq[i]), int(per[i])), int(cnt[i]))
                assert st & 0x7F == G.TAKE_OK, x
        else:
            kind, nm, now, freq, per, cnt, a, t, e = args
            out = repo.apply_mixed([(int(kind[i]), nm[i], int(now[i]), int(freq[i]), int(per[i]),
                                     int(cnt[i]), int(a[i]), int(t[i]), int(e[i]))
                                    for i in range(len(nm))])
            assert all(o[0] & 0x7F in (G.TAKE_OK, G.MERGED) for o in out)
    return {nm: (f2b(b.added), f2b(b.taken), b.elapsed, b.created) for nm, b in repo.buckets.items()}


def apply_steps(g, steps):
    """The steps through a GPURepo's real calls."""
    for call, args in steps:
        if call == "receive":
            g.receive_soa(*args)
        elif call == "take":
            g.take(*args)
        else:
            g.apply_mixed(*args)


def tie_groups(ref):
    """{key: [names]} of the keys more than one bucket has."""
    by = {}
    for nm, d in ref.items():
        by.setdefault(d, []).append(nm)
    return {d: v for d, v in by.items() if len(v) > 1}


# ---------------------------------------------------------------- the edges ----
TINY = 1 << 52                        # bits of 2^-1022, the smallest normal
NAN = 0x7FF8000000000000


def edge_table(s):
    """-> (names, base bits, taken bits): the fixed edge cases and the digit
    family of shift s (taken bits BASE + (i << s) over a +0.0 baseline)."""
    cases = [
        # subtractions that round
        (b"round-a", f2b(1.0), f2b(2.0 ** 53 + 2)),       # 2^53 + 1: a tie, to even
        (b"round-b", f2b(1.0), f2b(2.0 ** 53 + 6)),       # 2^53 + 5: a tie, down to 2^53 + 4
        (b"round-c", f2b(0.1), f2b(0.3)),
        (b"round-d", f2b(1.0 / 3.0), f2b(1e10 + 0.7)),
        # taken = base * (1 + 2^-52): the difference is one ulp of base
        (b"ulp-1", f2b(1.0), f2b(1.0) + 1),
        (b"ulp-2", f2b(1e6), f2b(1e6) + 1),
        (b"ulp-3", f2b(1e-300), f2b(1e-300) + 1),
        (b"ulp-4", f2b(1.5e300), f2b(1.5e300) + 1),
        # a denormal difference, key bits 1
        (b"denormal", TINY, TINY + 1),
        (b"inf-finite", f2b(5.0), INF),
        # never rank
        (b"never-inf-inf", INF, INF),
        (b"never-nan", f2b(5.0), NAN),
        (b"never-equal", f2b(42.0), f2b(42.0)),
        (b"never-zero", 0, 0),
        (b"never-negzero", SIGN, SIGN),
        # base = -0.0
        (b"negzero-base", SIGN, f2b(3.0)),
    ]
    cases += [(b"fam-%d" % i, 0, TP.BASE + (i << s)) for i in range(1, 9)]
    names = [c[0] for c in cases]
    return names, [c[1] for c in cases], [c[2] for c in cases]


def edge_rows(names, bits):
    return {nm: (f2b(5.0), b, 1, T0) for nm, b in zip(names, bits)}


def edge_cols(bits):
    n = len(bits)
    return [np.full(n, f2b(5.0), np.uint64), np.array(bits, np.uint64), np.full(n, 1, np.int64),
            np.full(n, T0, np.int64)]


def edge_expected(s):
    """-> [(name, key)] in list order; distinct keys except where stated."""
    names, base, taken = edge_table(s)
    ref = reference(edge_rows(names, base), edge_rows(names, taken))
    return sorted(ref.items(), key=lambda kv: -kv[1])
