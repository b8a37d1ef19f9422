"""The throttled sweep's model (include/patrolhip.h "Throttled sweep"), shared
by tests/test_throttled_abi.py (CPU) and tests/test_throttled.py (GPU).

Match rule, restated.  A rule is (prefix, freq, per, count); rule r matches a
name iff len(name) >= len(prefix) and name starts with prefix; the first rule
that matches, in list order, gives the bucket's query; no match: not reported.

expected().  From the rows of a dump, {name: (added bits, taken bits, elapsed,
created)}, the entries a whole sweep reports: every name of at most 231 bytes
that a rule matches and whose Take -- tests/_peek_cases.py's reference, the
oracle's pure Take on a copy of the state -- is denied at `now` and also at
now + min_wait (saturating).  Nothing here calls the library.

The table recipe.  600 names whose heads cycle through the four rule prefixes,
two heads shorter than their prefix, one no rule knows, the empty head and one
that differs from rule 0's prefix in its last byte (and so falls to rule 1);
each is filled with lower-case letters, or cut, to a length that cycles over
0-14, 15-22, 23-40 and 200-231 bytes (the empty name comes out once).  Every
third state is _peek_cases.extreme_state, the rest plain_state at the matching
rule's rate (any plain rate when no rule matches).
"""
from __future__ import annotations

import random

import numpy as np

from tests import _peek_cases as PC

T0, SEC = PC.T0, PC.SEC
I64_MAX = PC.I64_MAX
NEVER = PC.NEVER
MAX_NAME = 231
TILE = 4096   # PHIP_SWEEP_TILE

RULES = [(b"org:acme:0123456", 3, SEC, 2), (b"org:", 30, 60 * SEC, 5), (b"u:", 100, SEC, 1),
         (b"ip:", 3, SEC, 1)]
HEADS = [r[0] for r in RULES] + [b"u", b"or", b"x:", b"", b"org:acme:012345_"]
CLASSES = [(0, 14), (15, 22), (23, 40), (200, 231)]
NOW = T0 + 20 * SEC
NOW_EARLY = T0 - 100 * SEC
MIN_WAIT = 20 * SEC


def match(rules, name):
    """Index of the first rule whose prefix `name` starts with, or -1."""
    for i, r in enumerate(rules):
        p = r[0]
        if len(name) >= len(p) and name[:len(p)] == p:
            return i
    return -1


def window(max_entries):
    """W: the slots one call reads at most."""
    w = max(4 * max_entries, TILE)
    return (w + TILE - 1) // TILE * TILE


def make_names(rng, n, heads=HEADS, classes=CLASSES):
    """n distinct names: heads and length classes in turn (their periods, 9
    and 4, are coprime, so every head meets every class)."""
    out, seen = [], set()
    for draw in range(200 * n):
        if len(out) == n:
            break
        head = heads[draw % len(heads)]
        lo, hi = classes[draw % len(classes)]
        L = rng.randrange(lo, hi + 1)
        nm = (head + bytes(rng.randrange(97, 123) for _ in range(max(L - len(head), 0))))[:L]
        if nm not in seen:
            seen.add(nm)
            out.append(nm)
    assert len(out) == n
    return out


def table_case(seed=7, n=600, rules=RULES, **kw):
    """-> dict(names, cols (a, t, e, c numpy columns), rows {name: state})."""
    names = make_names(random.Random(seed), n, **kw)
    rng = random.Random(11 * seed)   # (the states' own stream: see check_mix)
    states = []
    for k, nm in enumerate(names):
        r = match(rules, nm)
        if k % 3 == 0:
            states.append(PC.extreme_state(rng))
        else:
            states.append(PC.plain_state(rng, rules[r][1:3] if r >= 0 else None)[0])
    cols = [np.array([s[j] for s in states], np.uint64 if j < 2 else np.int64) for j in range(4)]
    return dict(names=names, cols=cols, rows=dict(zip(names, states)))


def later_of(now, min_wait):
    return min(now + min_wait, I64_MAX)


def expected(dump, rules, now, min_wait=0):
    """-> {name: dict(rule, remaining, klass ("finite" / "never"), ref)} of the
    buckets a whole sweep reports, and the tally of everything else."""
    out = {}
    tally = dict(unmatched=0, granted=0, held_out=0, too_long=0)
    for name, state in dump.items():
        if len(name) > MAX_NAME:
            tally["too_long"] += 1
            continue
        r = match(rules, name)
        if r < 0:
            tally["unmatched"] += 1
            continue
        _, freq, per, count = rules[r]
        ref = PC.reference(state, now, freq, per, count)
        if ref["klass"] == "ok":
            tally["granted"] += 1
            continue
        if min_wait > 0 and PC.ok_at(ref["s"], later_of(now, min_wait), freq, per, count):
            tally["held_out"] += 1
            continue
        out[name] = dict(rule=r, remaining=ref["remaining"], klass=ref["klass"], ref=ref)
    return out, tally


def check_mix(dump, rules, now, min_wait=MIN_WAIT):
    """The conditions on a table's mix at `now`, from the reference alone: at
    least 10% of the buckets unmatched, 20% granted, 8% denied with a finite
    answer, 3% never, 5 throttled under every rule, and 10 that `min_wait`
    holds out.  -> the tally.

    Measured for table_case(7) (names from seed 7, states from their own
    stream 77, the first of a handful tried that meets every condition at both
    readings), 600 buckets: 285 unmatched at either reading; at NOW 213
    granted, 65 finite, 37 never, [7, 76, 10, 9] per rule, 11 held out; at
    NOW_EARLY 136 granted, 142 finite, 37 never, [33, 88, 27, 31], 11 held
    out."""
    exp, tally = expected(dump, rules, now, 0)
    held = expected(dump, rules, now, min_wait)[1]["held_out"]
    n = len(dump)
    finite = sum(e["klass"] == "finite" for e in exp.values())
    never = sum(e["klass"] == "never" for e in exp.values())
    per_rule = [sum(e["rule"] == i for e in exp.values()) for i in range(len(rules))]
    tally = dict(tally, finite=finite, never=never, per_rule=per_rule, held_out=held)
    assert tally["unmatched"] >= 0.10 * n, (tally, n)
    assert tally["granted"] >= 0.20 * n, (tally, n)
    assert finite >= 0.08 * n and never >= 0.03 * n, (tally, n)
    assert min(per_rule) >= 5, tally
    assert held >= 10, tally
    return tally


def check_entry(exp, rules, now, name, rule, remaining, retry_at):
    """One reported entry against the model: the rule, remaining bit-equal,
    retry_at by its definition (tests/_peek_cases.check_retry)."""
    e = exp[name]
    assert (int(rule), int(remaining)) == (e["rule"], e["remaining"]), (name, rule, remaining, e)
    _, freq, per, count = rules[e["rule"]]
    PC.check_retry(e["ref"], (None, now, freq, per, count), int(retry_at))
