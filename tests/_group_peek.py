"""Shared by the tests of the owner-routed peek (phip_group_peek):
tests/test_group_peek_abi.py (CPU) and tests/test_group_peek.py (GPU).

A table_case (tests/_peek_cases.py) is seeded into a shard group bucket by
bucket: each goes to the member that owns its name (tests/_group_ops.owners)
and into one oracle.  Member i's queries are table_queries(100 * world + i,
tab, n).  The expected answers are PC.reference over the oracle's state, so a
query answered on the wrong shard shows as a wrong PHIP_ST_ABSENT bit (about
85% of the queries name a present bucket); retry_at is checked by its
definition (PC.check_retry), never by a formula.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import _group_ops as GO
from tests import _peek_cases as PC

TABLE_SEED, TABLE_BUCKETS = 31, 600
# (world, member sizes) of the shared-device cases and of the small rounds
SHARED_CASES = [(2, (2700, 0)), (3, (2000, 0, 3000))]
ROUNDS_CASE = (2, (9000, 5000))
MIN_PAIR = 400   # queries every (source, owner) pair of a non-empty member holds
COLUMNS = ("status", "remaining", "have", "retry_at", "state")


def table():
    return PC.table_case(TABLE_SEED, TABLE_BUCKETS)


def seeded_oracle(tab):
    o = O.Repo()
    o.seed(tab["names"], *tab["cols"])
    return o


def seed_group(g, tab, world):
    """Every bucket of tab into the member that owns its name -> buckets per member."""
    own = GO.owners(tab["names"], world)
    per = []
    for r in range(world):
        idx = np.nonzero(own == r)[0]
        g.repos[r].seed([tab["names"][k] for k in idx], *[c[idx] for c in tab["cols"]])
        per.append(len(idx))
    return per


def member_queries(tab, world, sizes):
    return [PC.table_queries(100 * world + i, tab, n) for i, n in enumerate(sizes)]


def references(get, queries):
    """PC.reference of every query over the state get(name) returns (None: absent)."""
    return [PC.reference(get(q[0]), *q[1:]) for q in queries]


def device_batch(queries, dev, slack=64):
    """Queries as the dict of CUDA tensors GPUGroup.peek takes (an empty batch
    keeps one-entry columns)."""
    import torch
    names, now, freq, per, count = PC.columns(queries)
    offs = np.zeros(len(names) + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in names])
    blob = np.zeros(int(offs[-1]) + slack, np.uint8)
    blob[:offs[-1]] = np.frombuffer(b"".join(names), np.uint8)
    cols = dict(names=blob, name_offs=offs, now=now, freq=freq, per=per, count=count.view(np.int64))
    return {k: torch.from_numpy(v if v.size else np.zeros(1, v.dtype)).to(dev)
            for k, v in cols.items()}


def host_results(out, n):
    """One member's result dict (CUDA tensors) as host arrays of n entries."""
    r = {k: out[k].cpu().numpy()[:n] for k in COLUMNS if out.get(k) is not None}
    for k in ("remaining", "have"):
        if k in r:
            r[k] = r[k].view(np.uint64)
    return r


def check_member(res, queries, refs, tag=""):
    """status, remaining, have against the reference bit for bit, retry_at by
    its definition, the state column (when returned) the state evaluated."""
    n = len(queries)
    assert all(len(v) == n for v in res.values()), (tag, n)
    for i, (q, ref) in enumerate(zip(queries, refs)):
        got = (int(res["status"][i]), int(res["remaining"][i]), int(res["have"][i]))
        assert got == (ref["status"], ref["remaining"], ref["have"]), (tag, i, q, got, ref)
        PC.check_retry(ref, (None,) + q[1:], int(res["retry_at"][i]))
        if "state" in res:
            s = res["state"][i]
            got_s = (int(s[0]) & (2**64 - 1), int(s[1]) & (2**64 - 1), int(s[2]), int(s[3]))
            assert got_s == ref["s"], (tag, i, q, got_s, ref["s"])
