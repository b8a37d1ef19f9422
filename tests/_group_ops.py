"""Shared by the tests of the owner-routed op path (phip_route_pack_ops,
phip_group_apply_mixed): the order rule as plain Python, an op generator over
a fixed name pool, and the oracle's results mapped back to (member, index).

Order rule (include/patrolhip.h): the call runs rounds of `chunk` ops of
every member's batch; in a round an owner applies sources in rank order, each
source's ops in index order.  A bucket's ops therefore take effect in
(round, source rank, index) order, and since buckets are independent the
whole call equals one ordered pass over all ops sorted by that key.
"""
from __future__ import annotations

import numpy as np

from tests import _gen

CHUNK = 1 << 24
SMALL_CHUNK = 1 << 12
COLS = ("kind", "now", "freq", "per", "count", "added", "taken", "elapsed")
DTYPES = dict(kind=np.uint8, now=np.int64, freq=np.int64, per=np.int64, count=np.uint64,
              added=np.uint64, taken=np.uint64, elapsed=np.int64)


def apply_order(sizes, chunk=CHUNK):
    """[(member, index)] of every op of batches of the given sizes, in the
    order the group applies them: (round = index // chunk, member, index)."""
    keys = [(j // chunk, i, j) for i, n in enumerate(sizes) for j in range(n)]
    keys.sort()
    return [(i, j) for _, i, j in keys]


def rank_order(sizes):
    """The order a group WITHOUT rounds would give: (member, index)."""
    return [(i, j) for i, n in enumerate(sizes) for j in range(n)]


def name_pool(nbuckets):
    """The empty name, 1-byte names, the inline/arena boundary (22 and 23
    bytes), a 231-byte name, and b"b%d" ids."""
    pool = [b"", b"a", b"Z", b"\x00", b"n" * 22, b"twenty-two-bytes".ljust(22, b"."),
            b"N" * 23, b"twenty-three-bytes".ljust(23, b"."), b"L" * 231, bytes(range(1, 232))]
    pool += [b"b%d" % i for i in range(max(0, nbuckets - len(pool)))]
    return pool[:max(nbuckets, 1)]


def gen_ops(rng, n, pool, t0=_gen.T0, all_take=False):
    """n ops over `pool` as host arrays: ~60% TAKE (100:1s and 5:1s, counts 1-3:
    some are denied), ~30% RECEIVE (a few all-zero incasts), ~10% UPSERT; `now`
    non-decreasing.  -> dict(names=list[bytes], kind, now, freq, per, count,
    added, taken, elapsed)."""
    ids = _gen.zipf_ids(rng, n, len(pool)) if n else np.zeros(0, np.int64)
    names = [pool[int(i)] for i in ids]
    u = rng.random(n)
    kind = np.where(u < 0.6, 0, np.where(u < 0.9, 1, 2)).astype(np.uint8)
    if all_take:
        kind[:] = 0
    now = t0 + np.cumsum(rng.integers(0, 20_000_000, n)).astype(np.int64)
    fast = rng.random(n) < 0.5
    freq = np.where(fast, 100, 5).astype(np.int64)
    per = np.full(n, _gen.SEC, np.int64)
    count = rng.integers(1, 4, n).astype(np.uint64)
    a, t, e = _gen.clean_states(rng, n)
    z = (kind == 1) & (rng.random(n) < 0.1)   # incast requests
    a[z], t[z], e[z] = 0, 0, 0
    return dict(names=names, kind=kind, now=now, freq=freq, per=per, count=count, added=a,
                taken=t, elapsed=e)


def sorted_ops(batches, order):
    """The batches' ops gathered in `order` as one stream (oracle arguments)."""
    out = dict(names=[batches[i]["names"][j] for i, j in order])
    for c in COLS:
        out[c] = np.array([batches[i][c][j] for i, j in order], DTYPES[c])
    return out


def oracle_results(o, batches, order):
    """Run the oracle once over all ops in `order` and map its results back:
    -> one dict per member of status, remaining, have, reply (int64 [n, 4]:
    added, taken, elapsed, created bits), entry j for op j of that member."""
    s = sorted_ops(batches, order)
    ref = o.apply_mixed(s["kind"], s["names"], s["now"], s["freq"], s["per"], s["count"],
                        s["added"], s["taken"], s["elapsed"])
    per = []
    for b in batches:
        n = len(b["names"])
        per.append(dict(status=np.zeros(n, np.uint8), remaining=np.zeros(n, np.uint64),
                        have=np.zeros(n, np.uint64), reply=np.zeros((n, 4), np.int64)))
    rep = np.stack([ref["reply_added"].view(np.int64), ref["reply_taken"].view(np.int64),
                    ref["reply_elapsed"], ref["reply_created"]], axis=1) if order else None
    for k, (i, j) in enumerate(order):
        per[i]["status"][j] = ref["status"][k]
        per[i]["remaining"][j] = ref["remaining"][k]
        per[i]["have"][j] = ref["have"][k]
        per[i]["reply"][j] = rep[k]
    return per


_HASH = {}


def owners(names, world):
    """The owner rank of each name in a group of `world` members
    (patrol_amd.shard.owner_of over the names' FNV-1a hashes)."""
    import torch
    from oracle import go_semantics as G
    from patrol_amd import shard
    for nm in names:
        if nm not in _HASH:
            _HASH[nm] = G.fnv1a64(nm)
    if not len(names):
        return np.zeros(0, np.int64)
    h = np.array([_HASH[nm] for nm in names], np.uint64).view(np.int64)
    return shard.owner_of(torch.from_numpy(h), world).numpy().astype(np.int64)


def reply_mask(kind, status):
    """Ops whose reply state is defined (patrolhip.h phip_results.reply): TAKE,
    UPSERT and incast RECEIVEs; a merged replica's entry is all zeros."""
    st = status & 0x7F
    return (kind == 0) | (kind == 2) | (st == 2) | (st == 3)
