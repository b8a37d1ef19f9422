"""Incast reply egress (include/patrolhip.h "Incast reply egress"): the model
and the case builders of tests/test_replies.py and tests/test_replies_abi.py.

The model turns the oracle's Receive columns (status, reply a / t / e) and the
batch's names into the datagrams a *_replies call must hand back, with
patrol_amd.marshal (MarshalBinary, bucket.go:51-68): one per message whose
status is INCAST_REPLY, in batch order, cut at max_msgs / a byte budget.
Each builder's case is checked on the CPU, from the oracle alone, for what it
is meant to hold (check_case)."""
import struct

import numpy as np

import patrol_amd as pa
from tests import _gen

SEC = 10**9
NEG0 = np.uint64(0x8000000000000000)
REPLY, NOREPLY, CREATED = 2, 3, 0x80
INLINE = 22          # names longer than this live in the arena
NOW = _gen.T0 + 5 * SEC


def expected(names, st, ra, rt, re, max_msgs=None, budget=None):
    """-> dict(data bytes, offs uint64[n+1], src uint32[n], n, replies, skipped, bytes) for the
    messages the columns cover (a stopped batch: the columns before the stop)."""
    data, offs, src = [], [0], []
    replies = skipped = 0
    cut = False
    for i in np.nonzero((np.asarray(st) & 0x7F) == REPLY)[0]:
        i = int(i)
        replies += 1
        if len(names[i]) > 231:          # MarshalBinary refuses it (bucket.go:48)
            skipped += 1
            continue
        d = pa.marshal(names[i], pa.BucketState(int(ra[i]), int(rt[i]), int(re[i]), 0))
        cut = cut or (max_msgs is not None and len(src) >= max_msgs) or \
            (budget is not None and offs[-1] + len(d) > budget)
        if cut:
            continue
        data.append(d)
        offs.append(offs[-1] + len(d))
        src.append(i)
    return dict(data=b"".join(data), offs=np.array(offs, np.uint64), src=np.array(src, np.uint32),
                n=len(src), replies=replies, skipped=skipped, bytes=offs[-1])


def datagrams_of(e):
    """The model's datagrams as a list of bytes."""
    o = e["offs"]
    return [e["data"][int(o[k]):int(o[k + 1])] for k in range(e["n"])]


def wire(names, a, t, e):
    """The batch as datagrams (a name's length byte as UnmarshalBinary reads it)."""
    return [struct.pack(">QQQ", int(a[i]), int(t[i]), int(e[i]) & (2**64 - 1)) +
            bytes([len(names[i])]) + names[i] for i in range(len(names))]


def long_name(k):
    return b"a-bucket-name-of-the-arena-kind-%04d" % k


def make_case(seed, n, K=2000, replies=60, absent=6, zero=6, negzero=4, twice=6, long=0):
    """A seeded table and a batch of n Zipf messages over its K short-named
    buckets b0.. (names of at most 14 bytes), with requests at random places:
    `replies` to existing buckets, `absent` to names the table lacks, `zero` to
    existing buckets whose state is zero, `negzero` made of -0.0 fields, `twice`
    buckets asked twice with a raising merge in between, `long` to buckets with
    arena names.  -> dict(seed=(names, a, t, e, created), names, a, t, e, tags)
    where tags maps a kind to the batch positions of its requests."""
    rng = np.random.default_rng(seed)
    s_names = _gen.key_names(np.arange(K))
    sa, st, se = _gen.clean_states(rng, K)
    zero_names = [b"z%d" % k for k in range(zero)]
    long_names = [long_name(k) for k in range(long)]
    la, lt, le = _gen.clean_states(rng, max(long, 1))
    s_names = s_names + zero_names + long_names
    sa = np.concatenate([sa, np.zeros(zero, np.uint64), la[:long]])
    st = np.concatenate([st, np.zeros(zero, np.uint64), lt[:long]])
    se = np.concatenate([se, np.zeros(zero, np.int64), le[:long]])
    created = _gen.T0 - rng.integers(0, SEC, len(s_names))
    names = _gen.key_names(_gen.zipf_ids(rng, n, K))
    a, t, e = _gen.clean_states(rng, n)
    total = replies + absent + zero + negzero + 3 * twice + long
    pos = [int(p) for p in rng.choice(n, total, replace=False)]
    tags = {}

    def ask(kind, p, name, av=0, tv=0):
        names[p] = name
        a[p], t[p], e[p] = av, tv, 0
        tags.setdefault(kind, []).append(p)

    for _ in range(replies):
        ask("reply", pos.pop(), b"b%d" % int(rng.integers(0, K)))
    for k in range(absent):
        ask("absent", pos.pop(), b"n%d" % k)
    for k in range(zero):
        ask("zero", pos.pop(), zero_names[k])
    for k in range(negzero):
        ask("negzero", pos.pop(), b"b%d" % int(rng.integers(0, K)), NEG0, NEG0 if k % 2 else 0)
    for k in range(twice):
        p1, p2, p3 = sorted(pos.pop() for _ in range(3))
        nm = b"b%d" % int(rng.integers(0, K))
        ask("twice", p1, nm)
        names[p2] = nm                                    # a merge that raises every field
        a[p2] = np.float64(3e6 + k).view(np.uint64)
        t[p2] = np.float64(2e6 + k).view(np.uint64)
        e[p2] = (1 << 41) + k
        ask("twice", p3, nm)
    for k in range(long):
        ask("long", pos.pop(), long_names[k])
    return dict(seed=(s_names, sa, st, se, created), names=names, a=a, t=t, e=e, tags=tags)


def check_case(c, st, ra, rt, re, *, replies=0, absent=0, zero=0, negzero=0, twice=0, long=0):
    """What the case is for, from the oracle's columns alone."""
    st7 = np.asarray(st) & 0x7F
    tags = c["tags"]
    assert int((st7 == REPLY).sum()) >= replies
    got = [p for p in tags.get("absent", []) if st[p] == NOREPLY | CREATED]
    assert len(got) >= absent, len(got)
    got = [p for p in tags.get("zero", []) if st[p] == NOREPLY]
    assert len(got) >= zero, len(got)
    got = [p for p in tags.get("negzero", []) if st7[p] in (REPLY, NOREPLY)]
    assert len(got) >= negzero, len(got)
    tw = tags.get("twice", [])
    differ = 0
    for p1, p3 in zip(tw[0::2], tw[1::2]):
        assert c["names"][p1] == c["names"][p3] and p1 < p3
        if st7[p1] == REPLY and st7[p3] == REPLY and \
                (ra[p1], rt[p1], re[p1]) != (ra[p3], rt[p3], re[p3]):
            differ += 1
    assert differ >= twice, differ
    got = [p for p in tags.get("long", []) if st7[p] == REPLY and len(c["names"][p]) > INLINE]
    assert len(got) >= long, len(got)


def dirty_mask(a, t, e):
    """The messages whose place in the batch matters: requests and -0.0 fields."""
    return ((a == 0) & (t == 0) & (e == 0)) | (a == NEG0) | (t == NEG0)


SUFFIX_TILE = 256        # messages per tile of the ordered suffix's reply egress (kBlock)
CHUNK_TILES = 512        # tiles per chunk of k_reply_scan's walk


def chunk_case(seed=15, K=8, requests=48):
    """512 * 256 + 1 messages over K buckets with arena names, the first a
    request (a dirty name over 14 bytes: the whole batch is the ordered
    suffix), `requests` more at random places and one as the last message,
    alone in tile 512 -- the tile whose bases come through the carry of the
    scan's second chunk.  -> make_case's dict, tags["reply"] the requests."""
    rng = np.random.default_rng(seed)
    n = CHUNK_TILES * SUFFIX_TILE + 1
    s_names = [long_name(k) for k in range(K)]
    sa, st, se = _gen.clean_states(rng, K)
    created = _gen.T0 - rng.integers(0, SEC, K)
    names = [s_names[int(i)] for i in rng.integers(0, K, n)]
    a, t, e = _gen.clean_states(rng, n)
    pos = sorted({0, n - 1} | {int(p) for p in rng.choice(n, requests, replace=False)})
    for p in pos:
        a[p], t[p], e[p] = 0, 0, 0
    return dict(seed=(s_names, sa, st, se, created), names=names, a=a, t=t, e=e,
                tags={"reply": pos})
