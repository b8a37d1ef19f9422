"""The coalesced egress of a batch (include/patrolhip.h "Coalesced egress") as
plain Python over the oracle's results, shared by tests/test_egress_abi.py
(no GPU) and tests/test_egress.py.

An op stream is gen_ops' dict (names, kind, now, freq, per, count, added,
taken, elapsed); `ref` is oracle.Repo.apply_mixed's result for it and `dump`
the oracle's dump() taken afterwards.
"""
from __future__ import annotations

import struct

import numpy as np

from tests import _gen
from tests._group_ops import gen_ops, name_pool  # noqa: F401  (re-exported)

TAKE, RECEIVE, UPSERT = 0, 1, 2
CREATED = 0x80
MAX_NAME = 231
FIXED = 25


def bits_to_f(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


def is_zero(a, t, e):
    """Bucket.IsZero (bucket.go:165-170) over float bits: -0.0 == 0."""
    return bits_to_f(a) == 0 and bits_to_f(t) == 0 and int(e) == 0


def marshal(name, a, t, e):
    """MarshalBinary (bucket.go:51-68)."""
    return struct.pack(">QQq", int(a), int(t), int(e)) + bytes([len(name)]) + name


def request(name):
    """ReplicatedRepo.GetBucket's incast request (repo.go:96-106)."""
    return marshal(name, 0, 0, 0)


def call(o, ops):
    return o.apply_mixed(ops["kind"], ops["names"], ops["now"], ops["freq"], ops["per"],
                         ops["count"], ops["added"], ops["taken"], ops["elapsed"])


def expected(ops, ref, dump):
    """-> (incast_names, {name: (added, taken, elapsed)}): the buckets whose
    first op in the batch is a TAKE that created them, and the final state of
    every bucket a TAKE or UPSERT op named, zero states and names over 231
    bytes left out."""
    first = {}
    wants = set()
    for i, nm in enumerate(ops["names"]):
        first.setdefault(nm, i)
        if ops["kind"][i] in (TAKE, UPSERT):
            wants.add(nm)
    incast = [nm for nm, i in first.items()
              if ops["kind"][i] == TAKE and (int(ref["status"][i]) & CREATED)
              and len(nm) <= MAX_NAME]
    states = {}
    for nm in wants:
        a, t, e = dump[nm][:3]
        if len(nm) <= MAX_NAME and not is_zero(a, t, e):
            states[nm] = (a, t, e)
    return incast, states


def expected_datagrams(ops, ref, dump):
    """expected() as (request datagrams by name, state datagrams by name)."""
    incast, states = expected(ops, ref, dump)
    return ({nm: request(nm) for nm in incast},
            {nm: marshal(nm, *s) for nm, s in states.items()})


def per_op_broadcasts(ops, ref):
    """The reference's datagram sequence: UpsertBucket's broadcast of reply[i]
    for every TAKE and UPSERT op in order (api.go:67-74, repo.go:123-158), each
    creating TAKE's incast request in front of it (repo.go:96-106)."""
    out = []
    for i, nm in enumerate(ops["names"]):
        k = ops["kind"][i]
        if k not in (TAKE, UPSERT):
            continue
        if k == TAKE and (int(ref["status"][i]) & CREATED):
            out.append(request(nm))
        out.append(marshal(nm, ref["reply_added"][i], ref["reply_taken"][i],
                           ref["reply_elapsed"][i]))
    return out


def parse(data, offs, n):
    """Back-to-back datagrams -> [(name, added, taken, elapsed, raw bytes)]
    (UnmarshalBinary, bucket.go:71-91)."""
    raw = bytes(np.asarray(data, np.uint8)[:int(offs[n])]) if n else b""
    out = []
    for i in range(n):
        d = raw[int(offs[i]):int(offs[i + 1])]
        assert len(d) >= FIXED, (i, len(d))
        a, t, e = struct.unpack(">QQq", d[:24])
        assert len(d) == FIXED + d[24], (i, len(d), d[24])
        out.append((d[FIXED:], a, t, e, d))
    return out


def sections(eg):
    """An egress dict (data, offs, n, n_incast) -> (requests by name, states by
    name), asserting the layout: offsets monotone from 0, no name twice in a
    section, requests all-zero."""
    offs = np.asarray(eg["offs"], np.uint64)
    n, ni = eg["n"], eg["n_incast"]
    assert len(offs) >= n + 1 and int(offs[0]) == 0
    assert np.all(offs[1:n + 1] >= offs[:n])
    recs = parse(eg["data"], offs, n)
    req, st = {}, {}
    for nm, a, t, e, d in recs[:ni]:
        assert (a, t, e) == (0, 0, 0) and nm not in req, nm
        req[nm] = d
    for nm, a, t, e, d in recs[ni:]:
        assert nm not in st, nm
        st[nm] = d
    return req, st


def monotone_takes(rng, n, nbuckets, t0=_gen.T0):
    """TAKE-only ops, Zipf(1.1) over b"b%d" names, one rate per bucket chosen
    from the bucket's index, a non-decreasing clock: the reference's post-op
    states of a bucket are then field-wise non-decreasing."""
    ids = _gen.zipf_ids(rng, n, nbuckets)
    names = [b"b%d" % int(i) for i in ids]
    z = np.zeros(n, np.uint64)
    return dict(names=names, kind=np.zeros(n, np.uint8),
                now=t0 + np.cumsum(rng.integers(0, 20_000_000, n)).astype(np.int64),
                freq=np.where(ids % 2 == 0, 100, 5).astype(np.int64),
                per=np.full(n, _gen.SEC, np.int64),
                count=rng.integers(1, 4, n).astype(np.uint64),
                added=z, taken=z.copy(), elapsed=np.zeros(n, np.int64))


def assert_monotone(ops, ref):
    """Each bucket's post-op states, from the oracle's replies alone, never
    decrease in any field (as floats for added / taken)."""
    last = {}
    for i, nm in enumerate(ops["names"]):
        cur = (bits_to_f(ref["reply_added"][i]), bits_to_f(ref["reply_taken"][i]),
               int(ref["reply_elapsed"][i]))
        if nm in last:
            assert all(c >= p for c, p in zip(cur, last[nm])), (i, nm, last[nm], cur)
        last[nm] = cur
