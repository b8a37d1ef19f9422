"""The export sweep's model (patrolhip.h "Anti-entropy sweep"), shared by
tests/test_export_sweep_abi.py (which checks it against the oracle alone) and
tests/test_export_sweep.py (which holds the GPU to it).

From the rows of a dump, {name: (added bits, taken bits, elapsed, created)},
the datagrams a whole sweep writes: every bucket's MarshalBinary
(bucket.go:51-68, oracle.go_semantics.Bucket.marshal), except
  - zero states (Bucket.IsZero, bucket.go:165-170: -0.0 counts as zero): their
    datagram would be an incast request (repo.go:78,86-90);
  - with idle_ns > 0, the buckets the eviction rule calls idle at `now`
    (tests/_evict_cases.py: idle = now - (created + elapsed), exact, 0 when
    negative, saturating at INT64_MAX; idle >= idle_ns);
  - names MarshalBinary refuses (longer than 231 bytes, bucket.go:48).
"""
import struct

from oracle import go_semantics as G
from tests import _evict_cases as EC

I64MAX, I64MIN = 2**63 - 1, -2**63
SIGN = 1 << 63
MAX_NAME = 231
FIXED = 25
TILE = 4096   # PHIP_SWEEP_TILE


def is_zero(a_bits, t_bits, elapsed):
    return (a_bits & ~SIGN) == 0 and (t_bits & ~SIGN) == 0 and elapsed == 0


def idle_of(created, elapsed, now):
    d = now - (created + elapsed)
    return 0 if d < 0 else min(d, I64MAX)


def marshal(name, a_bits, t_bits, elapsed):
    dg = G.Bucket(name, G.b2f(a_bits), G.b2f(t_bits), elapsed).marshal()
    # (the float round trip keeps every bit, NaN payloads included)
    assert dg == struct.pack(">QQq", a_bits, t_bits, elapsed) + bytes([len(name)]) + name
    return dg


def exported(rows, now=0, idle_ns=0):
    """-> {name: datagram} of the buckets a sweep of `rows` writes."""
    out = {}
    for name, (a, t, e, c) in rows.items():
        if len(name) > MAX_NAME or is_zero(a, t, e):
            continue
        if idle_ns > 0 and idle_of(c, e, now) >= idle_ns:
            continue
        out[name] = marshal(name, a, t, e)
    return out


def window(max_msgs):
    """W: the slots one call reads at most."""
    w = max(4 * max_msgs, TILE)
    return (w + TILE - 1) // TILE * TILE


A1, T1 = G.f2b(10.0), G.f2b(3.0)
NOW = EC.NOW
SEC = EC.SEC

# One window over more than 512 tiles: the tile scan walks the tile arrays in
# chunks of 512 entries and carries the running totals from chunk to chunk, so
# only such a window has a tile whose base comes out of the carry.
# 4 * CHUNK_MSGS slots are 513 tiles.
CHUNK_TILES = 512
CHUNK_MSGS = (CHUNK_TILES + 1) * TILE // 4
CHUNK_LOG2_SLOTS = 22
CHUNK_CAP = 1 << 21      # bytes: more than every datagram of chunk_rows() together
CHUNK_RULE = [(b"", 3, SEC, 1)]   # the throttled sweep's catch-all: denies the drained half at NOW


def chunk_rows(count=6000):
    """A few thousand buckets for a table of 2^22 slots (about six a tile):
    the empty name once, inline names and arena names in turn; every other
    state has no token left under CHUNK_RULE, the others all three."""
    rows = {b"": (G.f2b(3.0), G.f2b(3.0), 0, NOW)}
    for k in range(1, count):
        L = (5, 14, 15, 22, 23, 40, 231)[k % 7]
        taken = G.f2b(3.0) if k % 2 else 0
        rows[(b"%05d" % k).ljust(L, b"n")] = (G.f2b(3.0), taken, k, NOW)
    return rows


def chunk_repo(pa, zeros=64, **kw):
    """chunk_rows() seeded into 2^22 slots, and zero states beside them (left
    by zero-state Receives: a sweep skips them)."""
    repo = pa.GPURepo(log2_slots=CHUNK_LOG2_SLOTS, arena_bytes=1 << 20, **kw)
    rows = chunk_rows()
    ks = list(rows)
    repo.seed(ks, *[[rows[k][j] for k in ks] for j in range(4)])
    zn = [b"zero-state-%d" % k for k in range(zeros)]
    out = repo.receive_soa(zn, [0] * zeros, [0] * zeros, [0] * zeros, NOW + 1)
    assert (out["status"] & 0x80).all()
    assert repo.capacity == 1 << CHUNK_LOG2_SLOTS and len(repo) == len(rows) + zeros
    return repo


def filter_rows():
    """{name: (added bits, taken bits, elapsed, created)} around NOW: the
    eviction tests' buckets (idle for exactly per, per + 1, 10 per under every
    rate), and the rule's edges: now < last, now == last, created + elapsed
    past either end of int64, a negative elapsed."""
    rows = {}
    for ri, rate in enumerate(EC.RATES):
        for nm, a, t, e, c in EC.buckets(rate):
            if a == 0.0 and t == 0.0 and e == 0:
                a = 1.0   # (a zero state is skipped whatever its age: keep the row a filter case)
            rows[b"r%d-" % ri + nm] = (G.f2b(a), G.f2b(t), e, c)
    edges = [(NOW, 1000), (NOW - 10, 10), (NOW - 11, 10), (NOW - SEC, 0), (NOW - SEC + 1, 0),
             (I64MAX, I64MAX), (I64MIN, I64MIN), (I64MIN, -1), (I64MIN, 0), (I64MAX, 1),
             (NOW + 50, -50), (NOW + 50, -51), (0, NOW), (0, NOW - 10 * SEC)]
    for k, (c, e) in enumerate(edges):
        rows[b"edge-%d" % k] = (A1, T1, e, c)
    return rows


IDLE_NS = [1, 10, 11, SEC, SEC + 1, 60 * SEC, 600 * SEC, I64MAX]
