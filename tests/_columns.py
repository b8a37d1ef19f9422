"""Poisoned result columns and the op streams that exercise them, shared by
tests/test_columns_cases.py (CPU: the streams against the oracle, the helper
against itself) and tests/test_result_columns.py (GPU).

The contract under test (include/patrolhip.h, "Result columns"): a column the
caller passes is written in all n entries, an entry the column does not apply
to reads zero, and nothing outside the n entries is touched.  Zero is also the
right answer for a large share of entries, so a column handed over as zeros
cannot show a path that never stores a default.  Here every column lies inside
a larger buffer filled with POISON, a byte that is no status and no plausible
result, with GUARD bytes on either side, and starts either aligned or at a
misalignment that keeps the entry's natural alignment and breaks the next one
up (a path that widens its stores shows there).

Every stream carries its own conditions (`shares`): for each column, over the
entries the column applies to, the default and the non-default values each make
up at least MIN_SHARE of the entries and at least MIN_COUNT entries.  They are
computed from the oracle's output alone.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests._gen import SEC, T0

POISON = 0xAB
GUARD = 64
MIN_SHARE, MIN_COUNT = 0.15, 64

TAKE, RECEIVE, UPSERT = 0, 1, 2
ST_MERGED, ST_INCAST_REPLY, ST_INCAST_NOREPLY, ST_SHORT, ST_NOT_PROCESSED = 1, 2, 3, 4, 5
ST_TAKE_OK, ST_TAKE_DENIED, ST_UPSERT_INSERTED, ST_CREATED = 6, 7, 8, 0x80
NEG_ZERO = 0x8000000000000000

# kOutStatus .. kOutReply (phip_kernels.hpp): the bit of each column in a subset mask
COLUMNS = ("status", "remaining", "have", "reply")
BIT = {"status": 1, "remaining": 2, "have": 4, "reply": 8}
REPLY_DT = np.dtype([("a", "<u8"), ("t", "<u8"), ("e", "<i8"), ("c", "<i8")])
DTYPE = {"status": np.dtype(np.uint8), "remaining": np.dtype(np.uint64),
         "have": np.dtype(np.uint64), "reply": REPLY_DT}
# status one byte in; the 8-byte columns not 16-byte aligned; reply not 32-byte aligned
SHIFT = {"status": 1, "remaining": 8, "have": 8, "reply": 8}
BASE_ALIGN = 64

# the thresholds the shapes are built around (test_columns_cases.py compares
# them with phip_kernels.hpp, so a retune fails there first)
SMALL_MAX, LONG_SEG, HUGE_SEG = 1024, 32, 32768


class Column:
    """n entries of one result column inside a poisoned buffer.

    where: "host" (numpy) or "device" (torch, cuda:0).  The buffer's first
    GUARD bytes start at a BASE_ALIGN boundary; the column follows them at
    SHIFT[name] more bytes when misaligned.  ptr: the address handed to the
    library."""

    def __init__(self, name: str, n: int, where: str = "host", misaligned: bool = True):
        self.name, self.n, self.where = name, n, where
        self.dtype = DTYPE[name]
        self.off = GUARD + (SHIFT[name] if misaligned else 0)
        self.nbytes = n * self.dtype.itemsize
        total = self.off + self.nbytes + GUARD
        if where == "device":
            import torch
            self.buf = torch.full((total,), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
            base = self.buf.data_ptr()
        else:
            raw = np.full(total + BASE_ALIGN, POISON, np.uint8)
            skip = -raw.ctypes.data % BASE_ALIGN
            self.buf = raw[skip:skip + total]
            base = self.buf.ctypes.data
        assert base % BASE_ALIGN == 0
        self.ptr = base + self.off
        assert self.ptr % min(self.dtype.itemsize, 8) == 0   # natural alignment kept

    def tensor(self):
        """The column's own bytes as a uint8 tensor view (device columns):
        what a binding that takes caller tensors is handed."""
        assert self.where == "device"
        t = self.buf[self.off:self.off + self.nbytes]
        assert t.data_ptr() == self.ptr
        return t

    def bytes(self) -> np.ndarray:
        """The whole buffer, guards included, as host bytes."""
        if self.where == "device":
            return self.buf.cpu().numpy()
        return self.buf

    def entries(self) -> np.ndarray:
        b = self.bytes()[self.off:self.off + self.nbytes]
        return np.frombuffer(b.tobytes(), self.dtype, self.n)

    def check(self) -> np.ndarray:
        """Asserts both guards are intact; -> the n entries."""
        b = self.bytes()
        lo, hi = b[:self.off], b[self.off + self.nbytes:]
        assert len(hi) == GUARD
        bad = np.nonzero(lo != POISON)[0]
        assert bad.size == 0, "%s: byte %d before the column written" % (self.name, self.off - int(bad[-1]))
        bad = np.nonzero(hi != POISON)[0]
        assert bad.size == 0, "%s: byte %d after the column written" % (self.name, int(bad[0]) + 1)
        return self.entries()


class Results:
    """A phip_results for a subset of the columns (mask: BIT values or-ed),
    NULL for every absent one, each present one a poisoned Column."""

    def __init__(self, n: int, mask: int, where: str = "host", misaligned: bool = True):
        from patrol_amd import _lib
        self.n, self.mask = n, mask
        self.cols = {c: Column(c, n, where, misaligned) for c in COLUMNS if mask & BIT[c]}
        self.struct = _lib.phip_results(*[self.cols[c].ptr if c in self.cols else None
                                          for c in COLUMNS])

    def byref(self):
        return C.byref(self.struct)

    def check(self) -> dict:
        return {c: col.check() for c, col in self.cols.items()}


def first_diff(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


def compare(got: dict, want: dict):
    """Every entry of every passed column, bit for bit."""
    for c, g in got.items():
        w = want[c]
        assert g.dtype == w.dtype and g.shape == w.shape, (c, g.dtype, g.shape)
        d = first_diff(g.view(np.uint8), w.view(np.uint8)) if c != "status" else first_diff(g, w)
        if d is not None:
            i = d[0] // g.dtype.itemsize
            raise AssertionError("%s: entry %d of %d is %r, want %r (%d bytes differ)"
                                 % (c, i, len(g), g[i], w[i], d[1]))


# ------------------------------------------------------------ expectations --
def reply_mask(kind, status):
    """Ops whose reply entry holds a state (patrolhip.h): Takes, Upserts and
    incast requests; a merged replica's reads zero."""
    st = np.asarray(status) & 0x7F
    kind = np.asarray(kind)
    return (kind == TAKE) | (kind == UPSERT) | (st == ST_INCAST_REPLY) | (st == ST_INCAST_NOREPLY)


def expected_mixed(kind, ref) -> dict:
    """What the four columns read after phip_apply_mixed, from the oracle's
    apply_mixed output: remaining / have zero on every op but a TAKE, reply
    zero where no state is owed."""
    kind = np.asarray(kind)
    take = kind == TAKE
    rep = reply_mask(kind, ref["status"])
    reply = np.zeros(len(kind), REPLY_DT)
    for f, k in (("a", "reply_added"), ("t", "reply_taken"), ("e", "reply_elapsed"),
                 ("c", "reply_created")):
        reply[f][rep] = ref[k][rep]
    return dict(status=ref["status"].copy(),
                remaining=np.where(take, ref["remaining"], 0).astype(np.uint64),
                have=np.where(take, ref["have"], 0).astype(np.uint64), reply=reply)


def expected_receive(o, names, added, taken, elapsed, now, stop=None) -> dict:
    """The columns after a Receive batch (applied to the oracle repo `o` here,
    as RECEIVE ops at one clock, which also yields each reply's `created`):
    remaining / have zero throughout; from a stop on (the batch's messages
    before it alone are applied), status SHORT then NOT_PROCESSED and zero in
    every other column."""
    n = len(names)
    stop = n if stop is None else stop
    kind = np.full(stop, RECEIVE, np.uint8)
    z = np.zeros(stop, np.int64)
    ref = o.apply_mixed(kind, list(names[:stop]), np.full(stop, now, np.int64), z, z,
                        z.astype(np.uint64), added[:stop], taken[:stop], elapsed[:stop])
    head = expected_mixed(kind, ref)
    out = {c: np.zeros(n, DTYPE[c]) for c in COLUMNS}
    for c in COLUMNS:
        out[c][:stop] = head[c]
    out["status"][stop:] = ST_NOT_PROCESSED
    if stop < n:
        out["status"][stop] = ST_SHORT
    return out


def is_default(col: str, entries) -> np.ndarray:
    if col == "status":
        return entries == ST_MERGED
    if col == "reply":
        return (entries.view(np.uint8).reshape(len(entries), -1) == 0).all(axis=1)
    return entries == 0


def applies(col: str, kind) -> np.ndarray:
    """The entries a column applies to: remaining / have to Takes, status and
    reply (a row of zeros being the reply of a merged replica) to every op."""
    kind = np.asarray(kind)
    return kind == TAKE if col in ("remaining", "have") else np.ones(len(kind), bool)


def shares(kind, want: dict, where=None) -> dict:
    """col -> (entries it applies to, defaults among them, non-defaults),
    optionally over the ops selected by `where` alone."""
    out = {}
    for c in COLUMNS:
        m = applies(c, kind)
        if where is not None:
            m = m & where
        d = is_default(c, want[c])[m]
        out[c] = (int(m.sum()), int(d.sum()), int((~d).sum()))
    return out


def assert_shares(sh: dict, what: str):
    for c, (n, d, nd) in sh.items():
        for label, k in (("default", d), ("non-default", nd)):
            assert k >= MIN_COUNT and k >= MIN_SHARE * n, \
                "%s: %s has %d %s entries of %d (needs %d and %.0f%%)" % (
                    what, c, k, label, n, MIN_COUNT, 100 * MIN_SHARE)


# ------------------------------------------------------------------ streams --
FREQ, PER = 5, SEC            # 5 tokens per second: capacity 5, one token per 200 ms
SEED_ADDED = 1000.0           # a seeded bucket is drained: added == taken, integers
SEED_ELAPSED = 2 * SEC
SEED_CREATED = T0 - SEC       # created + elapsed = T0 + 1 s, past every clock below


def f2b(x) -> int:
    return int(np.float64(x).view(np.uint64))


class Bucket:
    """One bucket's ops, drawn so that both halves of every column show.

    A seeded bucket starts drained (added == taken) with created + elapsed
    later than every clock of the stream, not equal to it: Take then moves
    `last` back to its own clock (bucket.go:199-200, `now.Before(last)`), so
    dt = now - last is 0 and nothing is refilled, as for a Take at exactly
    created + elapsed.  With no token it is denied with have bits 0 and remaining 0, with fewer
    than it asks for it is denied with have > 0, and otherwise granted.  Only
    a raising replica adds tokens (whole ones: the states stay integers); the
    stale ones between the Takes merge nothing.  A bucket the batch creates
    starts at capacity and refills by fractions of a token."""

    def __init__(self, name: bytes, seeded: bool):
        self.name, self.seeded = name, seeded
        self.top = SEED_ADDED if seeded else float(FREQ)   # the highest `added` sent so far

    def draw(self, rng, p_take=0.5):
        """-> (kind, count, added bits, taken bits, elapsed)"""
        u = rng.random()
        if u < p_take:
            return TAKE, int(rng.choice((1, 1, 2, 5))), 0, 0, 0
        kind = UPSERT if rng.random() < 0.2 else RECEIVE
        v = rng.random()
        if kind == RECEIVE and v < 0.10:                      # an incast request
            return RECEIVE, 0, 0, 0, 0
        if v < 0.45:                                          # raising: whole tokens
            self.top += float(rng.integers(1, 5))
            return kind, 0, f2b(self.top), f2b(1.0), int(rng.integers(1, SEC))
        if v < 0.50:                                          # a -0.0 field, stale otherwise
            return kind, 0, NEG_ZERO, f2b(1.0), 1
        return kind, 0, f2b(self.top - float(rng.integers(1, 10))), f2b(2.0), int(rng.integers(1, SEC))


class Stream:
    """Buckets of given op counts interleaved into one batch, each bucket's
    order kept; `cls[i]` is the size of op i's bucket (its fold class)."""

    def __init__(self, rng, sizes, seeded, step_ns=1000, p_take=0.5, prefix=b"c"):
        sizes = np.asarray(sizes)
        n = int(sizes.sum())
        owner = np.repeat(np.arange(len(sizes)), sizes)
        rng.shuffle(owner)
        buckets = [Bucket(prefix + b"%d" % i, bool(s)) for i, s in enumerate(seeded)]
        rows = [buckets[b].draw(rng, p_take) for b in owner]
        self.n = n
        self.names = [buckets[b].name for b in owner]
        self.kind = np.array([r[0] for r in rows], np.uint8)
        self.now = T0 + np.arange(n, dtype=np.int64) * step_ns
        self.freq = np.full(n, FREQ, np.int64)
        self.per = np.full(n, PER, np.int64)
        self.count = np.array([r[1] for r in rows], np.uint64)
        self.added = np.array([r[2] for r in rows], np.uint64)
        self.taken = np.array([r[3] for r in rows], np.uint64)
        self.elapsed = np.array([r[4] for r in rows], np.int64)
        self.cls = sizes[owner]
        sd = [b for b in buckets if b.seeded]
        k = len(sd)
        self.seed = ([b.name for b in sd], np.full(k, f2b(SEED_ADDED), np.uint64),
                     np.full(k, f2b(SEED_ADDED), np.uint64), np.full(k, SEED_ELAPSED, np.int64),
                     np.full(k, SEED_CREATED, np.int64))
        assert int(self.now[-1]) < SEED_CREATED + SEED_ELAPSED

    @property
    def args(self):
        """GPURepo.apply_mixed / oracle.Repo.apply_mixed positional arguments."""
        return (self.kind, self.names, self.now, self.freq, self.per, self.count, self.added,
                self.taken, self.elapsed)

    def seed_into(self, repo):
        repo.seed(*self.seed)

    def classes(self) -> dict:
        """label -> mask of the ops folded by that class of the ordered path."""
        return {"thread": self.cls <= LONG_SEG,
                "wave": (self.cls > LONG_SEG) & (self.cls <= HUGE_SEG),
                "block": self.cls > HUGE_SEG}


def small_stream() -> Stream:
    """1000 ops, under kSmallMax: a bucket of 260 ops and one of 60 (the small
    kernel's wave fold), thin buckets beside them; every other bucket is
    created by the batch.  Clocks 1 us apart."""
    rng = np.random.default_rng(4101)
    sizes = [260, 60] + [3] * 120 + [2] * 110 + [1] * 100
    assert sum(sizes) == 1000 < SMALL_MAX
    seeded = [1, 0] + [i % 2 for i in range(330)]
    return Stream(rng, sizes, seeded, prefix=b"s")


WAVE_SIZES = (33, 64, 65, 127, 128, 129)   # k_fold_wave: one-op, full and one-short tail windows
HOT_OPS = HUGE_SEG + 300                   # k_fold_block, k_huge_outputs


def large_stream() -> Stream:
    """About 36k ops: one bucket of more than kHugeSeg ops, two buckets of each
    k_fold_wave size (one seeded, one created by the batch), thin buckets."""
    rng = np.random.default_rng(4102)
    sizes = [HOT_OPS] + list(WAVE_SIZES) * 2 + [3] * 400 + [2] * 400 + [1] * 400
    seeded = [1] + [1] * 6 + [0] * 6 + [i % 2 for i in range(1200)]
    return Stream(rng, sizes, seeded, prefix=b"L")


def medium_stream() -> Stream:
    """About 1800 ops, just over kSmallMax and with no bucket over kHugeSeg:
    the ordered path's thread and wave folds alone store every entry (a huge
    bucket's fold clears the whole of three columns first, which would hide a
    store those two kernels miss)."""
    rng = np.random.default_rng(4103)
    sizes = list(WAVE_SIZES) * 2 + [3] * 120 + [2] * 120 + [1] * 120
    assert SMALL_MAX < sum(sizes) and max(sizes) <= HUGE_SEG
    seeded = [1] * 6 + [0] * 6 + [i % 2 for i in range(360)]
    return Stream(rng, sizes, seeded, prefix=b"M")


def stain_ops(n: int, tag: bytes = b"stain"):
    """n granted Takes with remaining > 0: every entry of every column
    non-default (status TAKE_OK, remaining and have > 0, a reply state).  A
    host call leaves them in the handle's staging buffers."""
    names = [tag + b"%d" % (i % 2000) for i in range(n)]
    kind = np.zeros(n, np.uint8)
    now = np.full(n, T0 - 5 * SEC, np.int64)
    z64, zi = np.zeros(n, np.uint64), np.zeros(n, np.int64)
    return (kind, names, now, np.full(n, 10**6, np.int64), np.full(n, SEC, np.int64),
            np.ones(n, np.uint64), z64, z64, zi)
