"""Directed op streams for the hot-bucket block fold (k_fold_block and its
window predicates, patrol_amd/csrc/phip_kernels.hpp), shared by the CPU model
tests (tests/test_fold_model.py) and the GPU parity tests
(tests/test_fold_directed.py).

Every case is a few hot buckets built on purpose, interleaved with a thin
tail of cold buckets (thread and wave folds beside the block fold), and a
`check(J, st)` that asserts, from the model program's JSON for the first hot
bucket (oracle/fold_model replay) and that bucket's statuses, that the stream
still shows the property it was written for.

The regime of the hand-built segments: rate 100 per second (interval 10 ms,
capacity 100), a seeded bucket with tokens = added - taken = 0.25 and
created + elapsed = T0, so a Take of 1 at a clock less than 2 ms past `last`
is denied, a Take exactly one interval past it is granted and leaves 0.25
again, a replica below the state merges nothing and a replica a little above
it raises it while tokens stay below 1.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess

import numpy as np

from tests._gen import SEC, T0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "oracle", "fold_model")

# The fold's tuning constants as these builders use them; test_fold_model.py
# compares them with the kernel header, so a retune fails there first.
LONG_SEG = 32
HUGE_SEG = 32768
FOLD_THREADS = 512
FOLD_PER = 1
HUGE_FIRST = 8
BURST_QUIET = 16
FOLD_WIN = FOLD_THREADS * FOLD_PER
SUM_CHUNK_OPS = FOLD_THREADS * FOLD_WIN      # kSumChunk windows of kFoldWin ops
WAVE_ROUND = 64                              # fold_window_absorb: ops per wave round

TAKE, RECEIVE, UPSERT = 0, 1, 2
ST_MERGED, ST_INCAST_REPLY, ST_INCAST_NOREPLY, ST_TAKE_OK, ST_TAKE_DENIED, ST_UPSERT_INSERTED = \
    1, 2, 3, 6, 7, 8
ST_CREATED = 0x80
NEG_ZERO = 0x8000000000000000
POS_INF = 0x7FF0000000000000
NAN = 0x7FF8000000000001
IV = 10_000_000                              # 100 per second


def f2b(x) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


class Seg:
    """One bucket's ops in order.  seed: (added bits, taken bits, elapsed,
    created) or None for a bucket absent at batch start."""

    def __init__(self, name: bytes, seed=None):
        self.name, self.seed = name, seed
        self.cols = [[] for _ in range(8)]   # kind now freq per count added taken elapsed
        self.marks = {}

    def __len__(self):
        return len(self.cols[0])

    def op(self, kind, now, freq=0, per=0, cnt=0, a=0, t=0, e=0):
        for c, v in zip(self.cols, (kind, now, freq, per, cnt, a, t, e)):
            c.append(int(v))

    def arrays(self):
        dt = (np.uint8, np.int64, np.int64, np.int64, np.uint64, np.uint64, np.uint64, np.int64)
        return [np.array(c, dtype=d) for c, d in zip(self.cols, dt)]


class Hot(Seg):
    """A hand-built segment in the module docstring's regime; the builder
    tracks the state its own ops lead to (A, T, E and the clock `last`)."""

    def __init__(self, name=b"hot", rng=None, seeded=True, a=5000.25, t=5000.0):
        self.A, self.T, self.E, self.created = a, t, SEC, T0 - SEC
        super().__init__(name, (f2b(a), f2b(t), self.E, self.created) if seeded else None)
        self.rng = rng or np.random.default_rng(1)
        self.count = 1

    @property
    def last(self):
        return self.created + self.E

    def pos_in_window(self):
        return len(self) % FOLD_WIN

    # ---- single ops
    def denied(self, count=None):
        self.op(TAKE, self.last + int(self.rng.integers(0, 2_000_000)), 100, SEC,
                self.count if count is None else count)

    def granted(self):
        """A Take one interval past `last`: refill exactly 1, granted, 0.25 left."""
        now = self.last + IV
        self.op(TAKE, now, 100, SEC, 1)
        self.E += IV
        self.A += 1.0
        self.T += 1.0

    def stale(self):
        r = self.rng.random(3)
        self.op(RECEIVE, T0, a=f2b(self.A - 10 * r[0] - 1), t=f2b(max(self.T - 10 * r[1] - 1, 0.0)),
                e=self.E - int(r[2] * 1e6) - 1)

    def raising(self, kind=RECEIVE):
        """A replica that raises every field a little; tokens stay 0.25."""
        self.T += 0.0005
        self.A = self.T + 0.25
        self.E += 1000
        self.op(kind, T0, a=f2b(self.A), t=f2b(self.T), e=self.E)

    def incast(self):
        self.op(RECEIVE, T0)

    def replica(self, a_bits, t_bits, e, kind=RECEIVE):
        self.op(kind, T0, a=a_bits, t=t_bits, e=e)

    # ---- stretches
    def unchanged(self, n):
        """n ops that change nothing: denied Takes, stale replicas, incasts."""
        for k in self.rng.integers(0, 10, n):
            if k < 5:
                self.denied()
            elif k < 9:
                self.stale()
            else:
                self.incast()

    def absorbing(self, n):
        """n ops of the absorbing model: denied Takes, raising and stale
        replicas, incast requests."""
        for k in self.rng.integers(0, 20, n):
            if k < 10:
                self.denied()
            elif k < 15:
                self.raising()
            elif k < 18:
                self.stale()
            else:
                self.incast()

    def takes_and_incasts(self, n):
        """n ops without any merge (G stays empty): denied Takes, incasts."""
        for k in self.rng.integers(0, 10, n):
            if k < 8:
                self.denied()
            else:
                self.incast()

    def incast_only(self, n):
        for _ in range(n):
            self.incast()

    def stale_only(self, n):
        for _ in range(n):
            self.stale()

    def raising_over(self):
        """A raising replica whatever the Takes since did to the state."""
        self.T += 1000.0
        self.A = self.T + 60.0
        self.E += 1000
        self.op(RECEIVE, T0, a=f2b(self.A), t=f2b(self.T), e=self.E)

    def fill_window(self, how="unchanged"):
        k = -len(self) % FOLD_WIN
        getattr(self, how)(k)

    def windows(self, k, how="unchanged"):
        assert self.pos_in_window() == 0
        getattr(self, how)(k * FOLD_WIN)

    def pad_huge(self, how="unchanged"):
        """Up to one op past kHugeSeg plus a whole window: a block-fold segment."""
        self.fill_window(how)
        while len(self) <= HUGE_SEG + FOLD_WIN:
            self.windows(1, how)


class Case:
    def __init__(self, name, segs, check, rng, cold=True):
        self.name, self.check = name, check
        self.marks = segs[0].marks
        cols = [s.arrays() for s in segs]
        owner = np.concatenate([np.full(len(s), i, np.int32) for i, s in enumerate(segs)])
        if cold:
            # the tail: 1-3 ops per bucket (thread fold) and 40-70 (wave fold)
            reps = np.concatenate([rng.integers(1, 4, 600), rng.integers(LONG_SEG + 8, 70, 12)])
            cold_ids = np.repeat(np.arange(len(reps)), reps)
            owner = np.concatenate([owner, np.full(len(cold_ids), -1, np.int32)])
        owner = owner[rng.permutation(len(owner))]
        n = len(owner)
        # the tail's ops: Takes and clean replicas on the batch's own clock
        kind = (rng.random(n) < 0.5).astype(np.uint8)
        now = T0 + np.arange(n, dtype=np.int64) * 20_000
        freq = np.full(n, 100, np.int64)
        per = np.full(n, SEC, np.int64)
        cnt = np.ones(n, np.uint64)
        taken = rng.integers(0, 10**4, n).astype(np.float64)
        added = taken + rng.random(n) * 100
        a, t = added.view(np.uint64).copy(), taken.view(np.uint64).copy()
        e = (rng.random(n) * (now - T0)).astype(np.int64)
        z = rng.random(n) < 0.03
        a[z], t[z], e[z] = 0, 0, 0
        out = [kind, now, freq, per, cnt, a, t, e]
        names = np.empty(n, object)
        self.hot = []
        for i, s in enumerate(segs):
            idx = np.nonzero(owner == i)[0]
            for dst, src in zip(out, cols[i]):
                dst[idx] = src
            names[idx] = s.name
            self.hot.append((s.name, idx))
        if cold:
            idx = np.nonzero(owner == -1)[0]
            ids = cold_ids[rng.permutation(len(cold_ids))]
            names[idx] = [b"cold%d" % i for i in ids]
        self.args = [out[0], list(names)] + out[1:]
        seeded = [s for s in segs if s.seed is not None]
        self.seed = None
        if seeded:
            self.seed = ([s.name for s in seeded], np.array([s.seed[0] for s in seeded], np.uint64),
                         np.array([s.seed[1] for s in seeded], np.uint64),
                         np.array([s.seed[2] for s in seeded], np.int64),
                         np.array([s.seed[3] for s in seeded], np.int64))
        self.seeds = {s.name: s.seed for s in segs}

    def seed_into(self, repo):
        if self.seed:
            repo.seed(*self.seed)


# ------------------------------------------------------------ the model ----
def write_replay(path, seed, cols):
    """One bucket's segment in fold_model's input layout (oracle/fold_model.hip)."""
    kind = cols[0]
    n = len(kind)
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", 0x314D4650, n, 1 if seed is not None else 0, 0))
        s = seed or (0, 0, 0, 0)
        f.write(struct.pack("<QQqq", *[int(x) for x in s]))
        f.write(kind.astype(np.uint8).tobytes() + b"\0" * (-n % 8))
        for c, d in zip(cols[1:], (np.int64, np.int64, np.int64, np.uint64, np.uint64, np.uint64,
                                   np.int64)):
            f.write(np.ascontiguousarray(c, d).tobytes())


def read_replay(path):
    with open(path, "rb") as f:
        b = f.read()
    magic, n, existed, _ = struct.unpack_from("<4I", b, 0)
    assert magic == 0x324D4650
    final = struct.unpack_from("<QQqq", b, 16)
    o = 48
    pad = n + (-n % 8)
    out = {"existed": existed, "final": final}
    out["status"] = np.frombuffer(b, np.uint8, n, o); o += pad
    out["remaining"] = np.frombuffer(b, np.uint64, n, o); o += 8 * n
    out["have"] = np.frombuffer(b, np.uint64, n, o); o += 8 * n
    out["has_reply"] = np.frombuffer(b, np.uint8, n, o); o += pad
    out["reply_added"] = np.frombuffer(b, np.uint64, n, o); o += 8 * n
    out["reply_taken"] = np.frombuffer(b, np.uint64, n, o); o += 8 * n
    out["reply_elapsed"] = np.frombuffer(b, np.int64, n, o); o += 8 * n
    out["reply_created"] = np.frombuffer(b, np.int64, n, o); o += 8 * n
    assert o == len(b)
    return out


def replay(tmpdir, seed, cols, tag="seg"):
    """Run oracle/fold_model replay on one segment -> (JSON dict, per-op results)."""
    path = os.path.join(str(tmpdir), tag + ".pfm")
    write_replay(path, seed, cols)
    p = subprocess.run([MODEL, "replay", path, path + ".out"], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(p.stdout), read_replay(path + ".out")


def segment_of(case, k=0):
    """(seed, columns) of the case's k-th hot bucket."""
    name, idx = case.hot[k]
    a = case.args
    return case.seeds[name], [a[0][idx]] + [a[j][idx] for j in range(2, 9)]


# ------------------------------------------------- the C3 absorbing shape --
def c3_segment(name, n, rng, seed=None):
    """The absorbing shape of test_hot_bucket_absorbing_merges for one bucket:
    half Takes of 1 at 100 per second, half clean replicas whose elapsed runs
    behind the clock.  2 us per op of the bucket (a window of 512 ops refills
    a tenth of a token), so that most windows are absorbed."""
    s = Seg(name, seed)
    kind = (rng.random(n) < 0.5).astype(np.uint8)
    now = T0 + np.arange(n, dtype=np.int64) * 2_000
    taken = rng.integers(0, 10**4, n).astype(np.float64)
    added = taken + rng.random(n) * 100
    e = (rng.random(n) * (now - T0)).astype(np.int64)
    s.cols = [kind, now, np.full(n, 100, np.int64), np.full(n, SEC, np.int64),
              np.ones(n, np.uint64), added.view(np.uint64).copy(), taken.view(np.uint64).copy(), e]
    return s


class ArraySeg(Seg):
    def arrays(self):
        return self.cols


def _c3(name, n, rng):
    s = c3_segment(name, n, rng)
    s.__class__ = ArraySeg
    return s


def case_length(n, variant=None):
    rng = np.random.default_rng(1000 + n % 997 + (7 if variant else 0))
    s = _c3(b"hot", n, rng)
    cols = s.cols
    if variant == "take":        # position n - 1: a granted Take (a clock far ahead)
        cols[0][-1], cols[1][-1] = TAKE, cols[1][-1] + 10 * SEC
    elif variant == "merge":     # a replica above everything merged so far
        cols[0][-1] = RECEIVE
        cols[5][-1], cols[6][-1], cols[7][-1] = f2b(3e4 + 50), f2b(3e4), 100 * SEC

    def check(J, st):
        assert J["windows"] == -(-n // FOLD_WIN), J
        if n > HUGE_SEG:
            assert J["absorbed"] > 0, J
        if variant == "take":
            assert st[-1] == ST_TAKE_OK
        if variant == "merge":
            assert st[-1] == ST_MERGED and J["raising_merges"] > 0

    return Case("length", [s], check, rng)


def case_count(h):
    rng = np.random.default_rng(2000 + h)
    segs = [_c3(b"hot%02d" % i, HUGE_SEG + 1 + FOLD_WIN * i, rng) for i in range(h)]

    def check(J, st):
        assert J["ops"] == HUGE_SEG + 1 and J["absorbed"] > 0, J

    return Case("count", segs, check, rng)


# ------------------------------------------------------ window decisions --
def case_quiet():
    rng = np.random.default_rng(3001)
    s = Hot(rng=rng)
    s.windows(2, "absorbing")      # G is not empty when the quiet stretch starts
    s.pad_huge("unchanged")

    def check(J, st):
        assert J["quiet"] >= 60 and J["absorbed"] >= 1 and J["folded"] == 0 and J["runs"] == 1, J

    return Case("quiet", [s], check, rng)


def case_absorbed():
    rng = np.random.default_rng(3002)
    s = Hot(rng=rng)
    s.pad_huge("absorbing")

    def check(J, st):
        assert J["absorbed"] >= 60 and J["folded"] == 0 and J["runs"] == 1, J
        assert J["incast_reply"] > 100 and J["raising_merges"] > 1000, J

    return Case("absorbed", [s], check, rng)


def case_bound(d):
    """The integer-exact window: added 5003, taken 5000, one Take two
    intervals past `last` (have = 3 + 2 = 5 = the absorbing bound, exactly),
    t = bound + d; a replica raising `taken` follows it, so the window is not
    quiet and the bound alone decides."""
    rng = np.random.default_rng(3010 + d)
    s = Hot(rng=rng, a=5003.0, t=5000.0)
    s.count = 6                    # tokens are 3: the other windows' Takes ask for more
    s.windows(3, "unchanged")
    for _ in range(200):
        s.stale()
    s.marks["take"] = len(s)
    s.op(TAKE, s.last + 2 * IV, 100, SEC, 5 + d)
    for _ in range(100):
        s.incast()
    s.replica(f2b(5003.0), f2b(5001.0), s.E)
    s.marks["window"] = len(s) // FOLD_WIN
    s.fill_window("incast_only")
    s.pad_huge("unchanged")

    def check(J, st):
        w = J["classes"][s.marks["window"]]
        assert w == ("A" if d > 0 else "F"), (d, w)
        assert st[s.marks["take"]] == (ST_TAKE_DENIED if d > 0 else ST_TAKE_OK)

    return Case("bound", [s], check, rng)


def case_edges(where):
    rng = np.random.default_rng({"last": 3021, "first": 3022, "straddle": 3023}[where])
    s = Hot(rng=rng)
    s.windows(2, "absorbing")
    for rep in range(3):
        if where in ("last", "straddle"):
            s.absorbing(FOLD_WIN - 1)
            s.granted()            # the window's last op: its run starts at the next p0
        if where in ("first", "straddle"):
            s.granted()            # the window's first op
            s.absorbing(FOLD_WIN - 1)
        s.windows(1, "absorbing")
    s.pad_huge("absorbing")

    def check(J, st):
        assert J["take_ok"] == (6 if where == "straddle" else 3), J
        assert J["runs"] == 1 + J["take_ok"] and J["exact"]["why"] == "never", J
        assert J["run_at_window_start"] == (0 if where == "first" else 3), J
        assert J["change_at_window_first_op"] == (0 if where == "last" else 3), J

    return Case("edges", [s], check, rng)


def case_burst_exact():
    """Exact mode (a -0.0 replica in window 0), then raising replicas, each a
    run, kBurstQuiet - 1, kBurstQuiet and kBurstQuiet + 1 unchanged ops apart
    (fold_window's burst ends after kBurstQuiet unchanged ops), and one in a
    window's last op after 511 unchanged ones."""
    rng = np.random.default_rng(3031)
    s = Hot(rng=rng)
    s.raising()
    s.replica(f2b(1.0), NEG_ZERO, 0)
    s.fill_window("unchanged")
    nchg = 1
    for rep in range(2):
        s.unchanged(5 + rep)
        for gap in (BURST_QUIET - 1, BURST_QUIET, BURST_QUIET + 1, BURST_QUIET, BURST_QUIET + 1,
                    2 * BURST_QUIET + 1, 0, 0, BURST_QUIET):
            s.raising()
            s.unchanged(gap)
            nchg += 1
        s.fill_window("unchanged")
    s.unchanged(FOLD_WIN - 1)
    s.raising()
    nchg += 1
    s.pad_huge("unchanged")

    def check(J, st):
        assert J["exact"] == {"why": "negzero", "pos": 0, "run": 0, "g_nonempty": False}, J
        assert J["runs"] == 1 + nchg and J["folded"] == 4 and J["absorbed"] == 0, J
        assert J["run_at_window_start"] == 1, J

    return Case("burst_exact", [s], check, rng)


def case_burst_absorb(raises):
    """Absorbing mode: granted Takes 64, 65, 128 and 129 ops apart
    (fold_window_absorb's wave rounds of 64 ops end after two without a
    change), with only unchanged ops between or with raising replicas among
    them, and one as a window's last op after 511 others."""
    rng = np.random.default_rng(3032 + raises)
    s = Hot(rng=rng)
    fill = "absorbing" if raises else "unchanged"
    s.windows(1, "absorbing")
    ngr = 0
    for start in (3, 0, 61):
        s.fill_window(fill)
        getattr(s, fill)(start)
        for gap in (2 * WAVE_ROUND - 1, 2 * WAVE_ROUND, WAVE_ROUND - 1, WAVE_ROUND):
            s.granted()
            getattr(s, fill)(gap)
            ngr += 1
        s.granted()
        ngr += 1
    s.fill_window(fill)
    getattr(s, fill)(FOLD_WIN - 1)
    s.granted()
    ngr += 1
    s.pad_huge(fill)

    def check(J, st):
        assert J["take_ok"] == ngr and J["runs"] == 1 + ngr and J["folded"] == 4, J
        assert J["exact"]["why"] == "never" and J["run_at_window_start"] == 1, J

    return Case("burst_absorb", [s], check, rng)


def case_lowering():
    """A replica lifts tokens above capacity; the next Take's refill is
    negative and lowers `added`: exact from that run, with merges absorbed
    before it.  Raising replicas (now runs) and more Takes follow."""
    rng = np.random.default_rng(3041)
    s = Hot(rng=rng)
    s.windows(3, "absorbing")
    s.absorbing(100)
    s.A = s.T + 150.0
    s.replica(f2b(s.A), f2b(s.T), s.E)
    s.stale_only(20)
    s.marks["take"] = len(s)
    s.op(TAKE, s.last + 1000, 100, SEC, 1)     # missing = 100 - 150: added drops by 50
    s.A, s.T, s.E = s.A - 50.0, s.T + 1.0, s.E + 1000
    for _ in range(40):
        s.raising_over()
        s.stale()
        s.op(TAKE, s.last + int(rng.integers(0, 2_000_000)), 100, SEC, 1)
    s.fill_window("stale_only")
    for _ in range(3):
        for _ in range(FOLD_WIN // 4):
            s.stale()
            s.raising_over()
            s.stale()
            s.op(TAKE, s.last + int(rng.integers(0, 2_000_000)), 100, SEC, 1)
    s.pad_huge("stale_only")

    def check(J, st):
        assert J["exact"]["why"] == "lowered" and J["exact"]["pos"] == s.marks["take"], J
        assert J["exact"]["g_nonempty"] and J["absorbed"] >= 3, J
        assert st[s.marks["take"]] == ST_TAKE_OK and J["take_ok"] > 100, J
        assert J["raising_merges"] > 500 and J["runs"] > 800, J

    return Case("lowering", [s], check, rng)


def case_elapsed_wrap():
    """A granted Take whose dt wraps `elapsed` below its old value (created +
    elapsed = 0, elapsed near the top of int64): only `elapsed` is lowered."""
    rng = np.random.default_rng(3051)
    s = Hot(rng=rng)
    s.E = (1 << 63) - 1 - 10**18
    s.created = -s.E
    s.seed = (f2b(s.A), f2b(s.T), s.E, s.created)
    for _ in range(2 * FOLD_WIN + 37):        # no Take before it: any would be granted
        k = rng.integers(0, 4)
        if k == 0:
            s.incast()
        elif k == 1:
            s.stale()
        else:                                  # raise added and taken only
            s.T += 0.0005
            s.A = s.T + 0.25
            s.replica(f2b(s.A), f2b(s.T), 0)
    s.marks["take"] = len(s)
    s.op(TAKE, T0, 100, SEC, 1)
    for _ in range(300):
        s.op(TAKE, T0 + int(rng.integers(0, SEC)), 100, SEC, 1)
        s.stale()
    s.pad_huge("stale_only")

    def check(J, st):
        assert J["exact"]["why"] == "lowered" and J["exact"]["pos"] == s.marks["take"], J
        assert J["exact"]["g_nonempty"] and J["absorbed"] == 2, J
        assert st[s.marks["take"]] == ST_TAKE_OK

    return Case("elapsed_wrap", [s], check, rng)


CREATORS = ("take", "receive", "receive_zero", "upsert")


def case_negzero_first(creator=None):
    """A -0.0 replica in the first window that is not quiet, with nothing
    merged before it (G empty): the segment is exact from the run in effect.
    The state's `taken` is +0.0, where Go's merge and the E max differ.
    creator: the bucket is absent at batch start and this op creates it."""
    rng = np.random.default_rng(3061 + (CREATORS.index(creator) + 1 if creator else 0))
    s = Hot(rng=rng, seeded=creator is None, a=0.25, t=0.0)
    if creator is None:
        s.windows(2, "takes_and_incasts")
        s.takes_and_incasts(100)
    elif creator == "take":
        s.op(TAKE, T0, 100, SEC, 1)
    elif creator == "receive":
        s.replica(f2b(0.25), 0, SEC)
    elif creator == "receive_zero":
        s.incast()
    else:
        s.replica(f2b(0.25), 0, SEC, UPSERT)
    first = len(s) // FOLD_WIN
    s.takes_and_incasts(50)
    s.replica(f2b(0.125), NEG_ZERO, 5)          # taken: +0.0 stays under Go's `<`
    s.replica(f2b(0.375), NEG_ZERO, SEC + 7)
    s.takes_and_incasts(50)
    s.replica(NEG_ZERO, NEG_ZERO, SEC + 9)
    s.pad_huge("takes_and_incasts")

    def check(J, st):
        assert J["exact"] == {"why": "negzero", "pos": first * FOLD_WIN, "run": 0,
                              "g_nonempty": False}, J
        assert J["classes"][:first] == "Q" * first and J["classes"][first] == "F", J
        if creator:
            want = {"take": ST_TAKE_OK, "receive": ST_MERGED, "receive_zero": ST_INCAST_NOREPLY,
                    "upsert": ST_UPSERT_INSERTED}[creator] | ST_CREATED
            assert st[0] == want, (st[0], want)

    return Case("negzero_first", [s], check, rng)


def case_negzero_late():
    """A -0.0 replica after merges were absorbed: a run holding the joined
    state is inserted and the segment is exact from it."""
    rng = np.random.default_rng(3071)
    s = Hot(rng=rng, a=0.25, t=0.0)

    def raise_added():
        s.A += 0.0005
        s.E += 1000
        s.replica(f2b(s.A), 0, s.E)

    for _ in range(3 * FOLD_WIN + 20):
        k = rng.integers(0, 10)
        if k < 5:
            s.denied()
        elif k < 8:
            raise_added()
        else:
            s.incast()
    s.replica(f2b(s.A + 0.001), NEG_ZERO, s.E)
    s.fill_window("takes_and_incasts")
    for _ in range(2 * FOLD_WIN):     # added passes 1: Takes are granted again
        raise_added()
        s.denied()
    s.pad_huge("takes_and_incasts")

    def check(J, st):
        assert J["classes"][:4] == "AAAF", J
        assert J["exact"] == {"why": "negzero", "pos": 3 * FOLD_WIN, "run": 1,
                              "g_nonempty": True}, J
        assert J["take_ok"] > 0, J

    return Case("negzero_late", [s], check, rng)


def case_added_zero():
    """Seeded added == 0: the first Take, denied, still writes added =
    capacity (bucket.go:194-196)."""
    rng = np.random.default_rng(3081)
    s = Hot(rng=rng, a=0.0, t=100.0)
    s.A = 100.0
    s.incast_only(40)
    s.marks["take"] = len(s)
    s.denied()
    s.fill_window("takes_and_incasts")     # no merge: only added == 0 keeps window 0 from quiet
    s.pad_huge("absorbing")

    def check(J, st):
        assert J["denied_changed"] == 1 and st[s.marks["take"]] == ST_TAKE_DENIED, J
        assert J["classes"][0] == "F" and J["absorbed"] >= 60 and J["runs"] == 2, J

    return Case("added_zero", [s], check, rng)


DOMAIN = ("mixed", "interval0", "negative", "count0", "nan", "inf")


def case_domain():
    """Windows outside the absorbing bound's domain between ordinary ones.
    Every window holds raising replicas, so none is quiet: the ordinary ones
    are absorbed, the others folded -- except the NaN replica field, which
    the merge ignores (enc_replica maps it to 0): its window is absorbed like
    its neighbours.  +Inf comes last, it ends the regime."""
    rng = np.random.default_rng(3091)
    s = Hot(rng=rng)
    where = {}
    for what in DOMAIN:
        s.windows(2, "absorbing")
        where[what] = len(s) // FOLD_WIN
        for k in rng.integers(0, 20, FOLD_WIN):
            if k >= 10:
                if what == "nan" and k < 13:
                    s.replica(NAN, f2b(s.T), s.E)
                elif what == "inf" and k == 19:
                    s.replica(POS_INF, f2b(s.T), s.E)
                elif k < 15:
                    s.raising()
                else:
                    s.stale()
            elif what == "mixed":
                s.denied(count=1 + int(k) % 2)
            elif what == "interval0":
                s.op(TAKE, s.last + 1000, 0, 0, 1)
            elif what == "negative":
                s.op(TAKE, s.last + 1000, -100, SEC, 1)
            elif what == "count0" and k < 2:
                s.op(TAKE, s.last + 1000, 100, SEC, 0)     # granted: elapsed and added move
                s.E += 1000
                s.A += 1e-4
            elif what == "count0":
                s.incast()
            else:
                s.denied()
    s.pad_huge("absorbing")

    def check(J, st):
        c = J["classes"]
        for what, w in where.items():
            assert c[w] == ("A" if what == "nan" else "F"), (what, w, c)
            assert c[w - 2:w] == "AA", (what, w, c)
        assert c[:where["inf"]].count("F") == 4, c

    return Case("domain", [s], check, rng)


def case_specials_late():
    """The absorbing stream with special values in its last tenth: a NaN
    `added` replica, then a +Inf `taken`, then a +Inf `added` (tokens Inf -
    Inf: the NaN whose bits depend on the machine's subtraction)."""
    rng = np.random.default_rng(3101)
    s = Hot(rng=rng)
    s.windows(60, "absorbing")
    s.absorbing(100)
    s.replica(NAN, f2b(s.T), s.E)
    s.absorbing(600)
    s.replica(f2b(s.A), POS_INF, s.E)
    s.absorbing(700)
    s.replica(POS_INF, f2b(s.T), s.E)
    s.absorbing(300)
    s.replica(0xFFF8000000000000, 0xFFF0000000000000, s.E + 5)
    s.pad_huge("absorbing")

    def check(J, st):
        # +Inf `taken` arrives inside window 61 (Takes stay denied: absorbed);
        # from window 62 on the state is outside the bound's domain
        assert J["classes"][:62] == "A" * 62 and J["classes"][62] == "F", J

    return Case("specials_late", [s], check, rng)


LENGTHS = [(HUGE_SEG, None), (HUGE_SEG + 1, None), (HUGE_SEG + FOLD_WIN, None),
           (HUGE_SEG + FOLD_WIN + 1, None), (SUM_CHUNK_OPS, None), (SUM_CHUNK_OPS + 1, "take"),
           (SUM_CHUNK_OPS + 1, "merge"), (SUM_CHUNK_OPS + FOLD_WIN + 1, None)]
COUNTS = [1, HUGE_FIRST, HUGE_FIRST + 1, 17]

# id -> builder of every directed case but the segment-count ones
CASES = {}
for _n, _v in LENGTHS:
    CASES["length-%d%s" % (_n, "-" + _v if _v else "")] = (lambda n=_n, v=_v: case_length(n, v))
CASES["quiet"] = case_quiet
CASES["absorbed"] = case_absorbed
for _d in (-1, 0, 1):
    CASES["bound%+d" % _d] = (lambda d=_d: case_bound(d))
for _w in ("last", "first", "straddle"):
    CASES["edge-" + _w] = (lambda w=_w: case_edges(w))
CASES["burst-exact"] = case_burst_exact
CASES["burst-absorb"] = lambda: case_burst_absorb(0)
CASES["burst-absorb-raises"] = lambda: case_burst_absorb(1)
CASES["lowering"] = case_lowering
CASES["elapsed-wrap"] = case_elapsed_wrap
CASES["negzero-first-seeded"] = case_negzero_first
for _c in CREATORS:
    CASES["negzero-first-absent-" + _c] = (lambda c=_c: case_negzero_first(c))
CASES["negzero-late"] = case_negzero_late
CASES["added-zero"] = case_added_zero
CASES["domain"] = case_domain
CASES["specials-late"] = case_specials_late
