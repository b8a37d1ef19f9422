"""phip_evict_idle on the GPU (include/patrolhip.h "Evict idle buckets").

The expected result of every sweep is computed here, in Python integers,
from the dump taken before it: survivors are the buckets that fail the rule
idle = now - (created + elapsed) >= idle_ns (idle 0 when negative, saturating
at INT64_MAX).  Behaviour after a sweep is compared with an oracle Repo
seeded with exactly those survivors: evicting a bucket is, for that bucket,
a node restart (repo.go:96-106).  Bit-exact throughout.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from oracle import go_semantics as G  # noqa: E402
from tests import _evict_cases as EC  # noqa: E402
from tests import _gen  # noqa: E402

SEC = 10**9
T0 = _gen.T0
I64MAX, I64MIN = 2**63 - 1, -2**63
INLINE = 22   # kInlineName: longer names live in the arena


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def f2b(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def gpu_dump(repo):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}
    assert len(repo) == len(d), (len(repo), len(d))
    return d


def assert_same_dump(g, o):
    assert len(g) == len(o), (len(g), len(o))
    bad = [k for k in o if g.get(k) != o[k]]
    assert not bad, [(k, g.get(k), o[k]) for k in bad[:5]]


def idle_of(created, elapsed, now):
    d = now - (created + elapsed)
    return 0 if d < 0 else min(d, I64MAX)


def survivors(dump, now, idle_ns):
    return {k: v for k, v in dump.items() if idle_of(v[3], v[2], now) < idle_ns}


def long_bytes(names):
    return sum(len(k) for k in names if len(k) > INLINE)


def oracle_of(dump):
    o = O.Repo()
    ks = list(dump)
    if ks:
        o.seed(ks, [dump[k][0] for k in ks], [dump[k][1] for k in ks], [dump[k][2] for k in ks],
               [dump[k][3] for k in ks])
    return o


def seed(repo, rows):
    """rows: [(name, added bits, taken bits, elapsed, created)]."""
    repo.seed([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows],
              [r[3] for r in rows], [r[4] for r in rows])


def sweep(repo, now, idle_ns, **kw):
    """One sweep checked against the model -> (stats, survivors dict)."""
    before = gpu_dump(repo)
    used = repo.evict_idle(now, 1, dry_run=True)["arena_used"]
    st = repo.evict_idle(now, idle_ns, **kw)
    want = survivors(before, now, idle_ns)
    assert st["idle"] == len(before) - len(want)
    assert st["evicted"] == st["idle"] and st["buckets"] == len(want) == len(repo)
    assert st["slots"] == repo.capacity
    if st["evicted"]:
        assert st["arena_used"] == long_bytes(want)
        assert st["arena_freed"] == used - st["arena_used"] == long_bytes(set(before) - set(want))
    assert_same_dump(gpu_dump(repo), want)
    return st, want


A, T = f2b(10.0), f2b(3.0)

# (created, elapsed, now, idle_ns, evicted)
RULE_ROWS = [
    (T0, 5, T0 + 105, 100, True),                 # idle == idle_ns
    (T0, 5, T0 + 104, 100, False),                # idle == idle_ns - 1
    (T0, 1000, T0 + 10, 1, False),                # now < last: idle is 0
    (T0, 10, T0 + 10, 1, False),                  # now == last
    (T0, 10, T0 + 11, 1, True),
    (I64MIN, 0, I64MAX, I64MAX, True),            # idle saturates at INT64_MAX
    (I64MIN, 0, I64MAX - 1, I64MAX, True),        # (2^64 - 2 saturates too)
    (0, 0, I64MAX - 1, I64MAX, False),            # idle == INT64_MAX - 1, no overflow involved
    (I64MAX, I64MAX, I64MAX, 1, False),           # created + elapsed = 2^64 - 2 (wrapped: -2, idle)
    (I64MIN, I64MIN, I64MIN, I64MAX, True),       # created + elapsed = -2^64 (wrapped: 0, kept)
    (I64MIN, -1, I64MIN, 1, True),                # last = -2^63 - 1 < now
    (T0, -50, T0 + 50, 100, True),                # negative elapsed: last before created
    (T0, -50, T0 + 50, 101, False),
]


def test_rule_edges(pa):
    """Fails without the feature (no evict_idle).  One bucket per row; every
    sweep also checked as a whole against the model."""
    repo = pa.GPURepo(log2_slots=5, arena_bytes=4096)
    for k, (created, elapsed, now, idle_ns, gone) in enumerate(RULE_ROWS):
        name = b"edge-%d" % k
        seed(repo, [(name, A, T, elapsed, created)])
        assert (idle_of(created, elapsed, now) >= idle_ns) == gone, k
        sweep(repo, now, idle_ns)
        assert (repo.get(name) is None) == gone, (k, RULE_ROWS[k])
    # a zero-state bucket left by an incast request (repo.go:78-90) ages from its creation
    out = repo.receive_soa([b"incast-left"], [0], [0], [0], T0)
    assert out["status"][0] & 0x80
    st = repo.get(b"incast-left")
    assert (st.added, st.taken, st.elapsed, st.created) == (0, 0, 0, T0)
    sweep(repo, T0 + 99, 100)
    assert repo.get(b"incast-left") is not None
    sweep(repo, T0 + 100, 100)
    assert repo.get(b"incast-left") is None
    # idle_ns <= 0 and unknown flag bits: PHIP_ERR_INVALID, the table untouched
    seed(repo, [(b"stays", A, T, 0, T0)])
    snap = repo.snapshot().tobytes()
    for bad in (0, -1, I64MIN):
        with pytest.raises(pa.PatrolHipError) as e:
            repo.evict_idle(I64MAX, bad)
        assert e.value.code == -1
    for flags in (0x1, 0x20, 0x100, 0x40 | 0x2):
        assert repo.L.phip_evict_idle(repo.h, I64MAX, 1, 1, None, flags) == -1
    assert repo.L.phip_evict_idle(repo.h, I64MAX, 1, 1, None, 0x80) == 0   # out may be NULL
    assert repo.snapshot().tobytes() == snap
    before = gpu_dump(repo)
    assert repo.L.phip_evict_idle(repo.h, T0 + SEC, SEC, 1, None, 0) == 0
    assert_same_dump(gpu_dump(repo), survivors(before, T0 + SEC, SEC))
    assert repo.get(b"stays") is None
    repo.close()


def test_probe_chains(pa):
    """Two tag bits and a fixed seed: four home slots for 40 buckets, every
    chain long.  Every second bucket (in insertion order) goes."""
    repo = pa.GPURepo(log2_slots=6, arena_bytes=4096, debug_tag_bits=2, hash_seed=0)
    names = [(b"pc-%d" % k) + (b"-long-enough-for-the-arena" if k % 5 == 0 else b"")
             for k in range(40)]
    for k, nm in enumerate(names):   # one by one: insertion order is chain order
        seed(repo, [(nm, f2b(100.0 + k), f2b(float(k)), k, T0 if k % 2 == 0 else T0 + 10 * SEC)])
    assert repo.table_stats()["max_probe"] >= 9
    now = T0 + 10 * SEC
    st, want = sweep(repo, now, 5 * SEC)
    assert st["evicted"] == 20 and sorted(want) == sorted(names[1::2])
    for k, nm in enumerate(names):
        got = repo.get(nm)
        if k % 2 == 0:
            assert got is None
        else:
            assert (got.added, got.taken, got.elapsed, got.created) == want[nm]
    dgs, found = repo.export_datagrams(names)
    assert list(found) == [k % 2 for k in range(40)]
    for k in range(1, 40, 2):
        v = want[names[k]]
        assert dgs[k] == pa.marshal(names[k], pa.BucketState(*v))
    ts = repo.table_stats()
    assert ts["buckets"] == 20 and ts["slots"] == 64
    assert len(repo) == len(repo.dump()) == 20
    repo.close()


LENGTHS = [0, 1, 14, 15, 22, 23, 24, 100, 231]


@pytest.mark.parametrize("flip", [False, True])
def test_name_lengths(pa, flip):
    """Inline, two-word, three-word and arena names, some idle and some not;
    the arena is compacted and its cursor left right behind the survivors."""
    repo = pa.GPURepo(log2_slots=6, arena_bytes=1024)
    rows = []
    for L in LENGTHS:
        # two names per length, one idle and one kept (flip swaps the roles);
        # the one empty name is kept in one case and idle in the other
        for tagc, idle in ((b"i", not flip), (b"k", flip)) if L else ((b"", flip),):
            nm = tagc + b"n" * (L - 1) if L else b""
            rows.append((nm, f2b(50.0 + L), f2b(float(L)), L, T0 if idle else T0 + 100 * SEC))
    seed(repo, rows)
    assert len(repo) == 2 * len(LENGTHS) - 1
    all_long = long_bytes(r[0] for r in rows)
    assert repo.evict_idle(T0, 1, dry_run=True)["arena_used"] == all_long
    st, want = sweep(repo, T0 + 100 * SEC, 50 * SEC)
    assert 0 < st["evicted"] < len(rows)
    assert st["arena_used"] == long_bytes(want) > 0
    assert st["arena_freed"] == all_long - long_bytes(want) > 0
    assert (b"" in want) == (not flip)
    # new arena names land behind the survivors', which stay intact
    o = oracle_of(want)
    new = [b"N" * 23, b"M" * 231, b"short-new"]
    a, t, e = _gen.clean_states(np.random.default_rng(5), len(new))
    out = repo.receive_soa(new, a, t, e, T0 + 200 * SEC)
    ref = o.receive_soa(new, a, t, e, T0 + 200 * SEC)
    assert np.array_equal(out["status"], ref[0])
    assert_same_dump(gpu_dump(repo), o.dump())
    assert repo.evict_idle(T0, 1, dry_run=True)["arena_used"] == long_bytes(want) + 23 + 231
    repo.close()


def test_behaviour_afterwards_vs_oracle(pa):
    """Receive and mixed batches over evicted, surviving and new names: the
    swept table behaves as the oracle seeded with the survivors."""
    rng = np.random.default_rng(11)
    K = 60
    names = [(b"bk-%d" % k) + (b"-with-an-arena-length-tail" if k % 7 == 0 else b"") for k in range(K)]
    a, t, e = _gen.clean_states(rng, K)
    e = e % (50 * SEC)
    created = np.where(np.arange(K) % 2 == 0, T0, T0 + 1000 * SEC)
    repo = pa.GPURepo(log2_slots=7, arena_bytes=4096)
    repo.seed(names, a, t, e, created)
    now = T0 + 1000 * SEC
    st, want = sweep(repo, now, 900 * SEC)
    gone = [nm for nm in names if nm not in want]
    assert len(gone) == 30 == st["evicted"]
    o = oracle_of(want)
    fresh = [b"new-%d" % k for k in range(10)] + [b"new-name-long-enough-for-the-arena-%d" % k
                                                  for k in range(3)]
    pool = gone + list(want) + fresh

    # ReplicatedRepo.Receive over datagrams, incast requests included
    n = 200
    pick = [pool[i] for i in rng.integers(0, len(pool), n)]
    ra, rt, re = _gen.clean_states(rng, n)
    z = rng.random(n) < 0.3
    ra[z], rt[z], re[z] = 0, 0, 0
    dgs = [pa.marshal(pick[i], pa.BucketState(int(ra[i]), int(rt[i]), int(re[i]), 0)) for i in range(n)]
    out = repo.receive_datagrams(dgs, now + 1)
    rs, rra, rrt, rre, stop = o.receive(dgs, now + 1)
    assert out["stop"] == stop == n
    assert np.array_equal(out["status"], rs)
    seen = set()
    for i, nm in enumerate(pick):   # the first message of an evicted name recreates it
        if nm not in seen and nm in gone:
            assert out["status"][i] & 0x80, (i, nm)
        if nm not in seen and nm in want:
            assert not out["status"][i] & 0x80, (i, nm)
        seen.add(nm)
    rep = (rs & 0x7F) == 2
    assert rep.any()
    assert np.array_equal(out["reply"]["a"][rep], rra[rep])
    assert np.array_equal(out["reply"]["t"][rep], rrt[rep])
    assert np.array_equal(out["reply"]["e"][rep], rre[rep])
    assert_same_dump(gpu_dump(repo), o.dump())

    # a second sweep, then an ordered TAKE / RECEIVE / UPSERT stream
    st2, want2 = sweep(repo, now + 2000 * SEC, 1500 * SEC)
    assert st2["evicted"] > 0
    o = oracle_of(want2)
    gone2 = [nm for nm in pool if nm not in want2]
    n = 400
    pick = [pool[i] for i in rng.integers(0, len(pool), n)]
    kind = rng.integers(0, 3, n).astype(np.uint8)
    nows = now + 2000 * SEC + np.sort(rng.integers(0, 5 * SEC, n))
    freq = rng.choice(np.array([100, 5, 3], np.int64), n)
    per = rng.choice(np.array([SEC, 60 * SEC], np.int64), n)
    cnt = rng.integers(0, 4, n).astype(np.uint64)
    ma, mt, me = _gen.clean_states(rng, n)
    z = rng.random(n) < 0.2
    ma[z], mt[z], me[z] = 0, 0, 0
    args = (kind, pick, nows, freq, per, cnt, ma, mt, me)
    out = repo.apply_mixed(*args)
    ref = o.apply_mixed(*args)
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["remaining"], ref["remaining"])
    take = kind == 0
    assert np.array_equal(out["have"][take], ref["have"][take])
    stt = ref["status"] & 0x7F
    rep = (kind == 0) | (kind == 2) | (stt == 2) | (stt == 3)
    for f, k in (("a", "reply_added"), ("t", "reply_taken"), ("e", "reply_elapsed"),
                 ("c", "reply_created")):
        assert np.array_equal(out["reply"][f][rep], ref[k][rep]), f
    seen = set()
    ncreated = 0
    for i, nm in enumerate(pick):
        if nm not in seen and kind[i] != 2:   # (an Upsert inserts without GetBucket)
            assert bool(out["status"][i] & 0x80) == (nm in gone2), (i, nm)
            ncreated += nm in gone2
        seen.add(nm)
    assert ncreated > 0
    assert_same_dump(gpu_dump(repo), o.dump())
    repo.close()


@pytest.mark.parametrize("rate", EC.RATES)
def test_first_take_after_eviction_equals_unswept_twin(pa, rate):
    """idle_ns >= per: the first Take on a recreated bucket returns the same
    (ok, remaining) as on the bucket that was evicted (the inputs
    tests/test_evict_abi.py pins with the oracle)."""
    freq, per, count = rate
    bs = EC.buckets(rate)
    rows = [(nm, f2b(a), f2b(t), e, c) for nm, a, t, e, c in bs]
    swept, twin = pa.GPURepo(log2_slots=6), pa.GPURepo(log2_slots=6)
    seed(swept, rows)
    seed(twin, rows)
    st, want = sweep(swept, EC.NOW, per)
    assert st["evicted"] == len(rows) and not want
    names = [r[0] for r in rows]
    n = len(names)
    args = (np.zeros(n, np.uint8), names, np.full(n, EC.NOW, np.int64), np.full(n, freq, np.int64),
            np.full(n, per, np.int64), np.full(n, count, np.uint64), np.zeros(n, np.uint64),
            np.zeros(n, np.uint64), np.zeros(n, np.int64))
    got, ref = swept.apply_mixed(*args), twin.apply_mixed(*args)
    assert np.array_equal(got["status"] & 0x7F, ref["status"] & 0x7F)
    assert np.array_equal(got["remaining"], ref["remaining"])
    assert (got["status"] & 0x80).all() and not (ref["status"] & 0x80).any()
    for (nm, a, t, e, c), s, r in zip(bs, ref["status"], ref["remaining"]):
        rem, ok, _ = O.take_fields([a, t, e], c, EC.NOW, freq, per, count)
        assert (int(r), int(s) & 0x7F == 6) == (rem, ok), nm
    swept.close()
    twin.close()


def test_count_only_paths(pa):
    """A dry run, a sweep under min_evict and a sweep with nothing idle read
    the table once and leave every byte of it alone."""
    repo = pa.GPURepo(log2_slots=7, arena_bytes=4096)
    rows = [((b"co-%d" % k) + (b"-and-a-tail-for-the-arena" if k % 3 == 0 else b""), A, T, k,
             T0 if k < 25 else T0 + 100 * SEC) for k in range(60)]
    seed(repo, rows)
    snap = repo.snapshot().tobytes()
    repo.set_timing(True)
    now, idle_ns = T0 + 100 * SEC, 50 * SEC
    used = long_bytes(r[0] for r in rows)
    for kw, idle in ((dict(dry_run=True), 25), (dict(min_evict=26), 25),
                     (dict(dry_run=True, shrink=True), 25), (dict(), 0), (dict(min_evict=0), 0)):
        st = repo.evict_idle(now if idle else T0, idle_ns, **kw)
        assert st == dict(idle=idle, evicted=0, buckets=60, slots=128, arena_used=used,
                          arena_freed=0), kw
        ran = [nm for nm, _ in repo.timings()]
        assert "k_evict_count" in ran and "k_evict_move" not in ran, ran
        assert repo.snapshot().tobytes() == snap
    # min_evict met exactly: the rebuild runs, and 0 means 1
    st = repo.evict_idle(now, idle_ns, min_evict=25)
    ran = [nm for nm, _ in repo.timings()]
    assert st["evicted"] == 25 and "k_evict_count" in ran and "k_evict_move" in ran
    seed(repo, [(b"one-more", A, T, 0, T0)])
    assert repo.evict_idle(now, idle_ns, min_evict=0)["evicted"] == 1
    assert len(repo) == 35
    repo.close()


def shrink_slots(keep, l_open, l_now, pct):
    for l in range(l_open, l_now):
        if keep <= ((1 << l) * pct // 100) // 2:
            return 1 << l
    return 1 << l_now


@pytest.mark.parametrize("pct", [90, 75])
def test_shrink(pa, pct):
    repo = pa.GPURepo(log2_slots=6, arena_bytes=4096, max_load_pct=pct)
    K = 400
    names = [(b"sh-%d" % k) + (b"-long-names-shrink-too-%d" % k if k % 11 == 0 else b"") for k in range(K)]
    seed(repo, [(names[k], f2b(1000.0 + k), f2b(float(k)), 0, T0 + k * SEC) for k in range(K)])
    grown = repo.capacity
    assert grown == (512 if pct == 90 else 1024) and repo.last_stats()[3] > 0
    now = T0 + 1000 * SEC

    def leave(n, **kw):   # buckets k < K - n are idle
        return sweep(repo, now, (1000 - (K - n - 1)) * SEC, **kw)

    st, _ = leave(300)
    assert st["evicted"] == 100 and repo.capacity == grown    # no flag: the slots stay
    lnow = grown.bit_length() - 1
    st, _ = leave(40, shrink=True)
    assert st["slots"] == repo.capacity == shrink_slots(40, 6, lnow, pct) == 128
    st, _ = leave(20, shrink=True)
    assert st["slots"] == repo.capacity == shrink_slots(20, 6, 7, pct) == 64
    st, want = leave(2, shrink=True)
    assert st["slots"] == repo.capacity == 64                  # never below the opening size
    # the table grows again as buckets arrive, and is the oracle's
    o = oracle_of(want)
    more = [b"again-%d" % k for k in range(300)] + names[:50]
    a, t, e = _gen.clean_states(np.random.default_rng(pct), len(more))
    out = repo.receive_soa(more, a, t, e, now)
    ref = o.receive_soa(more, a, t, e, now)
    assert np.array_equal(out["status"], ref[0]) and (out["status"] & 0x80).all()
    assert repo.capacity == grown // (1 if pct == 90 else 2)
    assert_same_dump(gpu_dump(repo), o.dump())
    repo.close()


def test_snapshot_round_trip(pa):
    repo = pa.GPURepo(log2_slots=6, arena_bytes=2048)
    K = 300
    names = [(b"sn-%d" % k) + (b"-a-name-kept-in-the-long-name-arena" if k % 4 == 0 else b"")
             for k in range(K)]
    seed(repo, [(names[k], f2b(7.0 + k), f2b(1.0), 0, T0 + k * SEC) for k in range(K)])
    assert repo.capacity == 512
    st, want = sweep(repo, T0 + 1000 * SEC, (1000 - 249) * SEC, shrink=True)
    assert st["buckets"] == 50 and st["slots"] == 128
    img = repo.snapshot()
    assert img.size == 64 + 128 * 64 + st["arena_used"]
    twin = pa.GPURepo(log2_slots=7, arena_bytes=2048)
    twin.restore(img)
    assert_same_dump(gpu_dump(twin), want)
    for nm in names[250::7] + names[:20:3]:
        got = twin.get(nm)
        assert (got is not None) == (nm in want)
        if got is not None:
            assert (got.added, got.taken, got.elapsed, got.created) == want[nm]
    assert twin.snapshot().tobytes() == img.tobytes()
    repo.close()
    twin.close()


def test_queued_batch_is_finished_first(pa):
    """A PHIP_RECV_ASYNC batch still queued when the sweep is called: its
    statuses are final afterwards and the sweep judged the buckets on the
    elapsed its merges left."""
    import torch
    rng = np.random.default_rng(21)
    K, n = 900, 1 << 16
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    e[:] = 0
    repo = pa.GPURepo(log2_slots=12)
    repo.seed(names, a, t, e, np.full(K, T0, np.int64))
    o = O.Repo()
    o.seed(names, a, t, e, np.full(K, T0, np.int64))
    ids = _gen.zipf_ids(rng, n, 1000)
    ba, bt, be = _gen.clean_states(rng, n)     # elapsed up to 2^40 ns, about 1100 s
    bn = _gen.key_names(ids)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in bn])
    dev = torch.device("cuda", 0)
    tb = torch.from_numpy(np.frombuffer(b"".join(bn) + b"\0" * 8, np.uint8).copy()).to(dev)
    to = torch.from_numpy(offs.astype(np.int32)).to(dev)
    ta, tt, te = (torch.from_numpy(x.view(np.int64).copy()).to(dev) for x in (ba, bt, be))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    repo.receive_soa(tb, ta, tt, te, T0, name_offs=to, n=n, status=status, device=True, queue=True)
    now, idle_ns = T0 + 600 * SEC, 100 * SEC
    st = repo.evict_idle(now, idle_ns)             # no flush in between
    rs = o.receive_soa(bn, ba, bt, be, T0)[0]
    assert np.array_equal(status.cpu().numpy(), rs)
    merged = o.dump()
    want = survivors(merged, now, idle_ns)
    touched = set(bn)
    assert any(k in want for k in touched) and any(k not in want for k in touched)
    assert all(k not in want for k in names if k not in touched)   # (judged on elapsed 0)
    assert st["idle"] == st["evicted"] == len(merged) - len(want) and st["buckets"] == len(want)
    assert_same_dump(gpu_dump(repo), want)
    repo.close()


def test_batcher_takes_while_sweeping(pa):
    """Take threads on 50 names through the batcher while the main thread
    sweeps twice: no errors, and every request is explained by the requests
    in seq order against a model in which a swept name restarts, the `created`
    flag of its take_reply marking the restart."""
    threads, per_thread, K = 8, 120, 50
    repo = pa.GPURepo(log2_slots=8)
    b = pa.TakeBatcher(repo, window_us=50)
    rng = np.random.default_rng(31)
    plan = []
    for tid in range(threads):
        ids = rng.integers(0, K, per_thread)
        now = T0 + np.sort(rng.integers(0, 5 * SEC, per_thread))
        freq = rng.choice(np.array([100, 5], np.int64), per_thread)
        cnt = rng.integers(1, 4, per_thread)
        plan.append([(b"bt-%d" % ids[k], int(now[k]), int(freq[k]), SEC, int(cnt[k]))
                     for k in range(per_thread)])
    results = [[] for _ in range(threads)]
    errors = []
    marks = [threading.Event(), threading.Event()]
    go_on = [threading.Event(), threading.Event()]

    def worker(tid):
        try:
            for k, req in enumerate(plan[tid]):
                if tid == 0 and k in (40, 80):   # the sweeps fall in the middle of the load
                    marks[k // 40 - 1].set()
                    go_on[k // 40 - 1].wait()
                results[tid].append((b.take_reply(*req), req))
        except Exception as ex:   # noqa: BLE001
            errors.append(ex)
            for ev in marks:
                ev.set()

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for th in ts:
        th.start()
    sts = []
    try:
        for k in range(2):
            marks[k].wait()
            sts.append(repo.evict_idle(T0 + 1000 * SEC, SEC))   # everything present is idle
            go_on[k].set()
    finally:
        for ev in go_on:
            ev.set()
        for th in ts:
            th.join()
    assert all(st["evicted"] == st["idle"] > 0 for st in sts), sts
    evicted = sum(st["evicted"] for st in sts)
    assert not errors, errors
    assert b.stats()["errors"] == 0
    b.close()
    allr = sorted((r["seq"], r, req) for rs in results for r, req in rs)
    n = threads * per_thread
    assert [x[0] for x in allr] == list(range(n))
    model = {}
    ncreated = 0
    for _, r, (nm, now, freq, per, cnt) in allr:
        if r["created"]:
            model[nm] = ([0.0, 0.0, 0], now)
            ncreated += 1
        assert nm in model, nm
        state, created = model[nm]
        rem, ok, _ = O.take_fields(state, created, now, freq, per, cnt)
        assert (r["remaining"], r["ok"]) == (rem, ok), (nm, r["seq"])
        assert (r["state"].added, r["state"].taken, r["state"].elapsed, r["state"].created) == \
            (f2b(state[0]), f2b(state[1]), state[2], created)
    final = gpu_dump(repo)
    assert ncreated > K >= len(final)                 # names restarted
    assert len(final) == ncreated - evicted           # every creation is still there or was swept
    for nm, v in final.items():
        state, created = model[nm]
        assert v == (f2b(state[0]), f2b(state[1]), state[2], created), nm
    repo.close()


def test_group_evict_idle(pa):
    """Two shards on one GPU: each sweeps its own table, with no exchange."""
    import torch
    from patrol_amd.engine import names_blob
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(41)
    world = 2
    g = pa.GPUGroup.open_all([0] * world, log2_slots=10)
    o = O.Repo()
    batches, host = [], []
    for _ in range(world):
        n = 3000
        ids = _gen.zipf_ids(rng, n, 600)
        names = [(b"a-group-bucket-with-a-long-name-%d" % i) if i % 9 == 0 else b"g%d" % i for i in ids]
        a, t, e = _gen.clean_states(rng, n)
        blob, offs = names_blob(names)
        batches.append([torch.from_numpy(blob).to(dev), torch.from_numpy(offs.view(np.int32)).to(dev)] +
                       [torch.from_numpy(x.view(np.int64)).to(dev) for x in (a, t, e)])
        host.append((names, a, t, e))
    torch.cuda.synchronize()
    g.receive(batches, T0)
    for names, a, t, e in host:
        o.receive_soa(names, a, t, e, T0)
    merged = o.dump()
    now, idle_ns = T0 + 1000 * SEC, 300 * SEC
    want = survivors(merged, now, idle_ns)
    assert 0 < len(want) < len(merged)

    def owner(nm):
        return ((G.fnv1a64(nm) >> 32) * world) >> 32

    dry = g.evict_idle(now, idle_ns, dry_run=True)
    assert sum(s["idle"] for s in dry) == len(merged) - len(want)
    assert all(s["evicted"] == 0 for s in dry)
    sts = g.evict_idle(now, idle_ns, shrink=True)
    assert len(sts) == world
    assert sum(s["evicted"] for s in sts) == len(merged) - len(want)
    for r, repo in enumerate(g.repos):
        share = {k: v for k, v in want.items() if owner(k) == r}
        assert sts[r]["buckets"] == len(share) > 0
        assert sts[r]["evicted"] == sum(1 for k in merged if owner(k) == r) - len(share)
        assert sts[r]["arena_used"] == long_bytes(share)
        assert_same_dump(gpu_dump(repo), share)
    with pytest.raises(pa.PatrolHipError) as e:
        g.evict_idle(now, 0)
    assert e.value.code == -1
    g.close()
