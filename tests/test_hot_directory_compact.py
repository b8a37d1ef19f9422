"""The compact layouts of a kept hot directory (phip_kernels.hpp HotCompact,
k_receive_fast's NW; phip_engine.hip keep_take).

k_hot_dir's last workgroup selects, beside the directory of the 736 rule, an
extended set: the lowest threshold t >= 8 with at most 1472 buckets sampled t
or more times, ordered by descending sample count, the 736 rule's set first.
A built pass loads the first set as ever.  A pass that takes the kept
directory holds it in the layout the build's longest selected name allows:
two name words an entry and up to 1472 entries (names <= 14 bytes), three
words and the first 1216 (<= 22 bytes), or today's layout and the first set.

Observables as in test_hot_directory_kept: last_stats() [0:3] entries loaded,
messages folded, misses; [7] the directory's age; and the kernels that ran.
Entries and hits are recomputed in numpy with the cap as a parameter; every
case compares statuses and the whole table dump with the oracle.

Shapes: test_hot_directory's 2^17 slots and 4000 seeded buckets; batches of
2^20 messages (16,384 samples at stride 64: the smallest at which more than
736, and more than 1472, buckets can each be sampled 8 times) and 2^20 + 65.
Unsampled positions name cold buckets of [2000, K) whose states mostly raise
nothing (every cold message that raises its record takes a log entry, and a
wave's region holds 88 for its 128 messages), one in eight of them raising.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests import _evict_cases as EC
from tests import _gen
from tests.test_hot_directory import K, MIN_COUNT, STRIDE, NamedBatch, same_table
from tests.test_receive_optimistic import check, classified, dump, kernels, raising_states

gpu = pytest.mark.gpu

SEC = 10**9
N = 1 << 20
NEG0 = np.uint64(0x8000000000000000)
HOT_MAX, HOT_MAX_EXT, HOT_MAX3, HOT_IDX, HOT_LDS = 736, 1472, 1216, 8192, 4096
SHORT_NAME, INLINE_NAME = 14, 22
LDS_BUDGET = 81920


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def expect(ids, cap, take=None):
    """(entries, hits, selected ids) of a batch naming bucket ids[i] in message
    i under the "at most cap" rule; take: only the first `take` of them by
    descending sample count (the count class the cut falls in must fold the
    same number of messages whichever of its buckets are taken)."""
    cnt = np.bincount(ids[::STRIDE])
    t = MIN_COUNT
    while (cnt >= t).sum() > cap:
        t += 1
    sel = np.nonzero(cnt >= t)[0]
    if take is not None and len(sel) > take:
        sel = sel[np.argsort(-cnt[sel], kind="stable")]
        tie = sel[cnt[sel] == cnt[sel[take - 1]]]
        assert len(set(np.bincount(ids, minlength=len(cnt))[tie].tolist())) == 1
        sel = sel[:take]
    return len(sel), int(np.isin(ids, sel).sum()), sel


def tier_ids(rng, n, shape="two_tiers"):
    """two_tiers: samples j < 9800 name j % 700 (14 each), the other 6584 name
    700 + j % 700 (9 or 10 each).  over_cap: 500 buckets x 12 samples, then
    1100 buckets sharing the other 10,384 (9 each, 484 of them 10)."""
    ids = rng.integers(2000, K, n)
    ns = (n + STRIDE - 1) // STRIDE
    j = np.arange(ns)
    if shape == "two_tiers":
        ids[::STRIDE] = np.where(j < 9800, j % 700, 700 + j % 700)
    else:
        ids[::STRIDE] = np.where(j < 6000, j % 500, 500 + (j - 6000) % 1100)
    return ids


def states(rng, ids, step):
    """Rising states (each batch raises what it names) for the hot messages
    and one cold message in eight; the other cold messages raise nothing."""
    a, t, e = raising_states(rng, len(ids), step)
    quiet = (ids >= 2000) & (rng.random(len(ids)) < 0.875)
    a[quiet] = np.float64(2.0).view(np.uint64)
    t[quiet] = np.float64(1.0).view(np.uint64)
    e[quiet] = 1
    return a, t, e


def seeded(pa, rng, names):
    a, t, e = _gen.clean_states(rng, len(names))
    created = _gen.T0 - rng.integers(0, SEC, len(names))
    g = pa.GPURepo(log2_slots=17, isolate=False)
    o = O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)
    return g, o


class Steps:
    """One batch of names run step after step with new states."""

    def __init__(self, pa, rng, names, ids):
        self.rng, self.ids = rng, ids
        self.g, self.o = seeded(pa, rng, names)
        self.g.set_timing(True, accumulate=True)
        self.b = NamedBatch([names[i] for i in ids], None, None, None, 0)
        self.ran = 0

    def run(self, step, queue=False, edit=None):
        b = self.b
        b.a, b.t, b.e = states(self.rng, self.ids, step)
        if edit:
            edit(b)
        b.now = _gen.T0 + step * SEC
        return b.run(self.g, queue), b.oracle(self.o)

    def new_kernels(self):
        ran = kernels(self.g)
        new, self.ran = ran[self.ran:], len(ran)
        return new

    def close(self):
        same_table(self.g, self.o)
        self.g.close()


def built_and_kept(s, built, kept, first_kept=3):
    """Synchronous batches 1..first_kept: the builds report `built`, the kept
    pass `kept` (entries, hits), launches no k_hot_dir and stands."""
    for step in range(1, first_kept + 1):
        d, ref = s.run(step)
        stats = s.g.last_stats()
        new = s.new_kernels()
        want = kept if step == first_kept else built
        print("step", step, "stats", stats[:3], "age", stats[7], "want", want[:2])
        assert stats[:3] == want[:2] + (0,), (step, stats, want[:2])
        assert stats[7] == (1 if step == first_kept else 0), (step, stats)
        assert new.count("k_hot_dir") == (0 if step == first_kept else 1), new
        assert new.count("k_receive_fast") == 1 and "k_undo" not in new and not classified(new), new
        check(d, ref)


@gpu
@pytest.mark.parametrize("n", [N, N + 65], ids=["2^20", "off_tile"])
def test_two_tiers(pa, n):
    """By hand: the 736 rule gives 700 (t = 11), the extended rule 1400
    (t = 8).  Batches 1-2 build and report 700; batch 3 takes the kept
    directory in the two-word layout and reports 1400 entries and numpy's hits
    for that set."""
    rng = np.random.default_rng(1201)
    ids = tier_ids(rng, n)
    built, kept = expect(ids, HOT_MAX), expect(ids, HOT_MAX_EXT)
    assert built[0] == 700 and kept[0] == 1400 and kept[1] > built[1]
    s = Steps(pa, rng, _gen.key_names(np.arange(K)), ids)
    built_and_kept(s, built, kept)
    s.close()


@gpu
def test_two_tiers_queued(pa):
    """Queued, batch 3 is begun before batch 2 is collected: three builds, and
    batches 4 and 5 take the kept directory (1400 entries)."""
    rng = np.random.default_rng(1202)
    ids = tier_ids(rng, N)
    kept = expect(ids, HOT_MAX_EXT)
    s = Steps(pa, rng, _gen.key_names(np.arange(K)), ids)
    done = [s.run(step, queue=True) for step in range(1, 6)]
    s.g.flush()
    stats = s.g.last_stats()
    ran = s.new_kernels()
    assert stats[:3] == kept[:2] + (0,) and stats[7] == 2 and stats[8] == 0, (stats, kept[:2])
    assert ran.count("k_hot_dir") == 3 and ran.count("k_receive_fast") == 5, ran
    assert "k_undo" not in ran and not classified(ran), ran
    for d, ref in done:
        check(d, ref)
    s.close()


@gpu
def test_over_cap(pa):
    """By hand: the 736 rule gives 500 (t = 11), the extended rule 984
    (t = 10: 1600 > 1472 at t = 8 and t = 9)."""
    rng = np.random.default_rng(1203)
    ids = tier_ids(rng, N, "over_cap")
    built, kept = expect(ids, HOT_MAX), expect(ids, HOT_MAX_EXT)
    assert built[0] == 500 and kept[0] == 984
    s = Steps(pa, rng, _gen.key_names(np.arange(K)), ids)
    built_and_kept(s, built, kept)
    s.close()


@gpu
def test_flush_beyond_reserve(pa):
    """two_tiers, every batch raising every hot bucket; in the kept batch the
    unsampled messages name the 1400 hot buckets too (message i: i % 1400), so
    a workgroup's 2048 messages raise more than 1024 of them and the waves that
    flush two entries a lane log past the 64 entries reserved for the flush,
    into what the loop left of their regions.  The pass stands and the table
    equals the oracle."""
    rng = np.random.default_rng(1204)
    ids = tier_ids(rng, N)
    built = expect(ids, HOT_MAX)
    names = _gen.key_names(np.arange(K))
    s = Steps(pa, rng, names, ids)
    for step in (1, 2):
        d, ref = s.run(step)
        assert s.g.last_stats()[:3] == built[:2] + (0,)
        check(d, ref)
    dense = np.arange(N) % 1400
    dense[::STRIDE] = ids[::STRIDE]
    s.ids, s.b = dense, NamedBatch([names[i] for i in dense], None, None, None, 0)
    s.new_kernels()
    d, ref = s.run(3)
    stats, new = s.g.last_stats(), s.new_kernels()
    print("stats", stats)
    assert stats[:3] == (1400, N, 0) and stats[7] == 1, stats
    # (no overflow; the workgroup that flushes first finds every record it
    # names below its maxima and logs them all, later ones only what they
    # still raise: the total depends on their order)
    assert stats[6] == 0 and stats[5] > 1024, stats
    assert "k_hot_dir" not in new and "k_undo" not in new and not classified(new), new
    check(d, ref)
    s.close()


@gpu
def test_undo_of_a_compact_pass(pa):
    """One -0.0 `added` on a first-tier bucket in the first kept batch of
    two_tiers: the pass, flush included, is undone (k_undo once) and the batch
    run again classified; table and statuses equal the oracle."""
    rng = np.random.default_rng(1205)
    ids = tier_ids(rng, N)
    s = Steps(pa, rng, _gen.key_names(np.arange(K)), ids)
    for step in (1, 2):
        check(*s.run(step))
    s.new_kernels()
    at = STRIDE * 5000
    assert ids[at] < 700

    def negzero(b):
        b.a[at] = NEG0

    d, ref = s.run(3, edit=negzero)
    new = s.new_kernels()
    assert new.count("k_undo") == 1 and classified(new) and new.count("k_receive_fast") == 2, new
    check(d, ref)
    s.close()


@gpu
@pytest.mark.parametrize("length", [15, 32])
def test_long_name_in_extension(pa, length):
    """One name of 15 or 32 bytes among the second tier (bucket 900, sampled
    10 times).  15: the kept pass takes the three-word layout and the first
    min(n_ext, 1216) entries by descending count, the long name among them.
    32: today's layout and the first 700."""
    rng = np.random.default_rng(1206)
    ids = tier_ids(rng, N)
    names = _gen.key_names(np.arange(K))
    names[900] = (b"h%014d" if length == 15 else b"L%031d") % 900
    assert len(names[900]) == length
    built = expect(ids, HOT_MAX)
    kept = expect(ids, HOT_MAX_EXT, HOT_MAX3) if length == 15 else built
    assert kept[0] == (1216 if length == 15 else 700) and (length == 32 or 900 in kept[2])
    s = Steps(pa, rng, names, ids)
    built_and_kept(s, built, kept)
    s.close()


@gpu
def test_names15(pa):
    """Every name 15 bytes, two_tiers' counts: the three-word layout."""
    rng = np.random.default_rng(1207)
    ids = tier_ids(rng, N)
    names = [b"n%014d" % i for i in range(K)]
    built, kept = expect(ids, HOT_MAX), expect(ids, HOT_MAX_EXT, HOT_MAX3)
    assert built[0] == 700 and kept[0] == 1216
    s = Steps(pa, rng, names, ids)
    built_and_kept(s, built, kept)
    s.close()


@gpu
def test_moved_record(pa):
    """After a kept compact pass, phip_evict_idle drops every bucket the
    batches named (test_hot_directory_kept's eviction case at these shapes) and
    moves the rest.  The next pass builds ([7] == 0), the buckets are created
    anew, and the pass after the next build is kept and compact again."""
    rng = np.random.default_rng(1208)
    now, idle_ns = EC.NOW + 20 * (1 << 40), EC.dts(SEC)[0]
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    created = _gen.T0 - rng.integers(0, SEC, K)
    created[3000:] = now                          # never named below, never idle
    g = pa.GPURepo(log2_slots=17, isolate=False)
    o = O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)
    ids = tier_ids(rng, N)
    cold = ids >= 2000
    ids[cold] = 2000 + ids[cold] % 1000           # cold buckets of [2000, 3000)
    kept = expect(ids, HOT_MAX_EXT)
    b = NamedBatch([names[i] for i in ids], None, None, None, 0)

    def run(step, t0):
        b.a, b.t, b.e = states(rng, ids, step)
        b.now = t0 + step * SEC
        return b.run(g), b.oracle(o)

    ages = []
    for step in (1, 2, 3):
        check(*run(step, _gen.T0))
        ages.append(g.last_stats()[7])
    assert ages == [0, 0, 1] and g.last_stats()[:2] == kept[:2], (ages, g.last_stats())
    same_table(g, o)
    before = dump(g)
    st = g.evict_idle(now, idle_ns)
    left = {k: v for k, v in before.items() if v[3] == now}
    assert st["evicted"] == K - 1000 and len(left) == 1000, st
    o = O.Repo()
    ks = list(left)
    o.seed(ks, *([left[k][f] for k in ks] for f in range(4)))
    ages = []
    for step in (4, 5, 6):
        check(*run(step, now))
        ages.append(g.last_stats()[7])
    assert ages == [0, 0, 1] and g.last_stats()[:3] == kept[:2] + (0,), (ages, g.last_stats())
    same_table(g, o)
    g.close()


def test_lds_bytes_of_the_layouts():
    """The three layouts' LDS bytes: today's 4096 32-bit slots and 88 B an
    entry, the compact ones' 8192 16-bit slots and 44 / 52 B an entry; each at
    most half a CU's 160 KiB with the kernel's 12 B of counters.  The constants
    mirrored here are the header's defaults."""
    today = HOT_LDS * 4 + HOT_MAX * (8 * 4 + 8 * 3 + 4 * 2 + 8 * 3)
    two = HOT_IDX * 2 + HOT_MAX_EXT * (2 * 8 + 4 + 3 * 8)
    three = HOT_IDX * 2 + HOT_MAX3 * (3 * 8 + 4 + 3 * 8)
    assert (today, two, three) == (81152, 81152, 79616)
    assert max(today, two, three) + 12 <= LDS_BUDGET
    assert HOT_MAX3 == (two - HOT_IDX * 2) // 52 // 64 * 64      # the largest multiple of 64 that fits
    assert HOT_IDX * 2 + (HOT_MAX3 + 64) * 52 + 12 > LDS_BUDGET
    assert HOT_MAX_EXT + 1 < (1 << 11)                           # entry + 1 in 11 bits of a slot
    src = (Path(__file__).resolve().parent.parent / "patrol_amd" / "csrc" / "phip_kernels.hpp").read_text()
    for name, value in (("PHIP_HOT_MAX", HOT_MAX), ("PHIP_HOT_LDS", HOT_LDS),
                        ("PHIP_HOT_MAX_EXT", HOT_MAX_EXT), ("PHIP_HOT_IDX", HOT_IDX)):
        assert re.search(r"#define %s (\d+)" % name, src).group(1) == str(value), name
    for name, value in (("kShortName", SHORT_NAME), ("kInlineName", INLINE_NAME)):
        dev = (Path(__file__).resolve().parent.parent / "patrol_amd" / "csrc" / "phip_device.hpp").read_text()
        assert re.search(r"constexpr u32 %s = (\d+);" % name, dev).group(1) == str(value), name
