"""The kept hot directory and the gated queue order of optimistic Receive
passes (phip_engine.hip keep_take / keep_collect, phip_kernels.hpp
k_receive_fast's `gate`).

A handle keeps the directory built last for later optimistic passes while two
consecutive builds selected the same buckets, the fraction of messages folded
holds, the directory is younger than 32 passes and no record has moved; such
a pass launches no k_hot_dir.  A queued optimistic pass goes on the stream
before the batch in front of it is settled, its kernel gated on that batch's
counters: shut, it writes nothing and is queued again.

Observables: GPURepo.last_stats() -- [0:3] directory entries, messages
folded, misses; [7] the passes the batch's directory served before it (0:
built for it); [8] 1 when the batch's first optimistic kernel found its gate
shut -- and the kernels that ran (set_timing / timings()).  last_stats()
finishes a queued batch, so a loop that reads it after every batch never has a
batch pending: the queued cases read it where they say.  Every case compares
statuses and the whole table dump with the oracle.

Shapes: test_hot_directory's -- 2^17 slots, 4000 seeded buckets, batches of
2^16 (the smallest with a directory) to 2^17 messages.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import _evict_cases as EC
from tests import _gen
from tests.test_hot_directory import K, expect, hot_cold_ids, same_table, seeded
from tests.test_receive_optimistic import (Batch, check, classified, dump, kernels, outputs,
                                           raising_states)

gpu = pytest.mark.gpu

SEC = 10**9
N = 1 << 17
KEEP_PASSES = 32
ST_MERGED, ST_CREATED = 1, 0x80   # (CREATED: a flag on the op's status)


def n_created(st):
    return int(((st & ST_CREATED) != 0).sum())


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def batch(rng, ids, step):
    return Batch(ids, *raising_states(rng, len(ids), step), _gen.T0 + step * SEC)


@gpu
@pytest.mark.parametrize("mode", ["sync", "queued", "queued_read"])
def test_kept_on_identical_names(pa, mode):
    """Eight batches naming the same ids with rising states.  The first build
    has nothing to agree with, the second agrees with it: synchronously the
    third batch on takes the kept directory (k_hot_dir twice), queued the
    fourth on (batch 3 is begun before batch 2 is collected: three times).
    The directory is the same set, so entries and hits are numpy's for every
    batch.  queued_read reads the stats after every batch, which finishes it:
    the decisions are the synchronous ones."""
    rng = np.random.default_rng(901)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    ids = _gen.zipf_ids(rng, N, K)
    want = expect(ids)[:2] + (0,)
    g.set_timing(True, accumulate=True)
    done, ages = [], []
    for step in range(1, 9):
        b = batch(rng, ids, step)
        done.append((b.run(g, mode != "sync"), b.oracle(o)))
        if mode != "queued":
            stats = g.last_stats()
            assert stats[:3] == want, (step, stats, want)
            assert stats[8] == 0
            ages.append(stats[7])
    g.flush()
    stats = g.last_stats()
    assert stats[:3] == want and stats[8] == 0, (stats, want)
    ran = kernels(g)
    print(mode, "k_hot_dir launches", ran.count("k_hot_dir"), "ages", ages, "last", stats[7])
    if mode == "queued":
        assert ran.count("k_hot_dir") == 3, ran
        assert stats[7] == 5, stats          # 0, 0, 0, 1, 2, 3, 4, 5
    else:
        assert ran.count("k_hot_dir") == 2, ran
        assert ages == [0, 0, 1, 2, 3, 4, 5, 6], ages
    assert ran.count("k_receive_fast") == 8 and not classified(ran) and "k_undo" not in ran, ran
    for d, ref in done:
        check(d, ref)
    same_table(g, o)
    g.close()


@gpu
@pytest.mark.parametrize("first_b", ["quiet", "raising"])
def test_hot_set_moves(pa, first_b):
    """Hot sets A x 4 then B x 4.  The first B batch runs on A's directory,
    which folds next to nothing of it, and is still exact.
    quiet: its states raise next to nothing, so its pass stands; the policy has
    then seen its hit fraction and the next batch builds, the one after agrees,
    the last is served by B's directory.
    raising: every message of a B bucket now takes the table path and finds
    its record below it, a wave logs all 64 of them and overflows its region:
    the pass is undone and the batch run again classified, with a directory of
    its own.  The overflow is the stale directory's, so the handle does not
    back off: the next batch is optimistic again, agrees with that directory,
    and the last two are served.
    Either way the last batch's entries and hits are those of its own ids."""
    rng = np.random.default_rng(902)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    g.set_timing(True, accumulate=True)
    done, ages, hits = [], [], []
    for step in range(1, 9):
        ids = hot_cold_ids(rng, N, 0 if step <= 4 else 1000)
        b = batch(rng, ids, step)
        if step == 5 and first_b == "quiet":
            b.a[:], b.t[:], b.e[:] = np.float64(2.0).view(np.uint64), np.float64(1.0).view(np.uint64), 1
        done.append((b.run(g), b.oracle(o)))
        stats = g.last_stats()
        ages.append(stats[7])
        hits.append(stats[1])
        assert stats[2] == 0 and stats[8] == 0, stats
    want = expect(ids)
    ran = kernels(g)
    print(first_b, "ages", ages, "hits", hits)
    if first_b == "quiet":
        assert ages == [0, 0, 1, 2, 3, 0, 0, 1], ages
        assert hits[4] < hits[3] // 8            # A's directory under B's batch
        assert "k_undo" not in ran and not classified(ran), ran
    else:
        assert ages == [0, 0, 1, 2, 0, 0, 1, 2], ages
        assert ran.count("k_undo") == 1 and sum(nm.startswith("k_classify") for nm in ran) == 1, ran
    assert stats[:3] == want[:2] + (0,), (stats, want[:2])
    assert ran.count("k_hot_dir") == 4, ran
    for d, ref in done:
        check(d, ref)
    same_table(g, o)
    g.close()


@gpu
def test_age_bound(pa):
    """40 batches of 2^16 naming the same ids: the directory built for batch 2
    serves 32 passes (its own included), batch 34 builds again, and since that
    build agrees with the directory before it, batch 35 is served at once."""
    rng = np.random.default_rng(903)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    n = 1 << 16
    ids = _gen.zipf_ids(rng, n, K)
    want = expect(ids)[:2] + (0,)
    g.set_timing(True, accumulate=True)
    ages = []
    b = batch(rng, ids, 0)                       # (the names once: 40 batches of them)
    for step in range(1, 41):
        b.a, b.t, b.e = raising_states(rng, n, step)
        b.now = _gen.T0 + step * SEC
        last = (b.run(g), b.oracle(o))
        stats = g.last_stats()
        assert stats[:3] == want, (step, stats, want)
        ages.append(stats[7])
        if step in (1, 33, 34, 40):
            check(*last)
    assert ages == [0, 0] + list(range(1, KEEP_PASSES)) + [0] + list(range(1, 7)), ages
    assert kernels(g).count("k_hot_dir") == 3
    same_table(g, o)
    g.close()


def oracle_of(d):
    o = O.Repo()
    ks = list(d)
    o.seed(ks, [d[k][0] for k in ks], [d[k][1] for k in ks], [d[k][2] for k in ks],
           [d[k][3] for k in ks])
    return o


@gpu
def test_eviction_under_a_kept_directory(pa):
    """After a pass served by a kept directory, phip_evict_idle drops every
    bucket the batches named (the hot ones with them) and moves the rest, which
    were created at the sweep's `now`.  The next batch names the evicted hot
    buckets again: its pass builds ([7] == 0, the records moved), the buckets
    are created anew and the statuses, CREATED included, and the table are
    exact."""
    rng = np.random.default_rng(904)
    now, idle_ns = EC.NOW + 20 * (1 << 40), EC.dts(SEC)[0]
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    created = _gen.T0 - rng.integers(0, SEC, K)
    created[3000:] = now                          # never named below, never idle
    g = pa.GPURepo(log2_slots=17, isolate=False)
    o = O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)

    def ids_of():
        ids = hot_cold_ids(rng, N, 0)
        cold = ids >= 2000
        ids[cold] = 2000 + ids[cold] % 1000       # cold buckets of [2000, 3000)
        return ids

    done, ages = [], []
    for step in (1, 2, 3):
        b = batch(rng, ids_of(), step)
        done.append((b.run(g), b.oracle(o)))
        ages.append(g.last_stats()[7])
    assert ages == [0, 0, 1], ages
    for d, ref in done:
        check(d, ref)
    same_table(g, o)
    before = dump(g)
    st = g.evict_idle(now, idle_ns)
    left = {k: v for k, v in before.items() if v[3] == now}
    assert st["evicted"] == K - 1000 and len(left) == 1000, st
    assert not any(b"b%d" % i in left for i in range(50))
    o = oracle_of(left)
    ages = []
    for step in (4, 5, 6):
        b = Batch(ids_of(), *raising_states(rng, N, step), now + step * SEC)
        d, ref = b.run(g), b.oracle(o)
        stats = g.last_stats()
        ages.append(stats[7])
        if step == 4:
            # (every bucket it names is gone: more than 2^16 misses, so a
            # nested pass merged it and the miss count read is that pass's)
            assert n_created(ref[0]) > 50
        check(d, ref)
    assert ages == [0, 0, 1], ages               # built (the records moved), built, kept
    same_table(g, o)
    g.close()


@gpu
def test_growth_under_a_kept_directory(pa):
    """A handle of 2^13 slots that may grow: between two passes served by a
    kept directory comes a batch with enough new names to rehash the table.
    That batch itself still runs on the kept directory (its slots are the
    table's until the inserts grow it); the pass after it builds."""
    rng = np.random.default_rng(905)
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    created = _gen.T0 - rng.integers(0, SEC, K)
    g = pa.GPURepo(log2_slots=13, isolate=False)
    o = O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)
    n = 1 << 16
    ages, grows = [], []
    for step in range(1, 8):
        ids = hot_cold_ids(rng, n, 0)
        if step == 4:
            new = rng.choice(n, 4000, replace=False)
            ids[new] = K + np.arange(4000)
        b = batch(rng, ids, step)
        d, ref = b.run(g), b.oracle(o)
        stats = g.last_stats()
        ages.append(stats[7])
        grows.append(stats[3])
        check(d, ref)
    print("ages", ages, "growths", grows)
    assert grows[2] == 0 and grows[3] > 0
    assert ages == [0, 0, 1, 2, 0, 0, 1], ages
    same_table(g, o)
    g.close()


def pair(pa, rng):
    """The seeded buckets on an optimistic handle, a classify_first one and in
    the oracle."""
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    created = _gen.T0 - rng.integers(0, SEC, K)
    go = pa.GPURepo(log2_slots=17, isolate=False)
    gc = pa.GPURepo(log2_slots=17, isolate=False, classify_first=True)
    o = O.Repo()
    for r in (go, gc, o):
        r.seed(names, a, t, e, created)
    return go, gc, o


def same_tables(go, gc, o):
    same_table(go, o)
    same_table(gc, o)


@gpu
@pytest.mark.parametrize("at", ["last", "first"])
def test_gate_keeps_the_order(pa, at):
    """Queued batches 0 (clean), j and j+1: j's dirty message is an incast on
    a bucket that j+1 raises.  j+1's kernel is on the stream before the host
    has read j's counters; its gate is shut, so j is undone and run again in
    order first: the incast's reply carries the state without any of j+1's
    merges, and both tables are the classify_first handle's and the oracle's."""
    rng = np.random.default_rng(906)
    go, gc, o = pair(pa, rng)
    go.set_timing(True, accumulate=True)
    b0 = batch(rng, _gen.zipf_ids(rng, N, K), 1)
    ids = _gen.zipf_ids(rng, N, K)
    k = N - 1 if at == "last" else 0
    bucket = int(np.bincount(ids).argmax())
    ids[k] = bucket
    bj = batch(rng, ids, 2)
    bj.a[k], bj.t[k], bj.e[k] = 0, 0, 0
    ids1 = _gen.zipf_ids(rng, N, K)
    ids1[7] = bucket
    bj1 = batch(rng, ids1, 3)
    done = []
    for b in (b0, bj, bj1):
        done.append((b.run(go, True), b.run(gc, True), b.oracle(o)))
        if b is bj:
            pass                                   # (no read here: j stays pending)
    stats = go.last_stats()                        # finishes j+1
    assert stats[8] == 1, stats
    assert gc.last_stats()[8] == 0
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    st, ra, _, _ = done[1][2]
    assert (st[k] & 0x7F) == 2                     # the incast, answered
    assert outputs(done[1][0])[1][k] == ra[k]
    ran = kernels(go)
    assert "k_undo" in ran and classified(ran), ran
    same_tables(go, gc, o)
    go.close()
    gc.close()


@gpu
def test_gate_shut_by_misses(pa):
    """j names 300 new buckets, j+1 names the same ones: j's inserts come
    first, so CREATED goes to j's first message of each and j+1 finds them.
    The miss path moves no policy: the batch after runs optimistically."""
    rng = np.random.default_rng(907)
    go, gc, o = pair(pa, rng)
    go.set_timing(True, accumulate=True)
    done = []
    for step, extra in ((1, 0), (2, 300), (3, 300), (4, 0)):
        ids = _gen.zipf_ids(rng, N, K)
        if extra:
            ids[rng.choice(N, 3 * extra, replace=False)] = K + np.arange(3 * extra) % extra
        b = batch(rng, ids, step)
        done.append((b.run(go, True), b.run(gc, True), b.oracle(o)))
        if step == 3:
            stats = go.last_stats()                # finishes j+1
            assert stats[8] == 1 and stats[2] == 0, stats
    go.flush()
    gc.flush()
    assert go.last_stats()[8] == 0
    assert n_created(done[1][2][0]) == 300 and n_created(done[2][2][0]) == 0
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    ran = kernels(go)
    assert not classified(ran) and "k_undo" not in ran, ran
    assert ran.count("k_receive_fast") == 5, ran   # j+1 twice: the gated launch returned at once
    same_tables(go, gc, o)
    go.close()
    gc.close()


@gpu
def test_gate_shut_by_log_overflow(pa):
    """j is test_log_overflow's batch (every cold message logs, the wave
    regions overflow), j+1 is clean: the gate is shut, j is undone and run
    again, and the handle classifies first from then on, j+1 included."""
    rng = np.random.default_rng(908)
    go, gc, o = pair(pa, rng)
    go.set_timing(True, accumulate=True)
    b0 = batch(rng, _gen.zipf_ids(rng, N, K), 1)
    up = np.arange(N, dtype=np.float64)
    bj = Batch(rng.integers(0, K, N), (3e7 + up + 0.5).view(np.uint64).copy(),
               (3e7 + up).view(np.uint64).copy(), (1 << 44) + np.arange(N, dtype=np.int64),
               _gen.T0 + 2 * SEC)
    bj1 = batch(rng, _gen.zipf_ids(rng, N, K), 40)
    done = [(b.run(go, True), b.run(gc, True), b.oracle(o)) for b in (b0, bj, bj1)]
    stats = go.last_stats()                        # finishes j+1
    assert stats[8] == 1, stats
    ran = kernels(go)
    assert ran.count("k_undo") == 1 and sum(nm.startswith("k_classify") for nm in ran) == 2, ran
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    same_tables(go, gc, o)
    go.close()
    gc.close()


@gpu
def test_gate_open(pa):
    """Twelve clean queued batches: every gate is open -- each fast kernel
    runs once, nothing is undone or classified -- and three builds serve them
    all."""
    rng = np.random.default_rng(909)
    go, gc, o = pair(pa, rng)
    go.set_timing(True, accumulate=True)
    ids = _gen.zipf_ids(rng, N, K)
    done = []
    for step in range(1, 13):
        b = batch(rng, ids, step)
        done.append((b.run(go, True), b.run(gc, True), b.oracle(o)))
    go.flush()
    gc.flush()
    stats = go.last_stats()
    assert stats[8] == 0 and stats[7] == 9 and stats[:3] == expect(ids)[:2] + (0,), stats
    ran = kernels(go)
    assert ran.count("k_receive_fast") == 12 and ran.count("k_hot_dir") == 3, ran
    assert not classified(ran) and "k_undo" not in ran, ran
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    same_tables(go, gc, o)
    go.close()
    gc.close()


@gpu
@pytest.mark.parametrize("off", [65, 64], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("queue", [False, True])
def test_status_column_of_a_pass_without_a_build(pa, queue, off):
    """n = 2^16 + 65 (a tail chunk of one message), the status column one byte
    into its allocation (or, aligned, at its start), 64 guard bytes on either
    side: the pass that takes the kept directory fills exactly the column with
    MERGED."""
    import torch
    rng = np.random.default_rng(910)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    n = (1 << 16) + 65
    ids = _gen.zipf_ids(rng, n, K)
    dev = torch.device("cuda", 0)
    keep = []
    for step in (1, 2, 3, 4):
        b = batch(rng, ids, step)
        d = b.device()
        buf = torch.full((1 + 64 + n + 64,), 0xAB, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        status = buf[off:off + n]
        g.receive_soa(d["tb"], d["ta"], d["tt"], d["te"], b.now, name_offs=d["to"], n=n,
                      status=status, device=True, queue=queue)
        keep.append((d, buf, b.oracle(o)))
    g.flush()
    assert g.last_stats()[7] >= 1                  # no build for the last batch
    for d, buf, ref in keep:
        got = buf.cpu().numpy()
        assert (got[:off] == 0xAB).all() and (got[off + n:] == 0xAB).all()
        assert np.array_equal(got[off:off + n], ref[0]) and (ref[0] == ST_MERGED).all()
    same_table(g, o)
    g.close()
