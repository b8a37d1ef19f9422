"""The optimistic Receive pass (phip_kernels.hpp "The optimistic pass"): a
decoded batch of a handle that does not set dirty buckets apart is merged
without classification, every merge logged; a pass that meets a dirty message
or a malformed name entry, or overflows its log, is undone and the batch run
again through the classified path.

Bar: bit-exact statuses, incast replies and full table dumps (created
included) against the oracle, and against a handle opened with
classify_first=True fed the same batches.

Shapes: n = 2^17 messages (just above the 2^16 from which the hot directory
and the persistent grid run), K = 20000 buckets in 2^17 slots.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import _gen

gpu = pytest.mark.gpu

SEC = 10**9
NEG0 = np.uint64(0x8000000000000000)
N = 1 << 17
K = 20000
ERR_INVALID = -1
ST_SHORT, ST_NOT_PROCESSED = 4, 5


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def trio(pa, rng, negative=0.0):
    """K buckets b0..b{K-1} on an optimistic handle, on a classify_first one
    and in the oracle; a fraction `negative` of them (the returned mask) holds
    negative added/taken."""
    names = _gen.key_names(np.arange(K))
    a, t, e = _gen.clean_states(rng, K)
    neg = rng.random(K) < negative
    a[neg] = (-np.abs(a[neg].view(np.float64)) - 1.0).view(np.uint64)
    t[neg] = (-np.abs(t[neg].view(np.float64)) - 2.0).view(np.uint64)
    created = _gen.T0 - rng.integers(0, SEC, K)
    go = pa.GPURepo(log2_slots=17, isolate=False)
    gc = pa.GPURepo(log2_slots=17, isolate=False, classify_first=True)
    o = O.Repo()
    for r in (go, gc, o):
        r.seed(names, a, t, e, created)
    return go, gc, o, neg


def raising_states(rng, n, step):
    """Clean states later than every state of the steps before (as the
    benchmark's batches): each batch raises the buckets it names."""
    taken = rng.integers(0, 10**6, n).astype(np.float64) + step * 2e6
    added = taken + rng.random(n) * 100.0
    elapsed = rng.integers(0, 1 << 40, n, dtype=np.int64) + step * (1 << 40)
    return added.view(np.uint64).copy(), taken.view(np.uint64).copy(), elapsed


class Batch:
    """A batch on the host (names, a, t, e) and, per handle, on the device."""

    def __init__(self, ids, a, t, e, now):
        self.names = _gen.key_names(ids)
        self.a, self.t, self.e, self.now = a, t, e, now
        self.n = len(self.names)
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([len(x) for x in self.names])
        self.offs = offs.astype(np.int32)
        self.blob = np.frombuffer(b"".join(self.names) + b"\0" * 8, np.uint8).copy()

    def device(self):
        import torch
        dev = torch.device("cuda", 0)
        d = dict(tb=torch.from_numpy(self.blob).to(dev), to=torch.from_numpy(self.offs).to(dev),
                 status=torch.zeros(self.n, dtype=torch.uint8, device=dev),
                 reply=torch.zeros((self.n, 4), dtype=torch.int64, device=dev))
        d["ta"], d["tt"], d["te"] = (torch.from_numpy(x.view(np.int64).copy()).to(dev)
                                     for x in (self.a, self.t, self.e))
        return d

    def run(self, g, queue=False):
        d = self.device()
        g.receive_soa(d["tb"], d["ta"], d["tt"], d["te"], self.now, name_offs=d["to"], n=self.n,
                      status=d["status"], device=True, reply=d["reply"], queue=queue)
        return d

    def oracle(self, o):
        return o.receive_soa(self.names, self.a, self.t, self.e, self.now)


def outputs(d):
    r = d["reply"].cpu().numpy()
    return d["status"].cpu().numpy(), r[:, 0].view(np.uint64), r[:, 1].view(np.uint64), r[:, 2]


def check(d, ref, other=None):
    """A device batch's statuses and incast replies against the oracle's (and
    against another handle's outputs for the same batch)."""
    st, ra, rt, re = ref
    gs, ga, gt, ge = outputs(d)
    assert np.array_equal(gs, st), np.nonzero(gs != st)[0][:8]
    rep = (st & 0x7F) == 2
    for got, want in ((ga, ra), (gt, rt), (ge, re)):
        assert np.array_equal(got[rep], want[rep])
    if other is not None:
        os_, oa, ot, oe = outputs(other)
        assert np.array_equal(gs, os_)
        for got, want in ((ga, oa), (gt, ot), (ge, oe)):
            assert np.array_equal(got[rep], want[rep])


def dump(g):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}
    assert len(g) == len(d)
    return d


def same_tables(go, gc, o):
    want = o.dump()
    for g in (go, gc):
        got = dump(g)
        assert len(got) == len(want)
        bad = [k for k in want if got.get(k) != want[k]]
        assert not bad, [(k, got.get(k), want[k]) for k in bad[:5]]


def kernels(g):
    return [nm for nm, _ in g.timings()]


def classified(names_run):
    return any(nm.startswith("k_classify") for nm in names_run)


@gpu
@pytest.mark.parametrize("queue", [False, True])
def test_clean_batches_run_without_classification(pa, queue):
    """Three clean batches back to back, synchronous and queued: the
    optimistic path runs them (k_receive_fast, no k_classify, no k_undo), the
    classify_first handle classifies; same results."""
    rng = np.random.default_rng(701)
    go, gc, o, _ = trio(pa, rng)
    for g in (go, gc):
        g.set_timing(True, accumulate=True)
    done = []
    for step in (1, 2, 3):
        b = Batch(_gen.zipf_ids(rng, N, K), *raising_states(rng, N, step), _gen.T0 + step * SEC)
        done.append((b.run(go, queue), b.run(gc, queue), b.oracle(o)))
    go.flush()
    gc.flush()
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    ran = kernels(go)
    assert ran.count("k_receive_fast") == 3 and not classified(ran) and "k_undo" not in ran, ran
    assert classified(kernels(gc))
    stats = go.last_stats()
    print("undo log of the last batch: %d entries for %d messages, %d overflowed" % (stats[5], N, stats[6]))
    assert stats[5] > 0 and stats[6] == 0, stats
    same_tables(go, gc, o)


def dirty_batch(rng, variant, at, neg, avoid):
    """A clean batch (step 4) whose only dirty message is at index `at`."""
    ids = _gen.zipf_ids(rng, N, K)
    ids[ids == avoid] = (avoid + 1) % K
    a, t, e = raising_states(rng, N, 4)
    cnt = np.bincount(ids, minlength=K)
    mid = N // 2
    if variant == "incast_hot":      # the directory path: the flush's log entries
        ids[at] = int(cnt.argmax())
    elif variant == "incast_cold":   # a bucket named once more in the batch
        ids[at] = int(np.nonzero(cnt == 1)[0][0])
    elif variant == "incast_new":    # a bucket the batch creates
        ids[[mid - 7, mid, mid + 9]] = K + 7
        ids[at] = K + 7
    if variant == "negzero":
        # a bucket seeded negative, named twice: +0.0 and -0.0 in `added`.
        # Go keeps the zero it sees first (+0 > negative, then -0 > +0 is false).
        ids[mid] = avoid
        a[mid] = np.uint64(0)
        ids[at] = avoid
        a[at] = NEG0
    else:
        a[at], t[at], e[at] = 0, 0, 0
    return Batch(ids, a, t, e, _gen.T0 + 4 * SEC)


@gpu
@pytest.mark.parametrize("at", [N - 1, 0], ids=["last", "first"])
@pytest.mark.parametrize("variant", ["incast_hot", "incast_cold", "incast_new", "negzero"])
def test_failed_speculation_is_undone(pa, variant, at):
    """Three clean batches raising the same buckets (a record line left stale
    across a batch boundary would show), then a batch whose only dirty message
    comes last -- everything else was merged before the pass saw it -- or
    first.  The pass is undone (k_undo) and the batch run again classified: a
    fresh handle's first dirty batch takes the prefix rule, so the ordered
    path gets n - (first dirty index) messages, and an incast's reply carries
    the prefix's state."""
    rng = np.random.default_rng(710 + ["incast_hot", "incast_cold", "incast_new", "negzero"].index(variant))
    go, gc, o, neg = trio(pa, rng, negative=0.3 if variant == "negzero" else 0.0)
    # (negzero: its bucket stays out of the clean batches, so it is still negative)
    avoid = int(np.nonzero(neg)[0][5]) if variant == "negzero" else K - 1
    keep = []
    for step in (1, 2, 3):
        ids = _gen.zipf_ids(rng, N, K)
        ids[ids == avoid] = (avoid + 1) % K
        b = Batch(ids, *raising_states(rng, N, step), _gen.T0 + step * SEC)
        keep.append((b.run(go), b.run(gc), b.oracle(o)))
    b = dirty_batch(rng, variant, at, neg, avoid)
    go.set_timing(True)
    dgo, dgc, ref = b.run(go), b.run(gc), b.oracle(o)
    ran = kernels(go)
    assert "k_undo" in ran and classified(ran), ran
    check(dgo, ref, dgc)
    if variant != "negzero":
        assert (ref[0][at] & 0x7F) in (2, 3)   # an incast, answered or not
    assert go.last_stats()[4] == N - at, go.last_stats()
    assert gc.last_stats()[4] == N - at, gc.last_stats()
    same_tables(go, gc, o)


@gpu
def test_queued_batches_with_a_dirty_one_and_new_buckets(pa):
    """Twelve queued batches back to back: batch 5 dirty (its optimistic pass
    is undone by the call that queues batch 6, whose front is queued again),
    batches 2 and 7 with new buckets (the miss path behind an optimistic and
    behind a classified pass)."""
    rng = np.random.default_rng(720)
    go, gc, o, _ = trio(pa, rng)
    done = []
    for j in range(12):
        ids = _gen.zipf_ids(rng, N, K + {2: 300, 7: 600}.get(j, 0))
        a, t, e = raising_states(rng, N, j + 1)
        if j == 5:
            hot = np.bincount(ids).argsort()[::-1][:4]
            pos = rng.choice(N, 11, replace=False)
            ids[pos[0]] = hot[0]
            ids[pos[1:6]] = rng.integers(0, K, 5)
            a[pos[:6]], t[pos[:6]], e[pos[:6]] = 0, 0, 0
            a[pos[6:9]] = NEG0
            t[pos[9:]] = NEG0
        b = Batch(ids, a, t, e, _gen.T0 + (j + 1) * SEC)
        done.append((b.run(go, True), b.run(gc, True), b.oracle(o)))
    go.flush()
    gc.flush()
    for dgo, dgc, ref in done:
        check(dgo, ref, dgc)
    same_tables(go, gc, o)


@gpu
@pytest.mark.parametrize("trailing_incast", [False, True])
def test_log_overflow(pa, trailing_incast):
    """Uniform ids, and every message exceeds in all three fields whatever its
    bucket held before it (values rise along the batch): every cold message
    logs, 64 a wave against the 56 a wave's region holds.  The pass counts the overflow and
    is undone, the results are exact, and the handle's next batch is
    classified first.  With an incast as the last message: overflow and a
    dirty message in one pass."""
    rng = np.random.default_rng(730)
    go, gc, o, _ = trio(pa, rng)
    ids = rng.integers(0, K, N)
    up = np.arange(N, dtype=np.float64)
    t = (2e6 + up).view(np.uint64).copy()
    a = (2e6 + up + 0.5).view(np.uint64).copy()
    e = (1 << 40) + np.arange(N, dtype=np.int64)
    if trailing_incast:
        a[-1], t[-1], e[-1] = 0, 0, 0
    b = Batch(ids, a, t, e, _gen.T0 + SEC)
    go.set_timing(True)
    dgo, dgc, ref = b.run(go), b.run(gc), b.oracle(o)
    assert "k_undo" in kernels(go)
    stats = go.last_stats()
    assert stats[6] > 0, stats
    assert stats[4] == (1 if trailing_incast else 0), stats
    check(dgo, ref, dgc)
    same_tables(go, gc, o)
    b2 = Batch(_gen.zipf_ids(rng, N, K), *raising_states(rng, N, 2), _gen.T0 + 2 * SEC)
    dgo, dgc, ref = b2.run(go), b2.run(gc), b2.oracle(o)
    ran = kernels(go)
    assert classified(ran) and "k_undo" not in ran, ran
    check(dgo, ref, dgc)
    same_tables(go, gc, o)


@gpu
@pytest.mark.parametrize("queue", [False, True])
def test_checked_names_non_monotone_entry(pa, queue):
    """Checked names (names_len: the binding's default) with a non-monotone
    offset entry in mid-batch: PHIP_ERR_INVALID, the prefix applied,
    PHIP_ST_SHORT at the entry and PHIP_ST_NOT_PROCESSED after it, the table
    as the oracle's after the prefix."""
    rng = np.random.default_rng(740)
    go, gc, o, _ = trio(pa, rng)
    b = Batch(_gen.zipf_ids(rng, N, K + 100), *raising_states(rng, N, 1), _gen.T0 + SEC)
    k = 70001
    stop = k - 1                        # message k-1 ends before it starts
    b.offs[k] = b.offs[k - 1] - 1
    got = []
    for g in (go, gc):
        d = b.device()
        with pytest.raises(pa.PatrolHipError) as ei:
            g.receive_soa(d["tb"], d["ta"], d["tt"], d["te"], b.now, name_offs=d["to"], n=N,
                          status=d["status"], device=True, reply=d["reply"], queue=queue)
            g.flush()
        assert ei.value.code == ERR_INVALID
        got.append(d["status"].cpu().numpy())
    st, _, _, _ = o.receive_soa(b.names[:stop], b.a[:stop], b.t[:stop], b.e[:stop], b.now)
    for s in got:
        assert np.array_equal(s[:stop], st), np.nonzero(s[:stop] != st)[0][:8]
        assert s[stop] == ST_SHORT and (s[stop + 1:] == ST_NOT_PROCESSED).all()
    same_tables(go, gc, o)


# ---- the log's sizing (host arithmetic, no device) ----

def layout(n, cus):
    from patrol_amd import _lib
    out = (C.c_uint64 * 4)()
    assert _lib.load().phip_undo_log_layout(n, cus, out, 4) == 4
    return tuple(int(x) for x in out)


def busiest_wave_chunks(n, grid):
    """The fast kernel's chunk walk, wave by wave (phip_kernels.hpp
    k_receive_fast): the most 64-message chunks one wave takes."""
    nchunks, waves = (n + 63) // 64, 16
    if grid % 8 == 0:
        per = (nchunks + 7) // 8
        best = 0
        for x in range(8):
            c0 = x * per
            end = min(nchunks, c0 + per)
            stride = grid // 8 * waves
            best = max(best, max(len(range(c0 + w, end, stride)) for w in range(stride)))
        return best
    stride = grid * waves
    return max(len(range(w, nchunks, stride)) for w in range(stride))


@pytest.mark.parametrize("n,cus", [(1, 256), (N, 256), (N + 1, 256), (N - 1, 256),
                                   (100_000_000, 256), (10**6, 3), (10**6 + 63, 7),
                                   (3 * 10**6 + 1, 12), (1 << 16, 2)])
def test_undo_log_layout(n, cus):
    """Grid, waves, entries per wave region and bytes of the log: n that is
    no multiple of 64 or of the block, grids that are and are not multiples of
    8.  A region holds an entry for every second message of the busiest wave,
    24 more, and 64 for the directory flush."""
    grid, waves, cap, nbytes = layout(n, cus)
    assert grid == max(1, min((n + 1023) // 1024, 2 * cus))
    assert waves == 16 * grid
    assert cap == 32 * busiest_wave_chunks(n, grid) + 24 + 64
    assert nbytes == waves * cap * 32


def test_undo_log_layout_shapes():
    assert layout(N, 256)[:3] == (128, 2048, 120)          # one chunk a wave
    assert layout(N + 1, 256)[0] % 8 != 0                   # 129 workgroups: the plain walk
    assert layout(100_000_000, 256)[:3] == (512, 8192, 191 * 32 + 88)
    assert layout(10**6, 3)[0] == 6
