"""The hot-bucket directory of a fast Receive batch (phip_kernels.hpp
k_hot_dir): message j*stride of the batch is resolved and counted, and the
buckets sampled most often -- the lowest threshold t >= 8 with at most 736
buckets counted t or more times -- form the directory.

The directory's observable is GPURepo.last_stats(): [0] its entries, [1] the
batch's messages folded through it.  The sample positions are fixed
(stride 64 below 2^23 messages), so both are deterministic and recomputed
here in numpy; every case also compares statuses and the full table dump
with the oracle.

Shapes: 2^17 slots, 4000 seeded buckets (every sampled name resolves),
batches of 2^16 (the smallest that builds a directory: 1024 samples) to 2^19
messages.
"""
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import _gen
from tests.test_receive_optimistic import Batch, check, dump, kernels, raising_states

gpu = pytest.mark.gpu

SEC = 10**9
K = 4000
STRIDE = 64
HOT_MAX = 736
MIN_COUNT = 8
OLD_CHAIN = ("k_hot_sample", "k_hot_select")


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def seeded(pa, rng, names, **kw):
    """The buckets `names` on a handle of 2^17 slots and in the oracle."""
    a, t, e = _gen.clean_states(rng, len(names))
    created = _gen.T0 - rng.integers(0, SEC, len(names))
    g = pa.GPURepo(log2_slots=17, isolate=False, **kw)
    o = O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)
    return g, o


def expect(ids):
    """(entries, hits, selected ids) of a batch naming bucket ids[i] in message i."""
    cnt = np.bincount(ids[::STRIDE])
    t = MIN_COUNT
    while (cnt >= t).sum() > HOT_MAX:
        t += 1
    sel = np.nonzero(cnt >= t)[0]
    return len(sel), int(np.isin(ids, sel).sum()), sel


class NamedBatch(Batch):
    """A Batch of arbitrary names."""

    def __init__(self, names, a, t, e, now):
        self.names = names
        self.a, self.t, self.e, self.now = a, t, e, now
        self.n = len(names)
        offs = np.zeros(self.n + 1, np.int64)
        offs[1:] = np.cumsum([len(x) for x in names])
        self.offs = offs.astype(np.int32)
        self.blob = np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()


def same_table(g, o):
    want, got = o.dump(), dump(g)
    assert len(got) == len(want)
    bad = [k for k in want if got.get(k) != want[k]]
    assert not bad, [(k, got.get(k), want[k]) for k in bad[:5]]


def shape_ids(rng, shape):
    if shape == "zipf_2^16":
        return _gen.zipf_ids(rng, 1 << 16, K)
    if shape == "zipf_off_tile":
        return _gen.zipf_ids(rng, (1 << 17) + 65, K)
    n = (1 << 16) if shape == "distinct" else (1 << 19)
    # unsampled positions: cold buckets of [1024, K), a few messages each
    ids = rng.integers(1024, K, n)
    j = np.arange(n // STRIDE)
    ids[::STRIDE] = {"mod900": j % 900, "mod700": j % 700, "distinct": j}[shape]
    return ids


# (entries the issue derives by hand from the selection rule; None: numpy's count alone)
SHAPES = [("zipf_2^16", None), ("zipf_off_tile", None), ("mod900", 92), ("mod700", 700),
          ("distinct", 0)]


@gpu
@pytest.mark.parametrize("shape,entries", SHAPES, ids=[s for s, _ in SHAPES])
def test_selection_is_exact(pa, shape, entries):
    """The directory is the selection rule's set: its size and the messages
    it folds equal numpy's, for the smallest batch with a directory, one off
    the tile, more qualifying buckets than the directory holds (8192 samples:
    92 buckets counted 10 times, 808 counted 9, threshold 10), all qualifying
    buckets fitting (counts 11 and 12), and none qualifying."""
    rng = np.random.default_rng(811)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    ids = shape_ids(rng, shape)
    n = len(ids)
    want_entries, want_hits, _ = expect(ids)
    if entries is not None:
        assert want_entries == entries
    if shape == "distinct":
        assert want_hits == 0
    b = Batch(ids, *raising_states(rng, n, 1), _gen.T0 + SEC)
    d = b.run(g)
    stats = g.last_stats()
    print(shape, "entries %d hits %d (expected %d, %d)" % (stats[0], stats[1], want_entries, want_hits))
    assert stats[:3] == (want_entries, want_hits, 0), stats
    check(d, b.oracle(o))
    same_table(g, o)
    g.close()


def hot_cold_ids(rng, n, hot):
    """90% of the messages on the 50 buckets from `hot` on, the rest cold."""
    ids = rng.integers(2000, K, n)
    m = rng.random(n) < 0.9
    ids[m] = hot + rng.integers(0, 50, int(m.sum()))
    return ids


@gpu
@pytest.mark.parametrize("queue", [False, True])
def test_no_state_carried_between_batches(pa, queue):
    """Three batches on one handle with disjoint hot sets A, B, A: each
    batch's directory is its own (a count table, ticket or candidate list
    left over from the batch before would change the entries or the hits)."""
    rng = np.random.default_rng(812)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)))
    n = 1 << 17
    done = []
    for step, hot in ((1, 0), (2, 1000), (3, 0)):
        ids = hot_cold_ids(rng, n, hot)
        want_entries, want_hits, sel = expect(ids)
        assert want_entries >= 50 and set(range(hot, hot + 50)) <= set(sel.tolist())
        b = Batch(ids, *raising_states(rng, n, step), _gen.T0 + step * SEC)
        done.append((b.run(g, queue), b.oracle(o)))
        stats = g.last_stats()   # (finishes a queued batch)
        assert stats[:3] == (want_entries, want_hits, 0), (step, stats, want_entries, want_hits)
    g.flush()
    for d, ref in done:
        check(d, ref)
    same_table(g, o)
    g.close()


@gpu
@pytest.mark.parametrize("path", ["classify_first", "datagrams"])
def test_other_paths_use_the_one_kernel(pa, path):
    """The classified pass (directory beside k_classify) and the wire path
    build the same directory with the same kernel: once per batch, and none
    of the chain it replaced."""
    rng = np.random.default_rng(811)
    g, o = seeded(pa, rng, _gen.key_names(np.arange(K)), classify_first=(path == "classify_first"))
    ids = shape_ids(rng, "zipf_2^16")
    n = len(ids)
    want_entries, want_hits, _ = expect(ids)
    a, t, e = raising_states(rng, n, 1)
    g.set_timing(True)
    if path == "datagrams":
        names = _gen.key_names(ids)
        dgs = [struct.pack(">QQQ", int(a[i]), int(t[i]), int(e[i])) + bytes([len(names[i])]) + names[i]
               for i in range(n)]
        out = g.receive_datagrams(dgs, _gen.T0 + SEC)
        ran = kernels(g)
        st = o.receive(dgs, _gen.T0 + SEC)[0]
        assert out["stop"] == n and np.array_equal(out["status"], st)
    else:
        b = Batch(ids, a, t, e, _gen.T0 + SEC)
        d = b.run(g)
        ran = kernels(g)
        check(d, b.oracle(o))
    assert ran.count("k_hot_dir") == 1 and not any(k in ran for k in OLD_CHAIN), ran
    assert any(k.startswith("k_classify") for k in ran), ran
    stats = g.last_stats()
    assert stats[:3] == (want_entries, want_hits, 0), (stats, want_entries, want_hits)
    same_table(g, o)
    g.close()


@gpu
def test_hot_long_names(pa):
    """Hot buckets named by 15 bytes (inline in the record) and by 32 bytes
    (in the arena, matched from the directory's tail words): entries, hits
    and the table are exact."""
    rng = np.random.default_rng(814)
    hot = [(b"h%014d" if i % 2 else b"L%031d") % i for i in range(50)]
    assert {len(x) for x in hot} == {15, 32}
    all_names = hot + _gen.key_names(np.arange(50, K))
    g, o = seeded(pa, rng, all_names)
    n = 1 << 17
    ids = hot_cold_ids(rng, n, 0)
    want_entries, want_hits, sel = expect(ids)
    assert set(range(50)) <= set(sel.tolist())
    b = NamedBatch([all_names[i] for i in ids], *raising_states(rng, n, 1), _gen.T0 + SEC)
    d = b.run(g)
    stats = g.last_stats()
    assert stats[:3] == (want_entries, want_hits, 0), (stats, want_entries, want_hits)
    check(d, b.oracle(o))
    same_table(g, o)
    g.close()
