"""Incast reply egress on the GPU (include/patrolhip.h "Incast reply
egress"): a receive call's incast replies as datagrams written on the device,
on each of its paths -- the one-launch small batch, the deferred sub-batch
(no column of the batch's size), the ordered suffix, the ring -- against the
model of tests/_replies_cases.py over the oracle's columns.

Bar: byte-identical datagrams, offsets and source indices; statuses and
tables bit-exact as the plain receive call leaves them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _replies_cases as RC  # noqa: E402

N = 1 << 16
SEED = 0x5EED


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def dump(repo):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}
    assert len(repo) == len(d)
    return d


def same(g, o):
    assert len(g) == len(o)
    bad = [k for k in o if g.get(k) != o[k]]
    assert not bad, [(k, g.get(k), o[k]) for k in bad[:5]]


def handle(pa, c, **kw):
    kw.setdefault("log2_slots", 14)
    kw.setdefault("hash_seed", SEED)
    g = pa.GPURepo(**kw)
    g.seed(*c["seed"])
    return g


def oracle_run(c, as_wire=False, dgs=None):
    """-> (oracle repo after the batch, st, ra, rt, re, stop)"""
    o = O.Repo()
    o.seed(*c["seed"])
    if as_wire:
        st, ra, rt, re, stop = o.receive(dgs or RC.wire(c["names"], c["a"], c["t"], c["e"]), RC.NOW)
    else:
        st, ra, rt, re = o.receive_soa(c["names"], c["a"], c["t"], c["e"], RC.NOW)
        stop = len(c["names"])
    return o, st, ra, rt, re, stop


@pytest.fixture(scope="module")
def small_case():
    c = RC.make_case(11, 600, K=200, long=6)
    ref = {w: oracle_run(c, w) for w in (False, True)}
    RC.check_case(c, *ref[False][1:5], replies=50, absent=5, zero=5, negzero=3, twice=5, long=5)
    return c, ref


@pytest.fixture(scope="module")
def deferred_case():
    """About 300 dirty messages over short names."""
    c = RC.make_case(12, N, replies=250)
    ref = {w: oracle_run(c, w) for w in (False, True)}
    RC.check_case(c, *ref[False][1:5], replies=250, absent=5, zero=5, negzero=3, twice=5)
    assert max(len(x) for x in c["names"]) <= 14
    return c, ref


@pytest.fixture(scope="module")
def suffix_case():
    """Dirty names over 14 bytes: the ordered path from the first dirty message on."""
    c = RC.make_case(13, N, replies=80, long=6)
    ref = {w: oracle_run(c, w) for w in (False, True)}
    RC.check_case(c, *ref[False][1:5], replies=80, absent=5, zero=5, negzero=3, twice=5, long=5)
    return c, ref


def got_bytes(r):
    """(data bytes, offs, src) of a reply dict, host or device, cut to what was written."""
    k = r["n"]
    data, offs, src = r["data"], r["offs"], r["src"]
    if hasattr(data, "cpu"):
        data, offs = data.cpu().numpy(), offs.cpu().numpy().view(np.uint64)
        src = src.cpu().numpy().view(np.uint32) if src is not None else None
    return (bytes(np.asarray(data)[:r["bytes"]]), np.asarray(offs)[:k + 1],
            np.asarray(src)[:k] if src is not None else None)


def assert_replies(r, e):
    assert (r["n"], r["replies"], r["skipped"], r["bytes"]) == \
        (e["n"], e["replies"], e["skipped"], e["bytes"]), (r["n"], r["replies"], r["skipped"])
    data, offs, src = got_bytes(r)
    assert np.array_equal(offs, e["offs"])
    assert data == e["data"]
    if src is not None:
        assert np.array_equal(src, e["src"])


def dev_out(max_msgs, out_cap=None, fill=0):
    import torch
    dev = torch.device("cuda", 0)
    out_cap = 256 * max_msgs + 8 if out_cap is None else out_cap
    return (torch.full((out_cap,), fill, dtype=torch.uint8, device=dev),
            torch.full((max_msgs + 1,), 7, dtype=torch.int64, device=dev),
            torch.full((max_msgs,), 7, dtype=torch.int32, device=dev))


def dev_soa(c):
    import torch
    dev = torch.device("cuda", 0)
    names = c["names"]
    offs = np.zeros(len(names) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in names])
    tb = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()).to(dev)
    to = torch.from_numpy(offs.astype(np.int32)).to(dev)
    ta, tt, te = (torch.from_numpy(x.view(np.int64).copy()).to(dev)
                  for x in (c["a"], c["t"], c["e"]))
    return tb, to, ta, tt, te


def dev_wire(dgs):
    import torch
    dev = torch.device("cuda", 0)
    offs = np.zeros(len(dgs) + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in dgs])
    data = torch.from_numpy(np.frombuffer(b"".join(dgs) + b"\0" * 8, np.uint8).copy()).to(dev)
    return data, torch.from_numpy(offs).to(dev)


def call_device(g, c, as_wire, max_msgs=4096, out_cap=None, status=False, dgs=None, **kw):
    """One device-pointer *_replies call over the case (soa or wire form)."""
    import torch
    n = len(c["names"])
    out, offs, src = dev_out(max_msgs, out_cap)
    st = torch.zeros(n, dtype=torch.uint8, device=out.device) if status else None
    if as_wire:
        data, doffs = dev_wire(dgs or RC.wire(c["names"], c["a"], c["t"], c["e"]))
        r = g.receive_datagrams_replies_device(data, doffs, n, RC.NOW, out, offs, src, max_msgs,
                                               status=st)
    else:
        tb, to, ta, tt, te = dev_soa(c)
        r = g.receive_soa_replies_device(n, tb, to, ta, tt, te, RC.NOW, out, offs, src, max_msgs,
                                         status=st, **kw)
    torch.cuda.synchronize()
    return r


# 1 ------------------------------------------------------------ small path --
@pytest.mark.parametrize("as_wire", [False, True])
def test_small_batch_one_launch(pa, small_case, as_wire):
    c, ref = small_case
    o, st, ra, rt, re, _ = ref[as_wire]
    e = RC.expected(c["names"], st, ra, rt, re)
    g, twin = handle(pa, c), handle(pa, c)
    g.set_timing(True)
    dgs = RC.wire(c["names"], c["a"], c["t"], c["e"])
    if as_wire:
        r = g.receive_datagrams_replies(dgs, RC.NOW)
        full = twin.receive_datagrams(dgs, RC.NOW)
        assert r["stop"] == len(dgs)
    else:
        r = g.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW)
        full = twin.receive_soa(c["names"], c["a"], c["t"], c["e"], RC.NOW)
    assert [k for k, _ in g.timings()] == ["k_small_mixed"]      # still one launch
    assert_replies(r, e)
    # the host helper over the twin's full columns writes the same bytes
    offs = np.zeros(len(dgs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in dgs])
    data, oo, _ = pa.incast_replies(np.frombuffer(b"".join(dgs), np.uint8).copy(), offs,
                                    full["status"], full["reply"])
    assert bytes(data) == bytes(r["data"]) and np.array_equal(oo, r["offs"])
    assert np.array_equal(r["status"], st) and np.array_equal(full["status"], st)
    same(dump(g), o.dump())
    same(dump(twin), o.dump())
    # no column at all: the same replies
    g2 = handle(pa, c)
    r2 = (g2.receive_datagrams_replies(dgs, RC.NOW, want_status=False) if as_wire else
          g2.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW, want_status=False))
    assert r2["status"] is None
    assert_replies(r2, e)


# 2 --------------------------------------------------------- deferred path --
@pytest.mark.parametrize("as_wire", [False, True])
def test_deferred_sub_batch_needs_no_column(pa, deferred_case, as_wire):
    c, ref = deferred_case
    o, st, ra, rt, re, _ = ref[as_wire]
    e = RC.expected(c["names"], st, ra, rt, re)
    ndirty = int(RC.dirty_mask(c["a"], c["t"], c["e"]).sum())
    assert 250 <= ndirty <= 400
    for status in (False, True):          # res NULL, then only status
        g = handle(pa, c, isolate=True)
        g.set_timing(True)
        r = call_device(g, c, as_wire, status=status)
        assert 0 < g.last_stats()[4] <= 5 * ndirty, g.last_stats()      # run_deferred ran
        ks = [k for k, _ in g.timings()]
        assert ks.count("k_reply_select") == 1 and ks.count("k_reply_write") == 1
        assert "k_reply_place" not in ks
        assert_replies(r, e)
        if status:
            assert np.array_equal(r["status"].cpu().numpy(), st)
        same(dump(g), o.dump())


def test_deferred_host_pointers(pa, deferred_case):
    """A large host-pointer batch: staged as the receive call stages, only what
    was written copied back."""
    c, ref = deferred_case
    o, st, ra, rt, re, _ = ref[False]
    g = handle(pa, c, isolate=True)
    r = g.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW, max_msgs=4096)
    assert_replies(r, RC.expected(c["names"], st, ra, rt, re))
    assert np.array_equal(r["status"], st)
    same(dump(g), o.dump())


# 3 ----------------------------------------------------------- suffix path --
@pytest.mark.parametrize("as_wire", [False, True])
def test_ordered_suffix(pa, suffix_case, as_wire):
    c, ref = suffix_case
    o, st, ra, rt, re, _ = ref[as_wire]
    e = RC.expected(c["names"], st, ra, rt, re)
    first = int(np.argmax(RC.dirty_mask(c["a"], c["t"], c["e"])))
    for status in (False, True):
        g = handle(pa, c, isolate=True)
        g.set_timing(True)
        r = call_device(g, c, as_wire, status=status)
        assert g.last_stats()[4] == N - first, g.last_stats()
        ks = [k for k, _ in g.timings()]
        assert [ks.count(k) for k in ("k_reply_count", "k_reply_scan", "k_reply_place")] == [1, 1, 1]
        assert_replies(r, e)
        if status:
            assert np.array_equal(r["status"].cpu().numpy(), st)
        same(dump(g), o.dump())


def test_suffix_over_the_dirty_cap(pa):
    """More than 4096 dirty messages over short names: the prefix rule, and
    more replies than one workgroup's sort would hold."""
    c = RC.make_case(14, N, replies=4600)
    o, st, ra, rt, re, _ = oracle_run(c)
    e = RC.expected(c["names"], st, ra, rt, re)
    assert e["replies"] > 4096
    g = handle(pa, c, isolate=True)
    r = call_device(g, c, False, max_msgs=8192)
    assert g.last_stats()[4] == N - int(np.argmax(RC.dirty_mask(c["a"], c["t"], c["e"])))
    assert_replies(r, e)
    same(dump(g), o.dump())


# 4 ------------------------------------------------------- stopped batches --
@pytest.mark.parametrize("n", [600, N])
def test_short_datagram_stops_the_replies(pa, small_case, deferred_case, n):
    c, _ = small_case if n == 600 else deferred_case
    dgs = RC.wire(c["names"], c["a"], c["t"], c["e"])
    k = n // 2
    while any(abs(p - k) < 2 for ps in c["tags"].values() for p in ps):
        k += 1
    dgs[k] = dgs[k][:20]
    o, st, ra, rt, re, stop = oracle_run(c, True, dgs)
    assert stop == k
    e = RC.expected(c["names"][:k], st[:k], ra[:k], rt[:k], re[:k])
    after = RC.expected(c["names"], *oracle_run(c, True)[1:5])
    assert 0 < e["n"] < after["n"]            # replies before and after k
    g = handle(pa, c, isolate=True)
    if n == 600:
        r = g.receive_datagrams_replies(dgs, RC.NOW)
        got_st = r["status"]
    else:
        r = call_device(g, c, True, status=True, dgs=dgs)
        got_st = r["status"].cpu().numpy()
    assert r["rc"] == -5 and r["stop"] == k
    assert_replies(r, e)
    assert np.array_equal(got_st, st)
    same(dump(g), o.dump())


def test_malformed_offset_stops_the_replies(pa, deferred_case):
    """A checked device soa batch (names_len) with a malformed offset entry."""
    import torch
    c, _ = deferred_case
    k = N // 2 + 1
    stop = k - 1              # message k - 1 ends past the blob
    o = O.Repo()
    o.seed(*c["seed"])
    st, ra, rt, re = o.receive_soa(c["names"][:stop], c["a"][:stop], c["t"][:stop],
                                   c["e"][:stop], RC.NOW)
    e = RC.expected(c["names"][:stop], st, ra, rt, re)
    assert 0 < e["n"]
    g = handle(pa, c, isolate=True)
    tb, to, ta, tt, te = dev_soa(c)
    to[k] = 0x7FFF0000
    out, offs, src = dev_out(4096)
    status = torch.zeros(N, dtype=torch.uint8, device=out.device)
    r = g.receive_soa_replies_device(N, tb, to, ta, tt, te, RC.NOW, out, offs, src, 4096,
                                     status=status, allow=(-1,))
    assert r["rc"] == -1
    assert_replies(r, e)
    got = status.cpu().numpy()
    assert np.array_equal(got[:stop], st) and got[stop] == 4 and (got[stop + 1:] == 5).all()
    same(dump(g), o.dump())


# 5 ------------------------------------------------------------------ caps --
@pytest.mark.parametrize("path", ["small", "deferred", "suffix"])
def test_caps_cut_at_a_record(pa, small_case, deferred_case, suffix_case, path):
    c, ref = {"small": small_case, "deferred": deferred_case, "suffix": suffix_case}[path]
    o, st, ra, rt, re, _ = ref[False]
    full = RC.expected(c["names"], st, ra, rt, re)
    half = full["n"] // 2
    # max_msgs below the reply count
    e = RC.expected(c["names"], st, ra, rt, re, max_msgs=half)
    g = handle(pa, c, isolate=True)
    if path == "small":
        r = g.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW, max_msgs=half)
    else:
        r = call_device(g, c, False, max_msgs=half)
    assert e["n"] == half < r["replies"] == full["replies"]
    assert_replies(r, e)
    assert e["data"] == full["data"][:e["bytes"]]          # a prefix, in order
    same(dump(g), o.dump())                                # the table as the uncut call leaves it
    # a byte budget that cuts mid-way (device: out_cap - 8, a multiple of 8)
    cap = (int(full["offs"][half]) + 3) // 8 * 8 + 8
    budget = cap if path == "small" else cap - 8
    e = RC.expected(c["names"], st, ra, rt, re, budget=budget)
    assert 0 < e["n"] < full["n"]
    g = handle(pa, c, isolate=True)
    if path == "small":
        r = g.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW, out_cap=cap)
    else:
        r = call_device(g, c, False, out_cap=cap)
        assert bytes(r["data"].cpu().numpy()[e["bytes"]:]) == bytes(cap - e["bytes"])   # untouched
    assert_replies(r, e)
    same(dump(g), o.dump())


def test_refused_arguments_leave_the_table(pa, small_case):
    import torch
    c, _ = small_case
    g = handle(pa, c)
    before = dump(g)
    tb, to, ta, tt, te = dev_soa(c)
    n = len(c["names"])
    out, offs, src = dev_out(64)

    def refused(out_, cap, max_msgs, flags=0):
        with pytest.raises(pa.PatrolHipError) as ei:
            g.receive_soa_replies_device(n, tb, to, ta, tt, te, RC.NOW, out_, offs, src, max_msgs,
                                         out_cap=cap, flags=flags)
        assert ei.value.code == -1
        torch.cuda.synchronize()
        assert dump(g) == before

    refused(out[1:], 512, 64)              # out not 8-byte aligned
    refused(out, 516, 64)                  # out_cap not a multiple of 8
    refused(out, 256, 64)                  # below PHIP_BUCKET_PACKET_SIZE + 8
    refused(out, 512, 0)                   # max_msgs == 0
    refused(out, 512, 64, flags=0x20)      # PHIP_RECV_ASYNC
    for kw in (dict(max_msgs=0), dict(out_cap=255)):
        with pytest.raises(pa.PatrolHipError) as ei:
            g.receive_soa_replies(c["names"], c["a"], c["t"], c["e"], RC.NOW, **kw)
        assert ei.value.code == -1
        assert dump(g) == before
    r = g.receive_soa_replies([], [], [], [], RC.NOW, max_msgs=4)      # no messages
    assert (r["n"], r["replies"], r["skipped"], r["bytes"]) == (0, 0, 0, 0) and r["offs"][0] == 0


# 6 ----------------------------------------------------------- long names --
@pytest.mark.parametrize("n", [300, N])
def test_names_over_231_bytes_are_skipped(pa, small_case, suffix_case, n):
    """Names of 232..255 bytes brought in by datagram, then asked for."""
    c, _ = small_case if n == 300 else suffix_case
    big = [bytes([65 + k]) * (232 + 4 * k) for k in range(6)]
    assert [len(b) for b in big][0] == 232 and len(big[-1]) <= 255
    a, t, e = c["a"].copy(), c["t"].copy(), c["e"].copy()
    names = list(c["names"])
    m = len(names) if n == N else n
    names, a, t, e = names[:m], a[:m], t[:m], e[:m]
    tagged = {q for ps in c["tags"].values() for q in ps}
    free = [p for p in range(10, m - 10) if p not in tagged]
    for k, b in enumerate(big):
        p1, p2 = free[7 * k], free[len(free) // 2 + 7 * k]
        names[p1] = b                      # a replica state creates the bucket
        a[p1], t[p1], e[p1] = np.float64(5.0 + k).view(np.uint64), 0, 9
        names[p2] = b                      # and a request asks for it
        a[p2], t[p2], e[p2] = 0, 0, 0
    dgs = RC.wire(names, a, t, e)
    c2 = dict(c, names=names, a=a, t=t, e=e)
    o, st, ra, rt, re, stop = oracle_run(c2, True, dgs)
    assert stop == m
    ex = RC.expected(names, st, ra, rt, re)
    assert ex["skipped"] == 6 and ex["n"] == ex["replies"] - 6 > 0
    g = handle(pa, c, isolate=True)
    if n == 300:
        r = g.receive_datagrams_replies(dgs, RC.NOW)
    else:
        r = call_device(g, c2, True, dgs=dgs)
    assert_replies(r, ex)
    same(dump(g), o.dump())


# 7 ----------------------------------------------------------- clean batch --
def test_clean_batch_launches_nothing_more(pa):
    import torch
    c = RC.make_case(17, N, replies=0, absent=0, zero=0, negzero=0, twice=0)
    assert not RC.dirty_mask(c["a"], c["t"], c["e"]).any()
    g, twin = handle(pa, c), handle(pa, c)
    for x in (g, twin):
        x.set_timing(True)
    tb, to, ta, tt, te = dev_soa(c)
    twin.receive_soa(tb, ta, tt, te, RC.NOW, name_offs=to, n=N, device=True)
    torch.cuda.synchronize()
    plain = sorted(k for k, _ in twin.timings())
    r = call_device(g, c, False)
    assert sorted(k for k, _ in g.timings()) == plain and plain
    assert (r["n"], r["replies"], r["skipped"], r["bytes"]) == (0, 0, 0, 0)
    assert int(r["offs"][0]) == 0
    o = oracle_run(c)[0]
    same(dump(g), o.dump())
    same(dump(twin), o.dump())


# 8 ------------------------------------------------------------------ ring --
@pytest.mark.parametrize("which", ["small", "large"])
def test_ring_receive_replies(pa, small_case, deferred_case, which):
    c, ref = small_case if which == "small" else deferred_case
    o, st, ra, rt, re, _ = ref[True]
    e = RC.expected(c["names"], st, ra, rt, re)
    dgs = RC.wire(c["names"], c["a"], c["t"], c["e"])
    n = len(dgs)
    peers = np.random.default_rng(3).integers(0, 256, (n, 128), dtype=np.uint8)
    g = handle(pa, c, isolate=True)
    ring = pa.Ring(g, nslots=2, max_msgs=n)
    slot, k = ring.fill(dgs)
    ring.submit(slot, k)
    r = ring.receive_replies(slot, k, RC.NOW, max_msgs=4096)
    assert r["stop"] == n and r["status"] is None
    assert_replies(r, e)
    assert np.array_equal(pa.reply_peers(peers, r["src"]), peers[e["src"]])
    same(dump(g), o.dump())
    # the ring goes on: an empty slot gives zeros
    slot, k = ring.fill([])
    ring.submit(slot, 0)
    r = ring.receive_replies(slot, 0, RC.NOW)
    assert (r["n"], r["replies"], r["bytes"]) == (0, 0, 0) and r["offs"][0] == 0
    ring.close()


# 9 ------------------------------------------------------------ round trip --
def test_replies_feed_a_peer_unchanged(pa, deferred_case):
    import torch
    c, ref = deferred_case
    o, st, ra, rt, re, _ = ref[False]
    e = RC.expected(c["names"], st, ra, rt, re)
    g = handle(pa, c, isolate=True)
    r = call_device(g, c, False)
    assert_replies(r, e)
    peer = pa.GPURepo(log2_slots=14, hash_seed=SEED + 1)
    status = torch.zeros(r["n"], dtype=torch.uint8, device=r["data"].device)
    stop = peer.receive_datagrams_device(r["data"], r["offs"], r["n"], RC.NOW + 1, status=status)
    torch.cuda.synchronize()
    assert stop == r["n"]
    assert ((status.cpu().numpy() & 0x7F) == 1).all()            # PHIP_ST_MERGED
    po = O.Repo()
    assert po.receive(RC.datagrams_of(e), RC.NOW + 1)[4] == e["n"]
    same(dump(peer), po.dump())


# 10 ------------------------------------- more tiles than one scan chunk --
def test_suffix_past_one_chunk_of_the_tile_scan(pa):
    """An ordered suffix of 512 * 256 + 1 messages: 513 tiles, so the last
    tile's bases and the totals come through the carry of k_reply_scan's second
    chunk.  Then max_msgs below the replies of the first chunk: the cut still
    reports every reply."""
    c = RC.chunk_case()
    n, pos = len(c["names"]), c["tags"]["reply"]
    assert n == 512 * 256 + 1 and pos[0] == 0 and pos[-1] == n - 1 and len(pos) >= 40
    o, st, ra, rt, re, _ = oracle_run(c)
    assert all((st[p] & 0x7F) == RC.REPLY for p in pos)
    for max_msgs in (4096, 10):
        e = RC.expected(c["names"], st, ra, rt, re, max_msgs=max_msgs)
        assert e["replies"] == len(pos) and e["n"] == min(len(pos), max_msgs)
        if max_msgs >= len(pos):
            assert int(e["src"][-1]) == n - 1                          # the last tile's reply
        else:
            assert max_msgs < sum(p < 512 * 256 for p in pos)          # cut inside the first chunk
        g = handle(pa, c, isolate=True)
        g.set_timing(True)
        r = call_device(g, c, False, max_msgs=max_msgs)
        assert g.last_stats()[4] == n, g.last_stats()                  # all of it the suffix
        ks = [k for k, _ in g.timings()]
        assert [ks.count(k) for k in ("k_reply_count", "k_reply_scan", "k_reply_place")] == [1, 1, 1]
        assert_replies(r, e)
        assert RC.datagrams_of(e)[-1] == got_bytes(r)[0][int(e["offs"][-2]):]
        same(dump(g), o.dump())
        g.close()
