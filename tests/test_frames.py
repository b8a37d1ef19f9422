"""Packed frames on the GPU (include/patrolhip.h "Packed frames"): the unframe
and cut kernels against the host forms (which tests/test_frames_abi.py holds
to the pure-Python rules), and the one-call ingest -- phip_receive_frames, its
replies form, the ring fed from a socket, the group's composition -- against
the datagram calls over the Python-split records and against the oracle.

Bar: exact equality of offsets, indices, statuses, reply bytes and tables."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _frames_cases as FC  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _replies_cases as RC  # noqa: E402

SEED = 0x5EED
FB = FC.FRAME_DEFAULT


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


@pytest.fixture(scope="module")
def repo(pa):
    """A small seeded table the kernel tests run on (and must leave alone)."""
    g = pa.GPURepo(log2_slots=10, hash_seed=SEED)
    g.seed([b"k%d" % i for i in range(50)], *_gen.clean_states(np.random.default_rng(1), 50),
           np.full(50, _gen.T0, np.int64))
    yield g
    g.close()


def dump(g):
    return {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}


def dev():
    import torch
    return torch.device("cuda", 0)


def up(x, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(dev())


def filled(n, dtype, v=-7):
    import torch
    return torch.full((max(n, 1),), v, dtype=dtype, device=dev())


# -------------------------------------------------------- unframe kernels --
@pytest.mark.parametrize("name", sorted(FC.unframe_cases()))
def test_unframe_device_equals_host(pa, repo, name):
    import torch
    frames = FC.unframe_cases()[name]
    want = pa.unframe(frames, FB)
    data, foffs = FC.frames_blob(frames)
    n = want["n"]
    rec_offs, rec_frame = filled(n + 3, torch.int64), filled(n + 2, torch.int32)
    got = repo.unframe_device(up(data), up(foffs), len(frames), rec_offs, rec_frame, frame_bytes=FB,
                              max_recs=n, bytes_len=int(foffs[-1]))
    assert got == n
    ro, rf = rec_offs.cpu().numpy(), rec_frame.cpu().numpy()
    assert np.array_equal(ro[:n + 1].view(np.uint64), want["rec_offs"])
    assert np.array_equal(rf[:n].view(np.uint32), want["rec_frame"])
    assert (ro[n + 1:] == -7).all() and (rf[n:] == -7).all()      # nothing past the count
    # without rec_frame, offsets trusted
    rec_offs2 = filled(n + 1, torch.int64)
    assert repo.unframe_device(up(data), up(foffs), len(frames), rec_offs2, None, frame_bytes=FB,
                               bytes_len=0) == n
    assert torch.equal(rec_offs2[:n + 1], rec_offs[:n + 1])


def test_unframe_device_errors_leave_everything_alone(pa, repo):
    import torch
    before = dump(repo)
    frames = [FC.record(b"a") * 3, FC.record(b"b" * 200) * 2, FC.record(b"c")]
    data, foffs = FC.frames_blob(frames)
    d_data = up(data)
    rec_offs, rec_frame = filled(16, torch.int64), filled(16, torch.int32)

    def refused(fo, fb, lim, max_recs=15, needed=0):
        with pytest.raises(pa.PatrolHipError) as e:
            repo.unframe_device(d_data, up(fo), len(fo) - 1, rec_offs, rec_frame, frame_bytes=fb,
                                max_recs=max_recs, bytes_len=lim)
        assert e.value.code == FC.INVALID and e.value.needed == needed
        assert (rec_offs == -7).all() and (rec_frame == -7).all()

    total = int(foffs[-1])
    refused(foffs, 256, total)                       # a frame longer than frame_bytes
    refused(foffs, 255, total)
    refused(foffs, 65508, total)
    # checked batches: the bad offsets lie far outside the buffer, nothing is read there
    far = 1 << 45
    dec = foffs.copy()
    dec[2] = dec[1] - 1
    refused(dec, FB, total)
    past = foffs.copy()
    past[1], past[2] = far, far + 30
    refused(past, FB, total)
    past[1], past[2] = foffs[1], total + 1
    past[3] = total + 2
    refused(past, FB, total)
    refused(foffs, FB, total, max_recs=5, needed=6)  # one short: the count comes back
    assert repo.unframe_device(d_data, up(foffs), 3, rec_offs, rec_frame, frame_bytes=FB,
                               max_recs=6, bytes_len=total) == 6
    assert dump(repo) == before


# ----------------------------------------------------------- cut kernels ---
@pytest.mark.parametrize("name", sorted(FC.cuts_cases()))
def test_frame_cuts_device_equals_host(pa, repo, name):
    import torch
    offs, fb = FC.cuts_cases()[name]
    n = len(offs) - 1
    want = pa.frame_cuts(offs, fb)
    k = want["n"]
    frame_offs, frame_first = filled(k + 3, torch.int64), filled(k + 2, torch.int32)
    got = repo.frame_cuts_device(up(offs), n, frame_offs, frame_first, frame_bytes=fb, max_frames=k)
    assert got == k
    fo, ff = frame_offs.cpu().numpy(), frame_first.cpu().numpy()
    assert np.array_equal(fo[:k + 1].view(np.uint64), want["frame_offs"])
    assert np.array_equal(ff[:k].view(np.uint32), want["frame_first"])
    assert (fo[k + 1:] == -7).all() and (ff[k:] == -7).all()
    if name == "tile_of_25_byte_records":
        assert k == 12 and int(want["frame_first"][1]) == 358     # 358 records a frame: the repeat path


def test_frame_cuts_device_errors(pa, repo):
    import torch
    before = dump(repo)
    frame_offs, frame_first = filled(8, torch.int64), filled(8, torch.int32)
    offs = FC.offsets_of([100, 257, 100])

    def refused(fb, max_frames=7, needed=0):
        with pytest.raises(pa.PatrolHipError) as e:
            repo.frame_cuts_device(up(offs), 3, frame_offs, frame_first, frame_bytes=fb,
                                   max_frames=max_frames)
        assert e.value.code == FC.INVALID and e.value.needed == needed
        assert (frame_offs == -7).all() and (frame_first == -7).all()

    refused(256)                                     # a record of 257 bytes
    refused(255)
    refused(65508)
    refused(257, max_frames=2, needed=3)
    assert repo.frame_cuts_device(up(offs), 3, frame_offs, frame_first, frame_bytes=257,
                                  max_frames=3) == 3
    assert dump(repo) == before


# ------------------------------------------------------------ one-call ingest --
def handle(pa, c, **kw):
    kw.setdefault("log2_slots", 13)
    kw.setdefault("hash_seed", SEED)
    g = pa.GPURepo(**kw)
    g.seed(*c["seed"])
    return g


@pytest.fixture(scope="module")
def case():
    """About 3000 records in about 80 frames: Zipf messages over 2000 seeded
    buckets with incast requests (answered, absent, zero, -0.0, asked twice, arena
    names), new buckets, and every ninth name over 14 bytes."""
    c = RC.make_case(21, 3000, K=2000, replies=40, long=6)
    asked = {c["names"][p] for ps in c["tags"].values() for p in ps}
    for i in range(0, 3000, 9):          # (the requests and their buckets' merges stay as built)
        if (c["a"][i] or c["t"][i] or c["e"][i]) and c["names"][i] not in asked:
            c["names"][i] = b"a-new-name-over-14-bytes-%d" % i
    recs = RC.wire(c["names"], c["a"], c["t"], c["e"])
    frames = FC.pack_frames(recs, 1250)              # room for a tail below frame_bytes
    assert 70 <= len(frames) <= 95 and FC.records_of(frames) == recs
    o = O.Repo()
    o.seed(*c["seed"])
    st, ra, rt, re, stop = o.receive(recs, RC.NOW)
    assert stop == len(recs)
    RC.check_case(c, st, ra, rt, re, replies=30, absent=5, zero=5, negzero=3, twice=5, long=5)
    assert int(((st & RC.CREATED) != 0).sum()) >= 100
    return dict(c=c, recs=recs, frames=frames, o=o, st=st, ra=ra, rt=rt, re=re)


def test_receive_frames_equals_the_datagram_call_and_the_oracle(pa, case):
    c, recs, frames = case["c"], case["recs"], case["frames"]
    g, twin = handle(pa, c), handle(pa, c)
    r = g.receive_frames(frames, RC.NOW, frame_bytes=FB)
    t = twin.receive_datagrams(recs, RC.NOW)
    assert r["n_recs"] == len(recs) == r["stop"] and r["rc"] == 0
    assert np.array_equal(r["rec_frame"], np.array(FC.unframe_model(frames)[1], np.uint32))
    assert np.array_equal(r["status"], t["status"]) and np.array_equal(r["status"], case["st"])
    rep = (case["st"] & 0x7F) == RC.REPLY
    assert np.array_equal(r["reply"]["a"][rep], case["ra"][rep])
    assert dump(g) == dump(twin) == case["o"].dump()
    g.close()
    twin.close()


def test_receive_frames_device_form(pa, case):
    import torch
    c, recs, frames = case["c"], case["recs"], case["frames"]
    g = handle(pa, c)
    data, foffs = FC.frames_blob(frames)
    cap = len(recs) + 5
    status, rec_frame = filled(cap, torch.uint8, 0), filled(cap, torch.int32)
    r = g.receive_frames_device(up(data), up(foffs), len(frames), RC.NOW, cap, frame_bytes=FB,
                                status=status, rec_frame=rec_frame)
    assert r == dict(stop=len(recs), n_recs=len(recs), rc=0)
    assert np.array_equal(status.cpu().numpy()[:len(recs)], case["st"])
    assert rec_frame.cpu().numpy()[:len(recs)].tolist() == FC.unframe_model(frames)[1]
    assert dump(g) == case["o"].dump()
    # max_recs one short: PHIP_ERR_INVALID with the count, nothing merged
    g2 = handle(pa, c)
    before = dump(g2)
    with pytest.raises(pa.PatrolHipError) as e:
        g2.receive_frames_device(up(data), up(foffs), len(frames), RC.NOW, len(recs) - 1,
                                 frame_bytes=FB)
    assert e.value.code == FC.INVALID and e.value.needed == len(recs)
    with pytest.raises(pa.PatrolHipError) as e:
        g2.receive_frames(frames, RC.NOW, frame_bytes=FB, max_recs=len(recs) - 1)
    assert e.value.code == FC.INVALID and e.value.needed == len(recs)
    assert dump(g2) == before
    g.close()
    g2.close()


def test_the_datagram_call_sees_only_each_frames_first_record(pa, case):
    """The pin of the opt-in boundary: the same frames handed to
    receive_datagrams as datagrams merge only each frame's first record
    (UnmarshalBinary ignores what follows the name)."""
    c, frames = case["c"], case["frames"]
    g = handle(pa, c)
    r = g.receive_datagrams(frames, RC.NOW)
    o = O.Repo()
    o.seed(*c["seed"])
    firsts = [f[:25 + f[24]] for f in frames]
    st = o.receive(firsts, RC.NOW)[0]
    assert r["stop"] == len(frames) and np.array_equal(r["status"], st)
    assert dump(g) == o.dump() != case["o"].dump()
    g.close()


def test_a_malformed_tail_stops_the_batch_there(pa, case):
    c, frames = case["c"], list(case["frames"])
    frames[40] = frames[40] + b"\x01\x02\x03"
    recs = FC.records_of(frames)
    stop = FC.unframe_model(frames)[1].index(41) - 1          # frame 40's last record: the tail
    assert recs[stop] == b"\x01\x02\x03"
    o = O.Repo()
    o.seed(*c["seed"])
    st, _, _, _, ostop = o.receive(recs, RC.NOW)
    assert ostop == stop
    for device in (False, True):
        g, twin = handle(pa, c), handle(pa, c)
        t = twin.receive_datagrams(recs, RC.NOW)
        if device:
            import torch
            data, foffs = FC.frames_blob(frames)
            status = filled(len(recs), torch.uint8, 0)
            r = g.receive_frames_device(up(data), up(foffs), len(frames), RC.NOW, len(recs),
                                        frame_bytes=FB, status=status)
            got_st = status.cpu().numpy()
        else:
            r = g.receive_frames(frames, RC.NOW, frame_bytes=FB)
            got_st = r["status"]
        assert r["rc"] == FC.SHORT_BUFFER and r["stop"] == stop == t["stop"]
        assert r["n_recs"] == len(recs)
        assert np.array_equal(got_st, t["status"]) and np.array_equal(got_st[:stop], st[:stop])
        # nothing after the stop is applied, the later frames included
        assert dump(g) == dump(twin) == o.dump()
        g.close()
        twin.close()


def test_receive_frames_replies(pa, case):
    c, recs, frames = case["c"], case["recs"], case["frames"]
    g, twin = handle(pa, c), handle(pa, c)
    r = g.receive_frames(frames, RC.NOW, frame_bytes=FB, replies={})
    t = twin.receive_datagrams_replies(recs, RC.NOW)
    e = RC.expected(c["names"], case["st"], case["ra"], case["rt"], case["re"])
    assert e["n"] >= 30
    for x in (r, t):
        assert (x["n"], x["replies"], x["skipped"], x["bytes"]) == \
            (e["n"], e["replies"], e["skipped"], e["bytes"])
        assert bytes(x["data"]) == e["data"]
        assert np.array_equal(x["offs"], e["offs"]) and np.array_equal(x["src"], e["src"])
    assert np.array_equal(r["status"], case["st"]) and dump(g) == dump(twin)
    # src[] are record indices: rec_frame maps them to the frames' senders
    peers = np.zeros((len(frames), 128), np.uint8)
    peers[:, 0] = np.arange(len(frames)) % 251
    peers[:, 1] = np.arange(len(frames)) // 251
    model_frame = np.array(FC.unframe_model(frames)[1])
    out = pa.frame_reply_peers(peers, r["rec_frame"], r["src"])
    assert np.array_equal(out, peers[model_frame[e["src"]]])
    g.close()
    twin.close()


def test_ring_receive_frames_over_loopback(pa):
    """export_sweep -> frame_cuts -> phip_udp_send_batch with the frame offsets
    -> phip_udp_recv_frames into a second handle's ring."""
    rng = np.random.default_rng(31)
    K = 5000
    names = [b"b%d" % i if i % 11 else b"a-bucket-name-of-the-arena-kind-%d" % i for i in range(K)]
    a, t, e = _gen.clean_states(rng, K)
    src = pa.GPURepo(log2_slots=14, hash_seed=SEED)
    src.seed(names, a, t, e, np.full(K, _gen.T0, np.int64))
    dgs, _, st = src.export_sweep(max_msgs=1 << 14)
    assert st["done"] and st["n"] == K
    data = np.frombuffer(b"".join(dgs) + bytes(8), np.uint8)
    cuts = pa.frame_cuts(st["offs"], FB)
    assert cuts["n"] < K // 30
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    rx.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
    rx.bind(("127.0.0.1", 0))
    tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tx.connect(rx.getsockname())
    dst = pa.GPURepo(log2_slots=14, hash_seed=SEED + 1)
    ring = pa.Ring(dst, nslots=2, max_msgs=64, max_bytes=FB * 64)
    try:
        assert pa.udp_send_batch(tx, data, cuts["frame_offs"]) == cuts["n"]
        left, recs = cuts["n"], 0
        while left:
            slot, n, peers = ring.recv_frames(rx, FB, timeout_ms=2000)
            assert n, "frames lost on loopback"
            assert len(peers) == n
            ring.submit(slot, n)
            r = ring.receive_frames(slot, 64 * 60, _gen.T0 + 5, frame_bytes=FB)
            assert r["rc"] == 0 and r["stop"] == r["n_recs"]
            assert ((r["status"] & 0x7F) == 1).all()
            recs += r["n_recs"]
            left -= n
        assert recs == K
        want = {k: v[:3] for k, v in dump(src).items()}
        got = dump(dst)
        assert {k: v[:3] for k, v in got.items()} == want       # `created` excepted
        assert all(v[3] == _gen.T0 + 5 for v in got.values())
    finally:
        ring.close()
        rx.close()
        tx.close()
        src.close()
        dst.close()


def test_group_receive_frames(pa, case):
    """Composition only: the union of a shared-device group's tables equals
    the datagram call's."""
    recs = case["recs"]
    per_recs = [recs[:1700], recs[1700:]]
    per_frames = [FC.pack_frames(p, FB) for p in per_recs]
    ga = pa.GPUGroup.open_all([0, 0], log2_slots=13)
    gb = pa.GPUGroup.open_all([0, 0], log2_slots=13)
    ra = ga.receive_frames(per_frames, RC.NOW, frame_bytes=FB)
    rb = gb.receive_datagrams(per_recs, RC.NOW)
    assert ra == rb and ga.last_rc == 0
    assert ra[2] == [len(p) for p in per_recs]                  # stopped: record counts
    for i in range(2):
        assert ga.last_rec_frame[i].cpu().numpy().tolist() == FC.unframe_model(per_frames[i])[1]
    ua, ub = {}, {}
    for repo in ga.repos:
        ua.update(dump(repo))
    for repo in gb.repos:
        ub.update(dump(repo))
    # (the group's tables start empty: one bucket per name of the batch)
    assert ua == ub and len(ua) == len(set(case["c"]["names"]))
    ga.close()
    gb.close()
