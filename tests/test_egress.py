"""phip_apply_mixed_egress and the egress batcher on the GPU (include/
patrolhip.h "Coalesced egress"), through the binding.

Every case compares the call's datagrams with tests/_egress_cases.py's model
over the oracle (n, n_incast, bytes, each section as a name -> datagram map
with no name twice, offsets monotone from 0), and its statuses, remaining,
have, reply and the table dump with a second handle's plain apply_mixed on
the same ops.  Bit-exact throughout.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _egress_cases as EC  # noqa: E402
from tests import _gen  # noqa: E402

T0, SEC = _gen.T0, _gen.SEC
COLS = ("kind", "now", "freq", "per", "count", "added", "taken", "elapsed")


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def gpu_dump(repo):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}
    assert len(repo) == len(d), (len(repo), len(d))
    return d


def plain(repo, ops):
    return repo.apply_mixed(ops["kind"], ops["names"], ops["now"], ops["freq"], ops["per"],
                            ops["count"], ops["added"], ops["taken"], ops["elapsed"])


def check_egress(eg, ops, ref, dump):
    """eg: dict(data, offs, n, n_incast) against the model."""
    want_req, want_st = EC.expected_datagrams(ops, ref, dump)
    print("egress: %d ops, %d buckets -> %d requests + %d states (want %d + %d), %d bytes"
          % (len(ops["names"]), len(set(ops["names"])), eg["n_incast"], eg["n"] - eg["n_incast"],
             len(want_req), len(want_st), len(eg["data"])))
    assert eg["n_incast"] == len(want_req)
    assert eg["n"] == len(want_req) + len(want_st)
    want_bytes = sum(map(len, want_req.values())) + sum(map(len, want_st.values()))
    assert len(eg["data"]) == want_bytes and int(eg["offs"][eg["n"]]) == want_bytes
    got_req, got_st = EC.sections(eg)
    assert got_req == want_req
    assert got_st == want_st


def run_case(pa, ops, prior=None, want_status=True, **kw):
    """The batch with egress on one handle, plainly on a twin, on the oracle."""
    kw.setdefault("log2_slots", 12)
    g, twin, o = pa.GPURepo(**kw), pa.GPURepo(**kw), O.Repo()
    try:
        if prior is not None:
            plain(g, prior)
            plain(twin, prior)
            EC.call(o, prior)
        res = g.apply_mixed(ops["kind"], ops["names"], ops["now"], ops["freq"], ops["per"],
                            ops["count"], ops["added"], ops["taken"], ops["elapsed"], egress=True,
                            want_status=want_status)
        base = plain(twin, ops)
        ref = EC.call(o, ops)
        dump = o.dump()
        if want_status:
            assert np.array_equal(res["status"], base["status"])
            assert np.array_equal(res["status"], ref["status"])
        for c in ("remaining", "have", "reply"):
            assert np.array_equal(res[c], base[c]), c
        assert gpu_dump(g) == gpu_dump(twin) == dump
        check_egress(res["egress"], ops, ref, dump)
        return res
    finally:
        g.close()
        twin.close()


# ------------------------------------------------------------ host batches --
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024])
def test_small_batches(pa, n):
    rng = np.random.default_rng(n)
    run_case(pa, EC.gen_ops(rng, n, EC.name_pool(40)))


def test_all_receive_batch_sends_nothing(pa):
    rng = np.random.default_rng(5)
    ops = EC.gen_ops(rng, 300, EC.name_pool(40))
    ops["kind"][:] = EC.RECEIVE
    res = run_case(pa, ops)
    assert res["egress"]["n"] == 0 and res["egress"]["n_incast"] == 0
    assert len(res["egress"]["data"]) == 0 and int(res["egress"]["offs"][0]) == 0


def test_empty_batch(pa):
    g = pa.GPURepo(log2_slots=8)
    z = np.zeros(0, np.int64)
    res = g.apply_mixed(np.zeros(0, np.uint8), [], z, z, z, z.astype(np.uint64), egress=True)
    assert res["egress"]["n"] == 0 and res["egress"]["n_incast"] == 0
    assert len(res["egress"]["data"]) == 0 and list(res["egress"]["offs"]) == [0]
    g.close()


def test_zero_rate_take_on_a_new_bucket_is_a_request_only(pa):
    """Rate 0:1s: the take is denied and the bucket stays a zero state: its
    creation sends the request, and no state datagram follows."""
    ops = dict(names=[b"fresh"], kind=np.zeros(1, np.uint8), now=np.array([T0], np.int64),
               freq=np.zeros(1, np.int64), per=np.array([SEC], np.int64),
               count=np.ones(1, np.uint64), added=np.zeros(1, np.uint64),
               taken=np.zeros(1, np.uint64), elapsed=np.zeros(1, np.int64))
    res = run_case(pa, ops)
    assert (res["egress"]["n"], res["egress"]["n_incast"]) == (1, 1)
    assert bytes(res["egress"]["data"]) == EC.request(b"fresh")


@pytest.mark.parametrize("n,small,want_status", [(5000, True, True), (5000, True, False),
                                                 (1025, True, True), (700, False, True),
                                                 (700, False, False)])
def test_large_path_host(pa, n, small, want_status):
    rng = np.random.default_rng(n + small)
    pool = EC.name_pool(400)
    prior = EC.gen_ops(rng, 300, pool)
    ops = EC.gen_ops(rng, n, pool, t0=int(prior["now"][-1]))
    run_case(pa, ops, prior=prior, small=small, want_status=want_status)


# ---------------------------------------------------------- device batches --
def to_device(ops):
    import torch
    dev = torch.device("cuda", 0)
    n = len(ops["names"])
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in ops["names"]])
    blob = np.frombuffer(b"".join(ops["names"]) + b"\0" * 8, np.uint8).copy()
    t = dict(names=torch.from_numpy(blob).to(dev), name_offs=torch.from_numpy(offs).to(dev))
    for c in COLS:
        a = np.ascontiguousarray(ops[c])
        t[c] = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    return t


def device_egress(repo, ops, with_status=True, names_len=None):
    """-> (egress dict with host copies, out tensor, offs tensor, status or None)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(ops["names"])
    t = to_device(ops)
    nb = int(t["names"].numel()) if names_len is None else (names_len or 231 * n)
    max_msgs, cap = repo.egress_caps(n, nb, device=True)
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev) if with_status else None
    r = repo.apply_mixed_egress_device(n, t["kind"], t["names"], t["name_offs"], t["now"], out,
                                       offs, max_msgs, freq=t["freq"], per=t["per"],
                                       count=t["count"], added=t["added"], taken=t["taken"],
                                       elapsed=t["elapsed"], status=status, names_len=names_len)
    ho = offs.cpu().numpy().view(np.uint64)
    assert int(ho[r["n"]]) == r["bytes"]
    eg = dict(data=out.cpu().numpy()[:r["bytes"]], offs=ho[:r["n"] + 1], n=r["n"],
              n_incast=r["n_incast"])
    return eg, out, offs, (status.cpu().numpy() if with_status else None)


@pytest.mark.parametrize("with_status,names_len", [(True, None), (False, None), (True, 0)])
def test_large_path_device(pa, with_status, names_len):
    rng = np.random.default_rng(21)
    pool = EC.name_pool(400)
    prior = EC.gen_ops(rng, 300, pool)
    ops = EC.gen_ops(rng, 5000, pool, t0=int(prior["now"][-1]))
    g, twin, o = pa.GPURepo(log2_slots=12), pa.GPURepo(log2_slots=12), O.Repo()
    for r in (g, twin):
        plain(r, prior)
    EC.call(o, prior)
    eg, _, _, status = device_egress(g, ops, with_status, names_len)
    base = plain(twin, ops)
    ref = EC.call(o, ops)
    dump = o.dump()
    if with_status:
        assert np.array_equal(status, base["status"])
    assert gpu_dump(g) == gpu_dump(twin) == dump
    check_egress(eg, ops, ref, dump)
    g.close()
    twin.close()


# ---------------------------------------------------------- segment classes --
def interleave(rng, seqs):
    """Per-bucket op sequences -> one stream, each bucket's order kept."""
    labels = np.repeat(np.arange(len(seqs)), [len(s) for s in seqs])
    rng.shuffle(labels)
    pos = [0] * len(seqs)
    out = []
    for b in labels:
        out.append(seqs[b][pos[b]])
        pos[b] += 1
    return out


def build_ops(rng, stream):
    """[(name, kind)] -> ops: takes at 100:1s, replicas with clean non-zero states."""
    n = len(stream)
    a, t, e = _gen.clean_states(rng, n)
    return dict(names=[s[0] for s in stream], kind=np.array([s[1] for s in stream], np.uint8),
                now=T0 + np.cumsum(rng.integers(0, 2_000_000, n)).astype(np.int64),
                freq=np.full(n, 100, np.int64), per=np.full(n, SEC, np.int64),
                count=rng.integers(1, 3, n).astype(np.uint64), added=a, taken=t, elapsed=e)


SIZES = (32, 33, 32768, 32769)   # thread | wave boundary, wave | workgroup boundary


def test_segment_classes_all_take(pa):
    """Buckets of exactly 32, 33, 32768 and 32769 ops and some single ones,
    all TAKE: a host batch of one kind reads no kinds at all."""
    rng = np.random.default_rng(31)
    seqs = [[(b"seg%d" % c, EC.TAKE)] * c for c in SIZES]
    seqs += [[(b"one%d" % i, EC.TAKE)] for i in range(100)]
    ops = build_ops(rng, interleave(rng, seqs))
    res = run_case(pa, ops, log2_slots=10)
    assert res["egress"]["n_incast"] == len(seqs)


def test_segment_classes_mixed(pa):
    """The same sizes with every op a RECEIVE but each bucket's last, a TAKE:
    the thread walk, the wave ballot and the workgroup vote must each find the
    one op that asks for a datagram.  RECEIVE-only buckets of the long and huge
    classes send nothing; a bucket a TAKE created, merged into by 40 RECEIVEs,
    sends its request and its state."""
    rng = np.random.default_rng(32)
    seqs = [[(b"seg%d" % c, EC.RECEIVE)] * (c - 1) + [(b"seg%d" % c, EC.TAKE)] for c in SIZES]
    seqs += [[(b"quiet40", EC.RECEIVE)] * 40, [(b"quiet33000", EC.RECEIVE)] * 33000]
    seqs += [[(b"made", EC.TAKE)] + [(b"made", EC.RECEIVE)] * 40]
    seqs += [[(b"one%d" % i, (EC.TAKE, EC.RECEIVE, EC.UPSERT)[i % 3])] for i in range(99)]
    ops = build_ops(rng, interleave(rng, seqs))
    res = run_case(pa, ops, log2_slots=10)
    req, st = EC.sections(res["egress"])
    assert b"quiet40" not in st and b"quiet33000" not in st
    assert all(b"seg%d" % c in st and b"seg%d" % c not in req for c in SIZES)
    assert b"made" in req and b"made" in st


# ------------------------------------------------------------------ tile edges --
def tile_names(k):
    L = (5, 14, 22, 23, 40)[k % 5]
    return (b"%05d" % k).ljust(L, b"t")


@pytest.mark.parametrize("K,mixed", [(4095, False), (4096, False), (4097, True), (8193, True)])
def test_tile_edges(pa, K, mixed):
    """K distinct buckets named once each, every other one new: both sections
    end at, or one past, a tile of 4096 segments (8193: two tiles and one)."""
    rng = np.random.default_rng(K)
    names = [tile_names(k) for k in range(K)]
    prior = build_ops(rng, [(nm, EC.TAKE) for nm in names[::2]])
    kinds = [(EC.UPSERT if mixed and k % 7 == 3 else EC.TAKE) for k in range(K)]
    order = rng.permutation(K)
    ops = build_ops(rng, [(names[k], kinds[k]) for k in order])
    ops["now"] += int(prior["now"][-1]) - T0
    res = run_case(pa, ops, prior=prior, log2_slots=15)
    assert res["egress"]["n"] - res["egress"]["n_incast"] == K


# ------------------------------------------------------- collisions, growth --
def test_tag_collisions(pa):
    rng = np.random.default_rng(41)
    run_case(pa, EC.gen_ops(rng, 3000, EC.name_pool(200)), log2_slots=12, debug_tag_bits=3)


def test_table_grows_inside_the_batch(pa):
    """16 slots at open: the batch's new buckets rehash the table more than
    once, and the datagrams come from the re-resolved slots."""
    rng = np.random.default_rng(42)
    g = pa.GPURepo(log2_slots=4)
    assert g.capacity == 16
    g.close()
    run_case(pa, EC.gen_ops(rng, 3000, EC.name_pool(300)), log2_slots=4)


# -------------------------------------------------------------------- caps --
def test_caps_refusal_leaves_everything_untouched(pa):
    import ctypes as C
    from patrol_amd import _lib
    from patrol_amd.engine import names_blob
    rng = np.random.default_rng(51)
    pool = EC.name_pool(60)
    prior = EC.gen_ops(rng, 200, pool)
    ops = EC.gen_ops(rng, 500, pool, t0=int(prior["now"][-1]))
    g = pa.GPURepo(log2_slots=10)
    plain(g, prior)
    before, len_before = gpu_dump(g), len(g)
    n = len(ops["names"])
    blob, offs = names_blob(ops["names"])
    cols = {c: np.ascontiguousarray(ops[c]) for c in COLS}
    o = _lib.phip_ops(n, 0, cols["kind"].ctypes.data, blob.ctypes.data, offs.ctypes.data,
                      *[cols[c].ctypes.data for c in COLS[1:]])
    max_msgs, cap = g.egress_caps(n, int(offs[n]))
    status = np.full(n, 0xEE, np.uint8)
    res = _lib.phip_results(status.ctypes.data, None, None, None)
    data = np.full(cap, 0xEE, np.uint8)
    eoffs = np.full(max_msgs + 1, 0xEE, np.uint64)
    for mm, cc in ((max_msgs - 1, cap), (max_msgs, cap - 1)):
        eg = _lib.phip_egress(data.ctypes.data, cc, eoffs.ctypes.data, mm, 7, 7, 0, 7)
        rc = g.L.phip_apply_mixed_egress(g.h, C.byref(o), C.byref(res), C.byref(eg), 0)
        assert rc == -1, (mm, cc, rc)
        assert (eg.n, eg.n_incast, eg.bytes) == (0, 0, 0)
        assert np.all(status == 0xEE) and np.all(data == 0xEE) and np.all(eoffs == eoffs[0])
        assert gpu_dump(g) == before and len(g) == len_before
    # the device form: one 8-byte granule short, and a misaligned buffer
    import torch
    dev = torch.device("cuda", 0)
    t = to_device(ops)
    dm, dc = g.egress_caps(n, int(t["names"].numel()), device=True)
    out = torch.zeros(dc + 8, dtype=torch.uint8, device=dev)
    doffs = torch.zeros(dm + 1, dtype=torch.int64, device=dev)
    args = dict(freq=t["freq"], per=t["per"], count=t["count"], added=t["added"], taken=t["taken"],
                elapsed=t["elapsed"])
    for buf, cc, mm in ((out, dc - 8, dm), (out, dc, dm - 1), (out[1:], dc, dm)):
        with pytest.raises(pa.PatrolHipError) as e:
            g.apply_mixed_egress_device(n, t["kind"], t["names"], t["name_offs"], t["now"], buf,
                                        doffs, mm, out_cap=cc, **args)
        assert e.value.code == -1
        assert gpu_dump(g) == before and len(g) == len_before
    assert int(out.sum()) == 0 and int(doffs.sum()) == 0
    # and the exact caps pass
    r = g.apply_mixed_egress_device(n, t["kind"], t["names"], t["name_offs"], t["now"], out, doffs,
                                    dm, out_cap=dc, **args)
    assert r["n"] > 0
    g.close()


# -------------------------------------------------------------- round trip --
def test_round_trip_into_a_peer(pa):
    """Monotone TAKE-only inputs (tests/test_egress_abi.py shows the premise on
    the oracle): the device buffers go unchanged into a second handle's
    receive_datagrams_device, and that peer's table equals an oracle peer that
    received the reference's per-op broadcasts."""
    rng = np.random.default_rng(61)
    ops = EC.monotone_takes(rng, 6000, 800)
    g, peer, o = pa.GPURepo(log2_slots=12), pa.GPURepo(log2_slots=12), O.Repo()
    eg, out, offs, _ = device_egress(g, ops)
    ref = EC.call(o, ops)
    EC.assert_monotone(ops, ref)
    check_egress(eg, ops, ref, o.dump())
    now = int(ops["now"][-1]) + 1
    stop = peer.receive_datagrams_device(out, offs, eg["n"], now)
    assert stop == eg["n"]
    want = O.Repo()
    per_op = EC.per_op_broadcasts(ops, ref)
    assert want.receive(per_op, now)[4] == len(per_op)
    assert gpu_dump(peer) == want.dump()
    g.close()
    peer.close()


# ----------------------------------------------------------------- batcher --
def test_batcher_egress(pa):
    """16 threads x 200 takes over 50 buckets, two egress slots, one drainer."""
    threads, per_thread, K = 16, 200, 50
    repo = pa.GPURepo(log2_slots=10)
    b = pa.TakeBatcher(repo, window_us=200, max_batch=1024, egress_slots=2)
    rng = np.random.default_rng(71)
    plan = []
    for tid in range(threads):
        ids = _gen.zipf_ids(rng, per_thread, K)
        cnt = rng.integers(1, 4, per_thread)
        now = T0 + np.sort(rng.integers(0, 5 * SEC, per_thread))
        plan.append([(b"b%d" % ids[k], int(now[k]), 100, SEC, int(cnt[k]))
                     for k in range(per_thread)])
    results = [[] for _ in range(threads)]
    drained = []
    takers_done = threading.Event()

    def worker(tid):
        for req in plan[tid]:
            r = b.take_reply(*req)
            results[tid].append((r["seq"], req, r["remaining"], r["ok"], r["created"]))

    def drainer():
        while True:
            e = b.egress_next(50)
            if e is None:
                if takers_done.is_set():
                    return
                continue
            drained.append(e)
            b.egress_done(e["batch"])

    dt = threading.Thread(target=drainer)
    dt.start()
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    takers_done.set()   # (a take returns only once its batch's egress is queued)
    dt.join()
    st = b.stats()
    allr = sorted(r for rs in results for r in rs)
    n = threads * per_thread
    assert [r[0] for r in allr] == list(range(n))
    assert st["requests"] == n and st["errors"] == 0
    # today's arrival-order check: the oracle one request at a time in seq order
    o = O.Repo()
    ref = o.apply_mixed(np.zeros(n, np.uint8), [r[1][0] for r in allr],
                        np.array([r[1][1] for r in allr], np.int64),
                        np.array([r[1][2] for r in allr], np.int64),
                        np.array([r[1][3] for r in allr], np.int64),
                        np.array([r[1][4] for r in allr], np.uint64),
                        np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int64))
    assert [r[2] for r in allr] == [int(x) for x in ref["remaining"]]
    assert [r[3] for r in allr] == [(int(s) & 0x7F) == 6 for s in ref["status"]]
    assert [r[4] for r in allr] == [bool(int(s) & 0x80) for s in ref["status"]]
    # the drained batches: consecutive numbers, in arrival order, counted by the stats
    assert [e["batch"] for e in drained] == list(range(len(drained)))
    assert [e["first_seq"] for e in drained] == sorted(e["first_seq"] for e in drained)
    assert sum(e["requests"] for e in drained) == n
    assert st["egress_batches"] == len(drained)
    assert st["egress_datagrams"] == sum(e["n"] for e in drained)
    # requests: the created buckets, each once; states: a later batch overrides
    reqs, states = [], {}
    for e in drained:
        rq, stt = EC.sections(e)
        reqs += list(rq)
        states.update(stt)
    taken = {r[1][0] for r in allr}
    assert sorted(reqs) == sorted(taken)
    dump = gpu_dump(repo)
    assert dump == o.dump()
    assert states == {nm: EC.marshal(nm, *dump[nm][:3]) for nm in taken}
    # close() with a blocked egress_next returns, and so does the call
    got = []
    blocked = threading.Thread(target=lambda: got.append(b.egress_next(-1)))
    blocked.start()
    b.close()
    blocked.join(30)
    assert not blocked.is_alive() and got == [None]
    # a plain batcher on the same handle still serves take_reply as before
    b2 = pa.TakeBatcher(repo)
    r = b2.take_reply(b"b0", T0 + 6 * SEC, 100, SEC, 1)
    st2 = repo.get(b"b0")
    assert r["datagram"] == EC.marshal(b"b0", st2.added, st2.taken, st2.elapsed)
    assert b2.stats()["egress_batches"] == 0
    with pytest.raises(pa.PatrolHipError):
        b2.egress_next(0)
    b2.close()
    repo.close()
