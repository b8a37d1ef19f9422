"""Group reply egress (phip_group_receive_datagrams_replies,
phip_group_receive_replies, phip_group_ring_receive_replies,
phip_group_reply_stats): the shard group's answers to incast requests against
the model of tests/_group_replies_cases.py -- one oracle.Repo fed round by
round, sources in rank order, its reply columns marshalled with
patrol_amd.marshal.  rq of every member is compared byte for byte, and after
every case the tables equal the oracle's dump with every bucket on its owner.

One GPU: shared-device groups (open_all([0] * world)) and world 1 with
rccl_self, as tests/test_group_wire.py; the RCCL exchange at world > 1 needs
one GPU per member and is not run here."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _group_replies_cases as GC  # noqa: E402
from tests import _replies_cases as RC  # noqa: E402
from tests import _wire_cases as W  # noqa: E402

NOW = GC.NOW
BIG = dict(max_msgs=1 << 15)   # caps no case below reaches


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def _dev():
    return torch.device("cuda", 0)


def _dump(repo):
    return {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}


def _tables_equal_oracle(g, world, o):
    got = {}
    for r, repo in enumerate(g.repos):
        d = _dump(repo)
        for name in d:
            assert GC.owner(name, world) == r
        got.update(d)
    want = o.dump()
    assert len(got) == len(want)
    assert all(got.get(k) == v for k, v in want.items())


def _host(x, n):
    return x[:n].cpu().numpy() if torch.is_tensor(x) else np.asarray(x[:n])


def _same_rq(got, want, untouched=False):
    assert len(got) == len(want)
    for r, (q, e) in enumerate(zip(got, want)):
        assert (q["n"], q["replies"], q["skipped"], q["bytes"]) == \
            (e["n"], e["replies"], e["skipped"], e["bytes"]), r
        assert _host(q["data"], e["bytes"]).tobytes() == e["data"], r
        assert _host(q["offs"], e["n"] + 1).astype(np.uint64).tolist() == e["offs"].tolist(), r
        assert _host(q["src"], e["n"]).astype(np.uint32).tolist() == e["src"].tolist(), r
        if untouched:   # nothing past the cut
            assert not _host(q["data"], q["data"].numel())[e["bytes"]:].any(), r
            assert not _host(q["offs"], q["offs"].numel())[e["n"] + 1:].any(), r
            assert not _host(q["src"], q["src"].numel())[e["n"]:].any(), r


_built = {}


def _case(key, *a, **kw):
    """A built case, its model computed once; the oracle is not fed again."""
    if key not in _built:
        _built[key] = GC.build(*a, **kw)
    return _built[key]


def _open_warm(pa, b, world, **kw):
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    sent, merged, stopped = g.receive_datagrams(b["warm"], _gen.T0, **kw)
    assert g.last_rc == 0 and sum(sent) == sum(merged)
    return g


SIZES = {2: (9000, 4097), 3: (9000, 4097, 1)}


# ------------------------------------------ 1, 2. pipelined rounds vs model --
@pytest.mark.parametrize("world,sizes,rccl_self", [(2, SIZES[2], False), (3, SIZES[3], False),
                                                   (3, (9000, 0, 4097), False), (1, (9000,), True)])
def test_pipelined_rounds_equal_the_model(pa, world, sizes, rccl_self):
    """small_chunks: requests at index 0, 4095, 4096 and the last, to own and to
    foreign buckets; one bucket asked by two members in one round with the lower
    rank raising it in between; one asked in two successive rounds; arena-length
    names.  World 1 runs the same through RCCL both ways (rccl_self)."""
    b = _case(("pipe", world, sizes), world, sizes, 9100 + world)
    kw = dict(rccl_self=True) if rccl_self else {}
    g = _open_warm(pa, b, world, **kw)
    sent, merged, stopped, rq = g.receive_datagrams(b["per"], NOW, small_chunks=True, replies=BIG, **kw)
    assert g.last_rc == 0 and stopped == list(sizes) and sum(sent) == sum(merged) == sum(sizes)
    want = GC.expected(b["case"]["names"], b["cols"], world)
    _same_rq(rq, want)
    K = GC.rounds_of(sizes, GC.CHUNK)
    for r in range(world):
        s = g.reply_stats(r)
        assert s["rounds"] == K and 1 <= s["return_rounds"] <= K and s["bound"] >= s["written"]
    assert sum(g.reply_stats(r)["written"] for r in range(world)) == sum(e["n"] for e in want)
    _tables_equal_oracle(g, world, b["oracle"])
    g.close()


# --------------------------------------------------------- 3. world 1 plain --
def test_world_one_plain_equals_the_handle(pa):
    b = _case(("pipe", 1, (9000,)), 1, (9000,), 9101)
    g = _open_warm(pa, b, 1)
    twin = pa.GPURepo(log2_slots=14)
    twin.receive_datagrams(b["warm"][0], _gen.T0)
    sent, merged, stopped, rq = g.receive_datagrams(b["per"], NOW, replies=BIG)
    ref = twin.receive_datagrams_replies(b["per"][0], NOW)
    q = rq[0]
    assert q["n"] == ref["n"] > 40 and q["bytes"] == ref["bytes"]
    assert q["replies"] == ref["replies"] - ref["skipped"] and q["skipped"] == ref["skipped"]
    assert _host(q["data"], q["bytes"]).tobytes() == np.asarray(ref["data"]).tobytes()
    assert _host(q["offs"], q["n"] + 1).astype(np.uint64).tolist() == ref["offs"].tolist()
    assert _host(q["src"], q["n"]).astype(np.uint32).tolist() == ref["src"].tolist()
    assert _dump(g.repos[0]) == _dump(twin)
    g.close()
    twin.close()


# ------------------------------------------------- 4. the ordered suffix --
def test_one_round_half_requests(pa):
    """20 000 messages per member at world 2 in one round, half of them
    requests: over 4096 dirty messages reach each owner, past the deferred
    sub-batch's reach."""
    world, n = 2, 20000
    b = _case("half", world, (n, n), 9300, chunk=1 << 24, extra=n // 2)
    want = GC.expected(b["case"]["names"], b["cols"], world)
    assert min(e["n"] for e in want) > 4096
    g = _open_warm(pa, b, world)
    sent, merged, stopped, rq = g.receive_datagrams(b["per"], NOW, replies=BIG)
    assert g.last_rc == 0 and stopped == [n, n]
    _same_rq(rq, want)
    for r in range(world):
        s = g.reply_stats(r)
        assert s["rounds"] == 1 and s["return_rounds"] == 1 and s["bound"] >= s["written"] > 4096
    _tables_equal_oracle(g, world, b["oracle"])
    g.close()


# ------------------------------------------------------------------ 5. caps --
@pytest.mark.parametrize("cap", ["max_msgs", "bytes"])
def test_caps_cut_in_batch_order(pa, cap):
    world, sizes = 2, SIZES[2]
    b = _case(("pipe", world, sizes), world, sizes, 9100 + world)
    full = GC.expected(b["case"]["names"], b["cols"], world)[0]
    j = int(np.searchsorted(full["src"], GC.CHUNK)) + 3    # inside member 0's round 2
    assert 3 < j < full["n"] - 1
    if cap == "max_msgs":
        caps = dict(max_msgs=j)
        want = GC.expected(b["case"]["names"], b["cols"], world, max_msgs=j)
    else:
        budget = (int(full["offs"][j + 1]) - 1) // 8 * 8
        assert int(full["offs"][j]) <= budget < int(full["offs"][j + 1])
        caps = dict(max_msgs=1 << 15, out_cap=budget + 8)
        want = GC.expected(b["case"]["names"], b["cols"], world, budget=budget)
    assert want[0]["n"] == j < want[0]["replies"] == full["replies"]
    g = _open_warm(pa, b, world)
    sent, merged, stopped, rq = g.receive_datagrams(b["per"], NOW, small_chunks=True, replies=caps)
    _same_rq(rq, want, untouched=True)
    _tables_equal_oracle(g, world, b["oracle"])
    g.close()


# ------------------------------------------------------------ 6. no request --
def test_no_request_runs_no_return_round(pa):
    world, sizes = 3, (9000, 4097, 1)
    rng = np.random.default_rng(9400)
    per = []
    for n in sizes:
        names = [GC.bucket_name(int(k)) for k in _gen.zipf_ids(rng, n, 3000)]
        per.append(RC.wire(names, *_gen.clean_states(rng, n)))
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    twin = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    sent, merged, stopped, rq = g.receive_datagrams(per, NOW, small_chunks=True, replies=BIG)
    s2, m2, st2 = twin.receive_datagrams(per, NOW, small_chunks=True)
    assert (sent, merged, stopped) == (s2, m2, st2) and g.last_rc == 0
    for r, q in enumerate(rq):
        assert (q["n"], q["replies"], q["skipped"], q["bytes"]) == (0, 0, 0, 0)
        assert int(q["offs"][0]) == 0
        assert g.reply_stats(r) == dict(rounds=3, return_rounds=0, bound=0, written=0)
    o = O.Repo()
    GC.model(o, per, NOW, GC.CHUNK)
    _tables_equal_oracle(g, world, o)
    assert [_dump(r) for r in g.repos] == [_dump(r) for r in twin.repos]
    g.close()
    twin.close()


# ------------------------------------------------------------ 7. stop rule --
def test_stop_rule_keeps_the_answers_before_the_stop(pa):
    world, sizes, pos = 3, (6000, 9000, 3000), 5000
    warm = GC.warm_batches(world, 3000, 9500)
    case = GC.make_group_case(world, sizes, 9501)
    per = GC.datagrams(case)
    per[1][pos] = W.malformed("short", per[1][pos])
    asked = sorted(p for ps in case["tags"][1].values() for p in ps)
    assert asked[0] < pos < asked[-1]
    stops = [sizes[0], pos, sizes[2]]
    o = O.Repo()
    GC.model(o, warm, _gen.T0, 1 << 24)
    cols = GC.model(o, per, NOW, GC.CHUNK, stops=stops)
    want = GC.expected(case["names"], cols, world)
    assert want[1]["n"] > 4 and all(int(s) < pos for s in want[1]["src"])
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    g.receive_datagrams(warm, _gen.T0)
    sent, merged, stopped, rq = g.receive_datagrams(per, NOW, small_chunks=True, replies=BIG)
    assert g.last_rc == -5 and stopped == stops and sum(sent) == sum(merged) == sum(stops)
    _same_rq(rq, want)
    _tables_equal_oracle(g, world, o)
    g.close()


# ----------------------------------------------------- 8. checked offsets --
def test_refused_checked_batch_zeroes_every_rq(pa):
    world = 2
    b = _case(("pipe", world, SIZES[2]), world, SIZES[2], 9100 + world)
    g = _open_warm(pa, b, world)
    before = [_dump(r) for r in g.repos]
    ws = (pa._lib.phip_wire * world)()
    keep = []
    for i, d in enumerate(b["per"]):
        offs = np.zeros(len(d) + 1, np.int64)
        offs[1:] = np.cumsum([len(x) for x in d])
        blob = np.zeros((int(offs[-1]) + 15) // 8 * 8 + 4096, np.uint8)
        blob[:int(offs[-1])] = np.frombuffer(b"".join(d), np.uint8)
        if i == 1:
            offs[2000] = offs[2001] + 5    # decreasing, still inside the allocation
        t = (torch.from_numpy(blob).to(_dev()), torch.from_numpy(offs).to(_dev()))
        keep.append(t)
        ws[i] = pa._lib.phip_wire(len(d), 0, t[0].data_ptr(), t[1].data_ptr(), int(offs[-1]) + 8)
    torch.cuda.synchronize()
    rq, bufs = g._group_rq(BIG)
    for q in rq:
        q.n, q.replies, q.skipped, q.bytes = 7, 7, 7, 7
    sent, merged, stopped = (C.c_uint64 * world)(), (C.c_uint64 * world)(), (C.c_uint32 * world)()
    rc = g.L.phip_group_receive_datagrams_replies(g.g, ws, NOW, sent, merged, stopped, rq,
                                                  g._wire_flags(True, False, True))
    assert rc == -1 and "member 1" in g.L.phip_group_last_error(g.g).decode()
    for q in rq:
        assert (q.n, q.replies, q.skipped, q.bytes) == (0, 0, 0, 0)
    assert [_dump(r) for r in g.repos] == before
    g.close()


# ------------------------------------------------------------ 9. long names --
def test_names_over_231_bytes_are_skipped_at_their_owner(pa):
    world = 2
    b = _case("long", world, (3000, 3000), 9200, long_names=6)
    want = GC.expected(b["case"]["names"], b["cols"], world)
    assert sum(e["skipped"] for e in want) >= 12
    g = _open_warm(pa, b, world)
    sent, merged, stopped, rq = g.receive_datagrams(b["per"], NOW, small_chunks=True, replies=BIG)
    _same_rq(rq, want)
    _tables_equal_oracle(g, world, b["oracle"])
    g.close()


# --------------------------------------------------------------- 10. combine --
@pytest.mark.parametrize("requests", [50, 0])
def test_combine(pa, requests):
    """2^20 datagrams per member with combine=True.  With 50 requests a pack
    holds a zero state and combines nothing; a clean batch combines and answers
    nothing."""
    world, n, K = 2, 1 << 20, 3000
    rng = np.random.default_rng(9600 + requests)
    warm = GC.warm_batches(world, K, 9600)
    o = O.Repo()
    GC.model(o, warm, _gen.T0, 1 << 24)
    per, devs, names_per = [], [], []
    for r in range(world):
        names = [GC.bucket_name(int(k)) for k in _gen.zipf_ids(rng, n, K)]
        a, t, e = _gen.clean_states(rng, n)
        for p in rng.choice(n, requests, replace=False).tolist():
            names[p] = GC.bucket_name(int(rng.integers(0, K)))
            a[p], t[p], e[p] = 0, 0, 0
        blob, offs = W.wire_blob(names, a, t, e)
        W.check_against_marshal(pa, names, a, t, e, blob, offs, step=n // 20)
        per.append(W.datagram_list(blob, offs))
        devs.append((torch.from_numpy(blob).to(_dev()), torch.from_numpy(offs).to(_dev())))
        names_per.append(names)
    cols = GC.model(o, per, NOW, 1 << 24)
    want = GC.expected(names_per, cols, world)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    g.receive_datagrams(warm, _gen.T0)
    torch.cuda.synchronize()
    sent, merged, stopped, rq = g.receive_datagrams(devs, NOW, combine=True, replies=BIG)
    assert g.last_rc == 0 and stopped == [n] * world and sum(sent) == sum(merged)
    if requests:
        assert sum(e["n"] for e in want) == world * requests
        assert sum(merged) == world * n          # no pack combined
    else:
        assert sum(e["n"] for e in want) == 0 and sum(merged) < world * n
        assert all(g.reply_stats(r)["return_rounds"] == 0 for r in range(world))
    _same_rq(rq, want)
    _tables_equal_oracle(g, world, o)
    g.close()


# ------------------------------------------------------------------ 11. ring --
def test_ring_form(pa):
    world = 2
    b = _case("ring", world, (3000, 2500), 9700)
    want = GC.expected(b["case"]["names"], b["cols"], world)
    g = _open_warm(pa, b, world)
    rings = [pa.Ring(g.repos[i], nslots=2, max_msgs=4096) for i in range(world)]
    slots = []
    for i in range(world):
        slot, n = rings[i].fill(b["per"][i])
        rings[i].submit(slot, n)
        slots.append(slot)
    sent, merged, stopped, rq = g.ring_receive(rings, slots, NOW, small_chunks=True,
                                               replies=dict(max_msgs=4096))
    assert g.last_rc == 0 and stopped == [3000, 2500]
    assert all(isinstance(q["data"], np.ndarray) for q in rq)
    _same_rq(rq, want)
    for i, q in enumerate(rq):
        peers = np.random.default_rng(i).integers(0, 256, (len(b["per"][i]), pa._lib.PEER_BYTES)).astype(np.uint8)
        assert q["n"] > 10 and np.array_equal(pa.reply_peers(peers, q["src"]), peers[q["src"]])
    _tables_equal_oracle(g, world, b["oracle"])
    for i in range(world):     # the slots are free again: both can be acquired
        for _ in range(2):
            slot, n = rings[i].fill(b["per"][i][:3])
            rings[i].submit(slot, n)
    for r in rings:
        r.close()
    g.close()


# --------------------------------------------------------- 12. decoded form --
def test_decoded_form_equals_the_wire_form(pa):
    world, sizes = 2, SIZES[2]
    b = _case(("pipe", world, sizes), world, sizes, 9100 + world)
    want = GC.expected(b["case"]["names"], b["cols"], world)
    g = _open_warm(pa, b, world)
    dv = []
    for r in range(world):
        c = b["case"]
        nblob, noffs = pa.names_blob(c["names"][r])
        t = [torch.from_numpy(nblob).to(_dev()), torch.from_numpy(noffs.view(np.int32)).to(_dev())]
        t += [torch.from_numpy(np.ascontiguousarray(c[k][r]).view(np.int64)).to(_dev()) for k in ("a", "t", "e")]
        dv.append(t)
    torch.cuda.synchronize()
    sent, merged, rq = g.receive(dv, NOW, small_chunks=True, replies=BIG)
    assert sum(sent) == sum(merged) == sum(sizes)
    _same_rq(rq, want)
    _tables_equal_oracle(g, world, b["oracle"])
    g.close()
