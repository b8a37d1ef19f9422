"""Owner-routed Take and mixed ops over the shard group (phip_route_pack_ops,
phip_group_apply_mixed) on one GPU, bit-exact against the oracle run over
all ops in (round, source rank, index) order (tests/_group_ops.py): the
stable owner partition itself, world 1 in both group forms with and without
the RCCL self-exchange, shared-device groups of world 2 and 3, the order of
sources on one hot bucket, many small rounds, Receive and apply_mixed taking
turns on one group, a corrupted offset column and the flag checks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import go_semantics as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _group_ops as GO  # noqa: E402


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


DEV = torch.device("cuda", 0)
POOL = GO.name_pool(400)
_owners = GO.owners


def _dev(b, drop=()):
    """A host batch (GO.gen_ops) as the dict of CUDA tensors the binding takes."""
    from patrol_amd.engine import names_blob
    blob, offs = names_blob(b["names"])
    d = dict(names=torch.from_numpy(blob).to(DEV), name_offs=torch.from_numpy(offs.view(np.int32)).to(DEV))
    for c in GO.COLS:
        if c in drop:
            d[c] = None
            continue
        x = np.ascontiguousarray(b[c])
        x = x.view(np.int64) if x.dtype == np.uint64 else x
        d[c] = torch.from_numpy(x if x.size else np.zeros(1, x.dtype)).to(DEV)
    return d


def _dump(repo):
    return {k: (v.added, v.taken, v.elapsed, v.created) for k, v in repo.dump().items()}


def _union(repos, world=None):
    got = {}
    for r, repo in enumerate(repos):
        d = _dump(repo)
        if world is not None and d:   # every bucket lies on its owner
            assert (_owners(list(d), world) == r).all()
        got.update(d)
    return got


def _check(out, want, b, tag=""):
    """One member's four result columns against the oracle's.  `have` is a
    TAKE output and the reply is defined under GO.reply_mask (zeros
    elsewhere: patrolhip.h), as the single-handle parity tests compare them."""
    st = out["status"].cpu().numpy()
    bad = np.nonzero(st != want["status"])[0]
    assert bad.size == 0, (tag, "status", int(bad[0]), int(st[bad[0]]), int(want["status"][bad[0]]))
    rem = out["remaining"].cpu().numpy().view(np.uint64)
    bad = np.nonzero(rem != want["remaining"])[0]
    assert bad.size == 0, (tag, "remaining", int(bad[0]))
    take = b["kind"] == 0
    have = out["have"].cpu().numpy().view(np.uint64)
    assert np.array_equal(have[take], want["have"][take]), (tag, "have")
    rep = GO.reply_mask(b["kind"], want["status"])
    reply = out["reply"].cpu().numpy()
    bad = np.nonzero((reply[rep] != want["reply"][rep]).any(axis=1))[0]
    assert bad.size == 0, (tag, "reply", int(np.nonzero(rep)[0][bad[0]]))
    assert not reply[~rep].any(), (tag, "reply of a merged replica")


# ------------------------------------------------------------- the partition --
@pytest.fixture(scope="module")
def pack_repo(pa):
    repo = pa.GPURepo(log2_slots=10)
    yield repo
    repo.close()


_PACK_BATCH = {}


def _pack_batch(n):
    if n not in _PACK_BATCH:
        rng = np.random.default_rng(4000 + n)
        b = GO.gen_ops(rng, n, POOL)
        bt = GO.gen_ops(rng, n, POOL, all_take=True)
        _PACK_BATCH[n] = (b, _dev(b), bt, _dev(bt, drop=("added", "taken", "elapsed")))
    return _PACK_BATCH[n]


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 5000])
def test_route_pack_ops_is_stable_owner_partition(pa, pack_repo, n, world):
    """send_src is the stable argsort of the owners; every send column is the
    input gathered through it, the operand words chosen by kind; counts /
    name_bytes are the per-owner sums; the packed names are byte-identical.
    512 ops are one scatter step, so 511 / 513 straddle it.  An all-TAKE batch
    passed without added / taken / elapsed packs its freq / per / count."""
    b, d, bt, dt = _pack_batch(n)
    for tag, hb, db in (("mixed", b, d), ("all-take, NULL state columns", bt, dt)):
        out = pack_repo.route_pack_ops_device(n, world, **db)
        own = _owners(hb["names"], world)
        src = np.argsort(own, kind="stable")
        assert np.array_equal(out["src"].cpu().numpy()[:n], src), tag
        take = hb["kind"] == 0
        lens = np.array([len(x) for x in hb["names"]], np.int64)
        want = dict(kind=hb["kind"], now=hb["now"], lens=lens,
                    x0=np.where(take, hb["freq"].view(np.uint64), hb["added"]),
                    x1=np.where(take, hb["per"].view(np.uint64), hb["taken"]),
                    x2=np.where(take, hb["count"], hb["elapsed"].view(np.uint64)))
        for c, w in want.items():
            got = out[c].cpu().numpy()[:n]
            got = got.view(np.uint64) if c in ("x0", "x1", "x2") else got
            assert np.array_equal(got.astype(w.dtype), w[src]), (tag, c)
        if tag != "mixed" and n:   # no operand word of a Take reads as zero
            assert out["x0"][:n].all() and out["x1"][:n].all() and out["x2"][:n].all()
        assert np.array_equal(out["counts"].cpu().numpy(), np.bincount(own, minlength=world)), tag
        assert np.array_equal(out["name_bytes"].cpu().numpy(),
                              np.bincount(own, weights=lens, minlength=world).astype(np.int64)), tag
        packed = b"".join(hb["names"][j] for j in src)
        assert out["names"].cpu().numpy()[:len(packed)].tobytes() == packed, tag


# ------------------------------------------------------------------ world 1 --
@pytest.mark.parametrize("mode,rccl_self", [("all", False), ("rank", False), ("all", True),
                                            ("rank", True)])
def test_group_apply_mixed_world1_vs_oracle(pa, mode, rccl_self):
    """3000 mixed ops over 400 buckets through a group of one, straight to
    phip_apply_mixed or (rccl_self) through the pack, the RCCL exchange to
    itself, the apply, the results' way back and the scatter."""
    rng = np.random.default_rng(5100)
    if mode == "all":
        g = pa.GPUGroup.open_all([0], log2_slots=12)
        repo = g.repos[0]
    else:
        repo = pa.GPURepo(log2_slots=12)
        g = pa.GPUGroup.open_rank(repo, pa.GPUGroup.unique_id(), 1, 0)
    n = 3000
    b = GO.gen_ops(rng, n, POOL)
    o = O.Repo()
    want = GO.oracle_results(o, [b], GO.apply_order([n]))
    out, sent, applied = g.apply_mixed([_dev(b)], rccl_self=rccl_self)
    _check(out[0], want[0], b)
    assert sent == [n] and applied == [n]
    assert _dump(repo) == o.dump()
    g.close()
    if mode == "rank":
        repo.close()


# ------------------------------------------------------------ shared device --
@pytest.mark.parametrize("world,sizes", [(2, (2700, 0)), (3, (2000, 0, 3000))])
def test_shared_device_group_apply_mixed_vs_oracle(pa, world, sizes):
    """`world` shards on one GPU, member i submitting its own batch (one of
    them empty): every member's results equal the oracle's under the order
    rule, every bucket lies on its owner, the tables together are the
    oracle's, and exactly one op per new bucket carries PHIP_ST_CREATED."""
    rng = np.random.default_rng(5200 + world)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=12)
    bs = [GO.gen_ops(rng, n, POOL, t0=_gen.T0 + 1000 * i) for i, n in enumerate(sizes)]
    o = O.Repo()
    want = GO.oracle_results(o, bs, GO.apply_order(sizes))
    out, sent, applied = g.apply_mixed([_dev(b) for b in bs])
    for i in range(world):
        _check(out[i], want[i], bs[i], "member %d" % i)
    assert sent == list(sizes) and sum(applied) == sum(sizes)
    tables = _union(g.repos, world)
    assert tables == o.dump()
    created = [nm for i in range(world)
               for nm, s in zip(bs[i]["names"], out[i]["status"].cpu().numpy()) if s & 0x80]
    assert sorted(created) == sorted(tables)
    g.close()


def test_group_apply_mixed_hot_bucket_order_across_sources(pa):
    """Three members, 600 Takes of 1 each on one bucket at 1000:1h with equal
    `now`: the bucket runs dry partway through member 1's ops, so source rank
    alone decides which Takes are denied."""
    world, n = 3, 600
    g = pa.GPUGroup.open_all([0] * world, log2_slots=10)

    def batch():
        return dict(names=[b"hot-bucket"] * n, kind=np.zeros(n, np.uint8),
                    now=np.full(n, _gen.T0, np.int64), freq=np.full(n, 1000, np.int64),
                    per=np.full(n, 3600 * _gen.SEC, np.int64), count=np.ones(n, np.uint64),
                    added=np.zeros(n, np.uint64), taken=np.zeros(n, np.uint64),
                    elapsed=np.zeros(n, np.int64))
    bs = [batch() for _ in range(world)]
    o = O.Repo()
    want = GO.oracle_results(o, bs, GO.apply_order([n] * world))
    out, _, _ = g.apply_mixed([_dev(b) for b in bs])
    ok = []
    for i in range(world):
        _check(out[i], want[i], bs[i], "member %d" % i)
        ok.append((out[i]["status"].cpu().numpy() & 0x7F) == 6)
    assert ok[0].all() and not ok[2].any()
    assert ok[1][:400].all() and not ok[1][400:].any()
    rem = np.concatenate([out[i]["remaining"].cpu().numpy()[ok[i]] for i in range(world)])
    assert np.array_equal(rem, np.arange(999, -1, -1))   # no gap across the member boundary
    assert _union(g.repos, world) == o.dump()
    g.close()


@pytest.mark.parametrize("world", [2, 1])
def test_group_apply_mixed_small_chunks_round_order(pa, world):
    """Rounds of 4096 ops: 9000 and 5000 ops give 3 and 2 rounds, so the
    shorter member sends an empty round, and the hottest bucket is named in
    every round by both members.  World 1 runs the same rounds through the
    RCCL exchange to itself."""
    rng = np.random.default_rng(5500)
    sizes = (9000, 5000)[:world]
    bs = [GO.gen_ops(rng, n, POOL, t0=_gen.T0 + 1000 * i) for i, n in enumerate(sizes)]
    order = GO.apply_order(sizes, GO.SMALL_CHUNK)
    o = O.Repo()
    want = GO.oracle_results(o, bs, order)
    if world == 2:
        hot = max(set(bs[0]["names"]), key=bs[0]["names"].count)
        for b, n in zip(bs, sizes):
            for lo in range(0, n, GO.SMALL_CHUNK):
                assert hot in b["names"][lo:lo + GO.SMALL_CHUNK]
        # the test can tell the orders apart: (rank, index) gives other results
        other = GO.oracle_results(O.Repo(), bs, GO.rank_order(sizes))
        assert any(not np.array_equal(other[i]["status"], want[i]["status"]) or
                   not np.array_equal(other[i]["remaining"], want[i]["remaining"])
                   for i in range(world))
        g = pa.GPUGroup.open_all([0, 0], log2_slots=12)
        out, sent, applied = g.apply_mixed([_dev(b) for b in bs], small_chunks=True)
    else:
        g = pa.GPUGroup.open_all([0], log2_slots=12)
        out, sent, applied = g.apply_mixed([_dev(b) for b in bs], rccl_self=True, small_chunks=True)
    for i in range(world):
        _check(out[i], want[i], bs[i], "member %d" % i)
    assert sent == list(sizes) and sum(applied) == sum(sizes)
    assert _union(g.repos, world) == o.dump()
    g.close()


def _msgs(rng, n):
    """n clean Receive messages over POOL: host columns and the tuple of CUDA
    tensors GPUGroup.receive takes (an empty batch keeps one-entry columns)."""
    from patrol_amd.engine import names_blob
    names = [POOL[int(i)] for i in _gen.zipf_ids(rng, n, len(POOL))] if n else []
    a, t, e = _gen.clean_states(rng, n)
    blob, offs = names_blob(names)
    cols = [blob if blob.size else np.zeros(8, np.uint8), offs.view(np.int32)]
    cols += [x.view(np.int64) if x.size else np.zeros(1, np.int64) for x in (a, t, e)]
    return names, a, t, e, tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in cols)


@pytest.mark.parametrize("world", [2, 1])
def test_group_receive_and_apply_mixed_interleaved(pa, world):
    """Receive, apply_mixed, Receive, apply_mixed on one group, in rounds of
    4096: both calls run the same exchange steps over the member's scan and
    bounds scratch, each over its own column sets.  Two shards on one GPU
    (9000 / 0 then 0 / 5000 messages, 9000 / 5000 ops: an empty member, both
    set parities, uneven round counts) and world 1 through the RCCL exchange
    to itself.  Every result column, the totals and the tables equal the
    oracle's under each call's order rule, and the stage timer of an
    apply_mixed call reads back for every member."""
    rng = np.random.default_rng(5800 + world)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=12)
    kw = dict(small_chunks=True, rccl_self=world == 1)
    g.set_timing(True)
    o = O.Repo()
    chunk = GO.SMALL_CHUNK

    def receive(sizes, now):
        per = [_msgs(rng, n) for n in sizes]
        sent, merged = g.receive([b[4] for b in per], now, **kw)
        assert sent == list(sizes) and sum(merged) == sum(sizes)
        # chunk by chunk, sources in rank order within a chunk
        for c in range(max((n + chunk - 1) // chunk for n in sizes)):
            for b, n in zip(per, sizes):
                if c * chunk < n:
                    sl = slice(c * chunk, min(n, (c + 1) * chunk))
                    o.receive_soa(b[0][sl], b[1][sl], b[2][sl], b[3][sl], now)

    def apply(sizes, t0, tag):
        bs = [GO.gen_ops(rng, n, POOL, t0=t0 + 1000 * i) for i, n in enumerate(sizes)]
        want = GO.oracle_results(o, bs, GO.apply_order(sizes, chunk))
        out, sent, applied = g.apply_mixed([_dev(b) for b in bs], **kw)
        for i in range(world):
            _check(out[i], want[i], bs[i], "%s, member %d" % (tag, i))
            ms = g.stage_ms(i)
            assert len(ms) == 3 and all(np.isfinite(v) and v >= 0 for v in ms.values()), (tag, i, ms)
        assert sent == list(sizes) and sum(applied) == sum(sizes)

    receive((9000, 0)[:world], _gen.T0)
    apply((9000, 5000)[:world], _gen.T0 + _gen.SEC, "first")
    receive((0, 5000)[-world:], _gen.T0 + 10**12)
    apply((9000, 5000)[:world], _gen.T0 + 10**12 + _gen.SEC, "second")
    assert _union(g.repos, world) == o.dump()
    g.close()


def test_group_apply_mixed_rejects_corrupted_offsets(pa):
    """One entry of member 1's name_offs past names_len: PHIP_ERR_INVALID
    naming member 1 and the op, both tables as they were, every status 0, and
    a following valid call on the same group matches the oracle."""
    rng = np.random.default_rng(5600)
    world, n, k = 2, 3000, 1777
    g = pa.GPUGroup.open_all([0] * world, log2_slots=12)
    o = O.Repo()
    bs = [GO.gen_ops(rng, n, POOL) for _ in range(world)]
    want = GO.oracle_results(o, bs, GO.apply_order([n] * world))
    out, _, _ = g.apply_mixed([_dev(b) for b in bs])
    for i in range(world):
        _check(out[i], want[i], bs[i], "first call, member %d" % i)
    before = [_dump(r) for r in g.repos]
    bs = [GO.gen_ops(rng, n, POOL, t0=_gen.T0 + 10**12) for _ in range(world)]
    ds = [_dev(b) for b in bs]
    good = int(ds[1]["name_offs"][k])
    ds[1]["name_offs"][k] = 0x7FFF0000   # entries k-1 and k are malformed
    with pytest.raises(pa.PatrolHipError) as ei:
        g.apply_mixed(ds)
    assert ei.value.code == -1
    assert "member 1" in str(ei.value) and "op %d " % (k - 1) in str(ei.value)
    assert [_dump(r) for r in g.repos] == before
    ds[1]["name_offs"][k] = good
    want = GO.oracle_results(o, bs, GO.apply_order([n] * world))
    out, _, _ = g.apply_mixed(ds)
    for i in range(world):
        _check(out[i], want[i], bs[i], "repaired, member %d" % i)
    assert _union(g.repos, world) == o.dump()
    g.close()


def test_group_apply_mixed_flags(pa):
    """PHIP_DEVICE_PTRS is required and PHIP_ROUTE_COMBINE (any other bit) is
    refused: PHIP_ERR_INVALID, nothing applied."""
    from patrol_amd import _lib
    from patrol_amd.engine import GPUGroup, phip_ops, phip_results
    g = pa.GPUGroup.open_all([0, 0], log2_slots=10)
    b = GO.gen_ops(np.random.default_rng(5700), 100, POOL)
    ds = [_dev(b), _dev(b)]
    ops = (phip_ops * 2)()
    res = (phip_results * 2)()
    status = [torch.zeros(100, dtype=torch.uint8, device=DEV) for _ in range(2)]
    for i, d in enumerate(ds):
        ops[i] = phip_ops(100, d["names"].numel(), *[d[key].data_ptr() for key in GPUGroup._OPS_KEYS])
        res[i] = phip_results(status[i].data_ptr(), None, None, None)
    torch.cuda.synchronize()
    for flags in (0, _lib.GROUP_RCCL_SELF, _lib.DEVICE_PTRS | _lib.ROUTE_COMBINE,
                  _lib.DEVICE_PTRS | _lib.RECV_ASYNC):
        assert g.L.phip_group_apply_mixed(g.g, ops, res, None, None, flags) == -1
        assert all(len(r) == 0 for r in g.repos)
        assert not any(bool(s.any()) for s in status)
    assert g.L.phip_group_apply_mixed(g.g, ops, res, None, None, _lib.DEVICE_PTRS) == 0
    assert sum(len(r) for r in g.repos) == len(set(b["names"]))
    assert all(bool(s.all()) for s in status)
    g.close()
