"""The shard group fed from the wire (phip_route_pack_datagrams,
phip_group_receive_datagrams, phip_group_ring_receive): raw MarshalBinary
datagrams owner-routed to their shards with no decoded copy, against the
oracle's Receive of the same datagrams (repo.go:54-92), a numpy restatement of
the stable owner partition, and phip_route_pack of the same messages decoded
on the host.  One GPU: shared-device groups (open_all([0] * world)) and world 1
with rccl_self, as tests/test_group.py.

The datagrams come from tests/_wire_cases.wire_blob (MarshalBinary vectorised,
pinned to patrol_amd.marshal on a sample of every batch) plus hand-made
malformed ones.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import go_semantics as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _wire_cases as W  # noqa: E402

CHUNK = 4096   # PHIP_GROUP_SMALL_CHUNKS


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


def _owner(name, world):
    from patrol_amd import shard
    h = torch.tensor([int(np.array([G.fnv1a64(name)], np.uint64).view(np.int64)[0])])
    return int(shard.owner_of(h, world))


def _union_on_owners(g, world):
    """The members' tables together, every bucket checked to lie on its owner."""
    got = {}
    for r, repo in enumerate(g.repos):
        d = _dump(repo)
        for name in d:
            assert _owner(name, world) == r
        got.update(d)
    return got


def _same(got, want):
    assert len(got) == len(want)
    assert all(got.get(k) == v for k, v in want.items())


def _upload(blob, offs):
    return torch.from_numpy(blob).to(_dev()), torch.from_numpy(offs).to(_dev())


def _zipf_batch(pa, rng, n, K, dirty=0.0):
    """n datagrams over Zipf names (test_group._batch's mix) -> (datagram list, device pair)."""
    ids = _gen.zipf_ids(rng, n, K)
    names = [(b"an-arena-length-bucket-name-%d" % i) if i % 97 == 0 else b"b%d" % i for i in ids]
    a, t, e = _gen.dirty_states(rng, n, dirty) if dirty else _gen.clean_states(rng, n)
    blob, offs = W.wire_blob(names, a, t, e)
    W.check_against_marshal(pa, names, a, t, e, blob, offs, step=max(1, n // 50))
    return dict(names=names, a=a, t=t, e=e, dgrams=W.datagram_list(blob, offs), dev=_upload(blob, offs))


def _empty_pair():
    return (torch.zeros(8, dtype=torch.uint8, device=_dev()), torch.zeros(1, dtype=torch.int64, device=_dev()))


# ------------------------------------------------------------ 1. the pack --
PACK_LENS = (0, 1, 14, 15, 16, 17, 22, 23, 100, 231)
_pack_cache = {}


def _pack_batch(pa, n):
    """Names of every length class (short, staged, byte-wise, arena), fields of
    _gen.dirty_states (-0.0, zero states, NaN, negatives), a tenth of the
    datagrams with 1-7 trailing junk bytes; the last datagram ends at the
    buffer's last byte before the slack to the next 8-byte boundary."""
    if n in _pack_cache:
        return _pack_cache[n]
    rng = np.random.default_rng(4100 + n)
    ids = rng.integers(0, 3000, n)
    names = []
    for i in ids.tolist():
        L = PACK_LENS[i % len(PACK_LENS)]
        names.append(bytes([i % 251]) if L == 1 else ((b"%07d-" % i) * 29)[:L])
    a, t, e = _gen.dirty_states(rng, n)
    junk = np.where(rng.random(n) < 0.1, rng.integers(1, 8, n), 0)
    junk[-1] = 0
    blob, offs = W.wire_blob(names, a, t, e, junk, rng)
    W.check_against_marshal(pa, names, a, t, e, blob, offs, junk, step=101)
    assert blob.size == (int(offs[-1]) // 8 + 1) * 8
    assert set((offs[:-1] % 8).tolist()) == set(range(8))   # every start alignment
    assert {len(x) for x in names} == set(PACK_LENS)
    hashes = {nm: G.fnv1a64(nm) for nm in set(names)}
    h = np.array([hashes[nm] for nm in names], np.uint64)
    nblob, noffs = pa.names_blob(names)
    b = dict(names=names, a=a, t=t, e=e, h=h, lens=np.fromiter((len(x) for x in names), np.int64, n),
             dev=_upload(blob, offs), nblob=nblob, noffs=noffs)
    _pack_cache[n] = b
    return b


@pytest.mark.parametrize("world", [1, 3, 8, 64])
@pytest.mark.parametrize("n", [5000, 70001])
def test_pack_datagrams_equals_restatement_and_decoded_pack(pa, n, world):
    """All seven outputs of phip_route_pack_datagrams (combine off), byte for
    byte, against (a) a numpy stable partition by owner = shard.owner_of(
    go_semantics.fnv1a64(name)) written here and (b) phip_route_pack of the same
    messages decoded on the host."""
    from patrol_amd import shard
    b = _pack_batch(pa, n)
    repo = pa.GPURepo(log2_slots=10)
    data, offs = b["dev"]
    got = repo.route_pack_datagrams_device(data, offs, n, world, combine=False)
    assert got["stop"] == n
    # (a) the restatement
    own = shard.owner_of(torch.from_numpy(b["h"].view(np.int64)), world).numpy()
    order = np.argsort(own, kind="stable")
    want_names = b"".join(b["names"][i] for i in order.tolist())
    cnt = np.bincount(own, minlength=world)
    nby = np.bincount(own, weights=b["lens"], minlength=world).astype(np.int64)
    assert got["counts"].cpu().numpy().tolist() == cnt.tolist()
    assert got["name_bytes"].cpu().numpy().tolist() == nby.tolist()
    assert got["lens"].cpu().numpy()[:n].tolist() == b["lens"][order].tolist()
    assert got["names"].cpu().numpy()[:len(want_names)].tobytes() == want_names
    for key in ("a", "t", "e"):
        col = got[{"a": "added", "t": "taken", "e": "elapsed"}[key]].cpu().numpy()[:n]
        assert col.tobytes() == np.ascontiguousarray(b[key][order]).tobytes()
    # (b) the decoded pack of the same messages
    dv = [torch.from_numpy(b["nblob"]).to(_dev()), torch.from_numpy(b["noffs"].view(np.int32)).to(_dev())]
    dv += [torch.from_numpy(np.ascontiguousarray(b[k]).view(np.int64)).to(_dev()) for k in ("a", "t", "e")]
    torch.cuda.synchronize()
    ref = shard.route_pack_native(*dv, repo, world, combine=False)
    torch.cuda.synchronize()
    keys = ("names", "lens", "added", "taken", "elapsed", "counts", "name_bytes")
    for key, r in zip(keys, ref):
        m = len(want_names) if key == "names" else r.numel() if key in ("counts", "name_bytes") else n
        assert torch.equal(got[key][:m].cpu(), r[:m].cpu()), key
    repo.close()


# ---------------------------------------------------- 2. group vs oracle --
@pytest.mark.parametrize("world,dirty", [(2, 0.0), (2, 0.05), (3, 0.0), (3, 0.05)])
def test_group_receive_datagrams_vs_oracle(pa, world, dirty):
    """Two calls (3 000 and 2^20 datagrams per member, the combine's threshold
    and the first size with several scatter steps per tile) with combine=True:
    every bucket on its owner, the tables together equal the oracle's Receive of
    member 0's datagrams, then 1's, ..., `created` included."""
    rng = np.random.default_rng(7100 + world)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    o = O.Repo()
    for k, n in enumerate((3000, 1 << 20)):
        per = [_zipf_batch(pa, rng, n, 30000, dirty) for _ in range(world)]
        torch.cuda.synchronize()
        sent, merged, stopped = g.receive_datagrams([b["dev"] for b in per], _gen.T0 + k, combine=True)
        assert g.last_rc == 0 and stopped == [n] * world
        assert sum(sent) == sum(merged) and 0 < sum(merged) <= world * n
        if n >= 1 << 20 and not dirty:
            assert sum(merged) < world * n   # hot names were combined at the senders
        for b in per:
            assert o.receive(b["dgrams"], _gen.T0 + k)[4] == n
    _same(_union_on_owners(g, world), o.dump())
    g.close()


# ------------------------------------------------------ 3. pipelined rounds --
@pytest.mark.parametrize("dirty", [0.0, 0.02])
def test_group_receive_datagrams_pipelined_vs_oracle(pa, dirty):
    """small_chunks, three members with batches of different lengths (one empty,
    one of a single datagram): the oracle receives chunk by chunk, sources in
    rank order, as test_shared_device_group_receive_pipelined_vs_oracle does."""
    rng = np.random.default_rng(7300 + int(dirty * 100))
    world = 3
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    o = O.Repo()
    for k, sizes in enumerate(((30000, 5000, 0), (70001, 4097, 1))):
        per = [_zipf_batch(pa, rng, n, 30000, dirty) if n else None for n in sizes]
        torch.cuda.synchronize()
        sent, merged, stopped = g.receive_datagrams([b["dev"] if b else _empty_pair() for b in per],
                                                    _gen.T0 + k, combine=True, small_chunks=True)
        assert g.last_rc == 0 and stopped == list(sizes)
        assert sum(sent) == sum(merged) and sum(merged) <= sum(sizes)
        for c in range(max((n + CHUNK - 1) // CHUNK for n in sizes)):
            for b, n in zip(per, sizes):
                if b and c * CHUNK < n:
                    o.receive(b["dgrams"][c * CHUNK:min(n, (c + 1) * CHUNK)], _gen.T0 + k)
    _same(_union_on_owners(g, world), o.dump())
    g.close()


# ---------------------------------------------------------- 4. stop rule --
STOP_SIZES = (6000, 9000, 3000)
_stop_cache = {}


def _stop_batches(pa):
    if not _stop_cache:
        rng = np.random.default_rng(7400)
        _stop_cache["per"] = [_zipf_batch(pa, rng, n, 20000)["dgrams"] for n in STOP_SIZES]
    return _stop_cache["per"]


@pytest.mark.parametrize("kind", ["short", "len_too_large", "zero_size"])
@pytest.mark.parametrize("pos", [0, 5000, 4096, STOP_SIZES[1] - 1])
def test_stop_rule(pa, pos, kind):
    """Member 1 of 3 holds a malformed datagram at `pos` (index 0, inside a
    chunk, exactly at a chunk boundary, the last index) and a second one later:
    stopped is the first index for member 1 and n for the others, the call
    reports PHIP_ERR_SHORT_BUFFER, the tables equal the oracle fed each
    member's prefix (the others' datagrams all merged).  The same batch through
    a world of one agrees with phip_receive_datagrams' stop_index."""
    world = 3
    per = [list(d) for d in _stop_batches(pa)]
    n1 = STOP_SIZES[1]
    per[1][pos] = W.malformed(kind, per[1][pos])
    later = pos + 1234
    if later < n1:
        per[1][later] = W.malformed("short", per[1][later])
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    sent, merged, stopped = g.receive_datagrams(per, _gen.T0, combine=True, small_chunks=True)
    assert g.last_rc == -5
    assert stopped == [STOP_SIZES[0], pos, STOP_SIZES[2]]
    assert "member 1" in g.L.phip_group_last_error(g.g).decode() and \
        "datagram %d" % pos in g.L.phip_group_last_error(g.g).decode()
    assert sum(sent) == sum(merged) == sum(stopped)   # clean 9 000-datagram batches: no combine
    o = O.Repo()
    for c in range((max(STOP_SIZES) + CHUNK - 1) // CHUNK):
        for d, stop in zip(per, stopped):
            if c * CHUNK < stop:
                part = d[c * CHUNK:min(stop, (c + 1) * CHUNK)]
                assert o.receive(part, _gen.T0)[4] == len(part)
    _same(_union_on_owners(g, world), o.dump())
    g.close()
    # a world of one (no rccl_self): the handle's own wire path
    g1 = pa.GPUGroup.open_all([0], log2_slots=14)
    s1, m1, st1 = g1.receive_datagrams([per[1]], _gen.T0, combine=True)
    ref = pa.GPURepo(log2_slots=14)
    assert st1 == [ref.receive_datagrams(per[1], _gen.T0)["stop"]] == [pos]
    assert g1.last_rc == -5 and s1 == m1 == [pos]
    assert _dump(g1.repos[0]) == _dump(ref)
    g1.close()
    ref.close()


# ------------------------------------------------------ 5. checked offsets --
@pytest.mark.parametrize("bad", ["decreasing", "past_bytes_len"])
@pytest.mark.parametrize("case", ["plain", "rccl_self", "shared_world2"])
def test_checked_offsets_are_refused(pa, case, bad):
    """bytes_len set (checked=True): a decreasing offset pair, or an offs[n]
    past bytes_len, is PHIP_ERR_INVALID naming the member and the entry; no
    table changes; the repaired batches then merge and equal the oracle.  The
    bad offsets still point inside the tensor's allocation (the bytes passed are
    a narrowed view of a larger tensor)."""
    rng = np.random.default_rng(7500)
    world = 2 if case == "shared_world2" else 1
    kw = dict(combine=True, rccl_self=case == "rccl_self")
    n, k = 20000, 12345
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    o = O.Repo()
    first = [_zipf_batch(pa, rng, 3000, 20000) for _ in range(world)]
    g.receive_datagrams([b["dev"] for b in first], _gen.T0, **kw)
    for b in first:
        o.receive(b["dgrams"], _gen.T0)
    before = [_dump(r) for r in g.repos]
    per = [_zipf_batch(pa, rng, n, 20000) for _ in range(world)]
    data, offs = per[0]["dev"]
    big = torch.zeros(data.numel() + 4096, dtype=torch.uint8, device=_dev())
    big[:data.numel()] = data
    view = big[:data.numel()]
    where = k if bad == "decreasing" else n
    good = int(offs[where])
    offs[where] = int(offs[k + 1]) + 5 if bad == "decreasing" else data.numel() + 8
    entry = k if bad == "decreasing" else n - 1
    batches = [(view, offs)] + [b["dev"] for b in per[1:]]
    torch.cuda.synchronize()
    with pytest.raises(pa.PatrolHipError) as ei:
        g.receive_datagrams(batches, _gen.T0 + 1, **kw)
    assert ei.value.code == -1
    assert "member 0" in str(ei.value) and "datagram %d " % entry in str(ei.value)
    assert [_dump(r) for r in g.repos] == before
    offs[where] = good
    torch.cuda.synchronize()
    sent, merged, stopped = g.receive_datagrams(batches, _gen.T0 + 1, **kw)
    assert g.last_rc == 0 and stopped == [n] * world and sum(sent) == sum(merged)
    for b in per:
        o.receive(b["dgrams"], _gen.T0 + 1)
    _same(_union_on_owners(g, world), o.dump())
    g.close()


# ------------------------------------------------------ 6. wire == decoded --
def test_wire_equals_decoded(pa):
    """The same 2^20 messages through receive_datagrams on one group and
    through receive (decoded) on a twin, both world 1 with rccl_self and the
    combine on: identical dumps."""
    rng = np.random.default_rng(7600)
    n = 1 << 20
    b = _zipf_batch(pa, rng, n, 30000)
    nblob, noffs = pa.names_blob(b["names"])
    dv = [torch.from_numpy(nblob).to(_dev()), torch.from_numpy(noffs.view(np.int32)).to(_dev())]
    dv += [torch.from_numpy(np.ascontiguousarray(b[k]).view(np.int64)).to(_dev()) for k in ("a", "t", "e")]
    torch.cuda.synchronize()
    gw = pa.GPUGroup.open_all([0], log2_slots=14)
    gd = pa.GPUGroup.open_all([0], log2_slots=14)
    sw, mw, stopped = gw.receive_datagrams([b["dev"]], _gen.T0, combine=True, rccl_self=True)
    sd, md = gd.receive([dv], _gen.T0, combine=True, rccl_self=True)
    assert stopped == [n] and sw == mw and sd == md
    assert 0 < mw[0] < n and 0 < md[0] < n   # both combined
    dw, dd = _dump(gw.repos[0]), _dump(gd.repos[0])
    assert len(dw) > 1000 and dw == dd
    gw.close()
    gd.close()


# ------------------------------------------------------------------ 7. ring --
def test_group_ring_receive(pa):
    """World 2 shared, one Ring per member over g.repos[i], two slots each
    (2 000 and 40 000 datagrams; member 1's second slot holds a short datagram)
    received in submit order: the tables equal the oracle, stopped is right, the
    slots can be acquired again; a ring of a foreign handle is refused, and an
    out-of-order slot is PHIP_ERR_BUSY and stays submitted."""
    rng = np.random.default_rng(7700)
    world = 2
    g = pa.GPUGroup.open_all([0] * world, log2_slots=14)
    rings = [pa.Ring(g.repos[i], nslots=2, max_msgs=40000) for i in range(world)]
    o = O.Repo()
    sizes = (2000, 40000)
    per = [[_zipf_batch(pa, rng, n, 20000)["dgrams"] for n in sizes] for _ in range(world)]
    bad_at = 31000
    per[1][1][bad_at] = W.malformed("short", per[1][1][bad_at])
    slots = [[None, None] for _ in range(world)]
    for i in range(world):
        for s in range(2):
            slot, n = rings[i].fill(per[i][s])
            rings[i].submit(slot, n)
            slots[i][s] = slot
    # out of order: the second slots first
    with pytest.raises(pa.PatrolHipError) as ei:
        g.ring_receive(rings, [slots[0][1], slots[1][1]], _gen.T0)
    assert ei.value.code == -9
    # a ring of a foreign handle
    other = pa.GPURepo(log2_slots=10)
    foreign = pa.Ring(other, nslots=1, max_msgs=16)
    fs, fn = foreign.fill([per[0][0][0]])
    foreign.submit(fs, fn)
    with pytest.raises(pa.PatrolHipError) as ei:
        g.ring_receive([rings[0], foreign], [slots[0][0], fs], _gen.T0)
    assert ei.value.code == -1
    assert all(len(r) == 0 for r in g.repos)   # nothing was received, every slot still submitted
    for s in range(2):
        sent, merged, stopped = g.ring_receive(rings, [slots[0][s], slots[1][s]], _gen.T0 + s)
        want = [sizes[s], bad_at if s == 1 else sizes[s]]
        assert stopped == want and g.last_rc == (-5 if s == 1 else 0)
        assert sum(sent) == sum(merged) == sum(want)
        for i in range(world):
            assert o.receive(per[i][s][:want[i]], _gen.T0 + s)[4] == want[i]
    _same(_union_on_owners(g, world), o.dump())
    # every slot is free again (acquire would raise PHIP_ERR_BUSY otherwise);
    # a NULL ring is an empty batch for its member
    for i in range(world):
        for s in range(2):
            slot, n = rings[i].fill(per[i][0][:10])
            rings[i].submit(slot, n)
            slots[i][s] = slot
    sent, merged, stopped = g.ring_receive([rings[0], None], [slots[0][0], 0], _gen.T0 + 2)
    assert stopped == [10, 0] and sum(sent) == sum(merged) == 10
    for r in rings + [foreign]:
        r.close()
    other.close()
    g.close()
