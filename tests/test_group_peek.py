"""Owner-routed peek over the shard group (phip_group_peek) on one GPU.

The reference is tests/_group_peek.py's: PC.reference over the oracle's state,
status / remaining / have bit for bit, retry_at by its definition.  World 1 in
both group forms with and without the RCCL self-exchange (there also against
GPURepo.peek_device on the same handle), shared-device groups of world 2 and
3, the scatter-step sizes, small rounds, that nothing is written, a peek
against the take that follows it, peeks between the group's writing calls,
poisoned result columns, a corrupted offset column, the flag checks and the
query pack itself.
"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _columns as CO  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _group_ops as GO  # noqa: E402
from tests import _group_peek as GP  # noqa: E402
from tests import _peek_cases as PC  # noqa: E402

DEV = torch.device("cuda", 0)
POISON = CO.POISON


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


@pytest.fixture(scope="module")
def tab():
    """The seeded table and its oracle: computed once, shared, never changed."""
    t = GP.table()
    return t, GP.seeded_oracle(t)


_REFS = {}


def _case(tab, world, sizes):
    """Member queries of (world, sizes) and their references, computed once."""
    t, o = tab
    key = (world, tuple(sizes))
    if key not in _REFS:
        qs = GP.member_queries(t, world, sizes)
        _REFS[key] = (qs, [GP.references(o.get, q) for q in qs])
    return _REFS[key]


def _group(pa, tab, world, **kw):
    g = pa.GPUGroup.open_all([0] * world, log2_slots=11, **kw)
    per = GP.seed_group(g, tab[0], world)
    assert [len(r) for r in g.repos] == per
    return g


def _check_all(out, qs, refs, tag=""):
    for i, (q, r) in enumerate(zip(qs, refs)):
        GP.check_member(GP.host_results(out[i], len(q)), q, r, "%s member %d" % (tag, i))


# ------------------------------------------------------------------ world 1 --
@pytest.mark.parametrize("mode,rccl_self", [("all", False), ("rank", False), ("all", True),
                                            ("rank", True)])
def test_group_peek_world1_equals_peek_on_the_handle(pa, tab, mode, rccl_self):
    """3000 queries through a group of one: straight to phip_peek, or
    (rccl_self) through the pack, the RCCL exchange to itself, the owner's
    peek, the answers' way back and the scatter.  Every column equals
    GPURepo.peek_device on the same handle bit for bit, and the reference."""
    t, _ = tab
    n = 3000
    (q,), (refs,) = _case(tab, 1, (n,))
    if mode == "all":
        g = pa.GPUGroup.open_all([0], log2_slots=11)
        repo = g.repos[0]
    else:
        repo = pa.GPURepo(log2_slots=11)
        g = pa.GPUGroup.open_rank(repo, pa.GPUGroup.unique_id(), 1, 0)
    repo.seed(t["names"], *t["cols"])
    d = GP.device_batch(q, DEV)
    out, sent, answered = g.peek([d], rccl_self=rccl_self, want_state=True)
    assert sent == [n] and answered == [n]
    got = GP.host_results(out[0], n)
    GP.check_member(got, q, refs)
    one = dict(status=torch.zeros(n, dtype=torch.uint8, device=DEV),
               state=torch.zeros((n, 4), dtype=torch.int64, device=DEV))
    for k in ("remaining", "have", "retry_at"):
        one[k] = torch.zeros(n, dtype=torch.int64, device=DEV)
    repo.peek_device(n, **d, **one)
    for k in GP.COLUMNS:
        assert torch.equal(out[0][k], one[k]), k
    g.close()
    if mode == "rank":
        repo.close()


# ------------------------------------------------------------ shared device --
@pytest.mark.parametrize("want_state", [False, True])
@pytest.mark.parametrize("world,sizes", GP.SHARED_CASES)
def test_shared_device_group_peek_vs_reference(pa, tab, world, sizes, want_state):
    """`world` shards on one GPU, member i submitting its own queries (one of
    them empty): every member's answers equal the reference over the bucket's
    owner's state; with want_state the state column is the state evaluated."""
    qs, refs = _case(tab, world, sizes)
    g = _group(pa, tab, world)
    out, sent, answered = g.peek([GP.device_batch(q, DEV) for q in qs], want_state=want_state)
    assert all((o["state"] is not None) == want_state for o in out)
    _check_all(out, qs, refs)
    assert sent == list(sizes) and sum(answered) == sum(sizes)
    own = np.concatenate([GO.owners([x[0] for x in q], world) for q in qs if q])
    assert answered == np.bincount(own, minlength=world).tolist()
    g.close()


@pytest.fixture(scope="module")
def pair(pa, tab):
    """A seeded world-2 group that read-only tests share."""
    g = _group(pa, tab, 2)
    yield g
    g.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513])
def test_group_peek_sizes_around_the_scatter_step(pa, tab, pair, n):
    """n queries on member 0 of a world-2 group (512 are one scatter step of
    the pack): the results are complete and in place."""
    qs, refs = _case(tab, 2, (2700, 0))
    q, r = qs[0][4 * n:5 * n], refs[0][4 * n:5 * n]   # (different queries at every size)
    out, sent, answered = pair.peek([GP.device_batch(q, DEV), GP.device_batch([], DEV)],
                                    want_state=True)
    assert sent == [n, 0] and sum(answered) == n
    GP.check_member(GP.host_results(out[0], n), q, r)


@pytest.mark.parametrize("world", [2, 1])
def test_group_peek_small_rounds(pa, tab, world):
    """Rounds of 4096 queries: 9000 and 5000 give 3 and 2 rounds, so the
    shorter member sends an empty round.  World 1 runs 9000 through the RCCL
    exchange to itself."""
    sizes = GP.ROUNDS_CASE[1][:world]
    qs, refs = _case(tab, 2, GP.ROUNDS_CASE[1])
    qs, refs = qs[:world], refs[:world]
    g = _group(pa, tab, world)
    out, sent, answered = g.peek([GP.device_batch(q, DEV) for q in qs], small_chunks=True,
                                 rccl_self=world == 1, want_state=True)
    _check_all(out, qs, refs)
    assert sent == list(sizes) and sum(answered) == sum(sizes)
    g.close()


# ---------------------------------------------------------- nothing written --
def _held(g):
    """What every member holds: its buckets, len, the change set's count and
    the sweep's layout generation."""
    out = []
    for r in g.repos:
        dump = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in r.dump().items()}
        out.append((dump, len(r), r.capacity, r.changes_count(), r.export_sweep(None, 1)[1][1]))
    return out


def test_group_peek_writes_nothing(pa, tab):
    """A group with change sets, takes first (marks pending, new buckets), then
    2700 queries of which ~15% name absent buckets, with and without rounds:
    every member's dump, len, changes_count and layout generation stay, and no
    absent name exists on any member afterwards."""
    t, _ = tab
    g = _group(pa, tab, 2, track_changes=True)
    rng = np.random.default_rng(41)
    b = GO.gen_ops(rng, 300, t["names"][:200] + [b"new-%d" % i for i in range(40)], all_take=True)
    from tests.test_group_ops import _dev
    g.apply_mixed([_dev(b), _dev(GO.gen_ops(rng, 0, t["names"]))])
    before = _held(g)
    assert sum(h[3]["pending"] for h in before) > 0
    o = O.Repo()
    for r in g.repos:   # the reference over what the group holds now
        d = r.dump()
        o.seed(list(d), *[np.array([getattr(v, f) for v in d.values()], dt) for f, dt in
                          (("added", np.uint64), ("taken", np.uint64), ("elapsed", np.int64),
                           ("created", np.int64))])
    qs = GP.member_queries(t, 2, (2700, 0))
    refs = [GP.references(o.get, q) for q in qs]
    absent = {q[0] for q in qs[0] if o.get(q[0]) is None}
    assert len(absent) >= 100
    for kw in (dict(), dict(small_chunks=True), dict(want_state=True)):
        out, _, _ = g.peek([GP.device_batch(q, DEV) for q in qs], **kw)
        _check_all(out, qs, refs, str(kw))
        assert _held(g) == before, kw
    held = set().union(*[set(h[0]) for h in before])
    assert not (absent & held)
    g.close()


# --------------------------------------------------- the take that follows --
def test_group_peek_equals_the_take_that_follows(pa, tab):
    """One query per name of a 500-name set (present and absent), g.peek, then
    g.apply_mixed of the same operands as TAKE ops: status without ABSENT /
    CREATED, remaining and have agree entry for entry, and ABSENT is set
    exactly where CREATED is."""
    t, _ = tab
    rng = np.random.default_rng(43)
    names = t["names"][:420] + t["absent"][:80]
    order = rng.permutation(len(names))
    qs = []
    prng = random.Random(44)
    for k in order:
        k = int(k)
        state = t["states"][k] if k < 420 else None
        rate = t["rates"][k] if k < 420 else None
        q = PC.plain_query(prng, state, rate or prng.choice(PC.PLAIN_RATES)) \
            if (rate or prng.random() < 0.5) else PC.extreme_query(prng, state)
        qs.append((names[k],) + q)
    halves = [qs[:260], qs[260:]]
    g = _group(pa, tab, 2)
    ds = [GP.device_batch(q, DEV) for q in halves]
    peek, _, _ = g.peek(ds)
    ops = []
    for d, q in zip(ds, halves):
        ops.append(dict(d, kind=torch.zeros(len(q), dtype=torch.uint8, device=DEV), added=None,
                        taken=None, elapsed=None))
    take, _, _ = g.apply_mixed(ops)
    n_abs = 0
    for i, q in enumerate(halves):
        p, k = GP.host_results(peek[i], len(q)), take[i]
        ts = k["status"].cpu().numpy()
        assert np.array_equal(p["status"] & 0x3F, ts & 0x3F), i
        assert np.array_equal((p["status"] & PC.ABSENT) != 0, (ts & 0x80) != 0), i
        assert np.array_equal(p["remaining"], k["remaining"].cpu().numpy().view(np.uint64)), i
        assert np.array_equal(p["have"], k["have"].cpu().numpy().view(np.uint64)), i
        n_abs += int(((p["status"] & PC.ABSENT) != 0).sum())
    assert n_abs == 80
    g.close()


# -------------------------------------------------------------- interleaving --
@pytest.mark.parametrize("world", [2, 1])
def test_group_peek_between_the_writing_calls(pa, tab, world):
    """apply_mixed, peek, receive, peek, apply_mixed, peek on one group in
    rounds of 4096: the peek's column sets and the ops path's share the
    member's scratch and split sizes.  Every peek equals the reference over
    the oracle's state at that moment; the final tables equal the oracle's."""
    from patrol_amd.engine import names_blob
    from tests.test_group_ops import _dev, _union
    t, _ = tab
    rng = np.random.default_rng(4700 + world)
    kw = dict(small_chunks=True, rccl_self=world == 1)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=12)
    GP.seed_group(g, t, world)
    o = GP.seeded_oracle(t)
    pool = t["names"][:300] + t["absent"][:60]
    chunk = GO.SMALL_CHUNK
    sizes = (5000, 4500)[:world]
    step = [0]

    def apply():
        step[0] += 1
        bs = [GO.gen_ops(rng, n, pool, t0=PC.T0 + step[0] * 10**12 + 1000 * i)
              for i, n in enumerate(sizes)]
        GO.oracle_results(o, bs, GO.apply_order(sizes, chunk))
        _, sent, applied = g.apply_mixed([_dev(b) for b in bs], **kw)
        assert sent == list(sizes) and sum(applied) == sum(sizes)

    def receive():
        step[0] += 1
        now = PC.T0 + step[0] * 10**12
        per = []
        for n in sizes:
            ids = _gen.zipf_ids(rng, n, len(pool))
            names = [pool[int(i)] for i in ids]
            a, tk, e = _gen.clean_states(rng, n)
            per.append((names, a, tk, e))
        bt = []
        for names, a, tk, e in per:
            blob, offs = names_blob(names)
            bt.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in
                            (blob, offs.view(np.int32), a.view(np.int64), tk.view(np.int64), e)))
        sent, merged = g.receive(bt, now, **kw)
        assert sent == list(sizes) and sum(merged) == sum(sizes)
        for c in range(max((n + chunk - 1) // chunk for n in sizes)):
            for (names, a, tk, e), n in zip(per, sizes):
                if c * chunk < n:
                    sl = slice(c * chunk, min(n, (c + 1) * chunk))
                    o.receive_soa(names[sl], a[sl], tk[sl], e[sl], now)

    def peek(seed):
        qs = [PC.table_queries(seed + i, t, n) for i, n in enumerate((4500, 200)[:world])]
        refs = [GP.references(o.get, q) for q in qs]
        out, sent, answered = g.peek([GP.device_batch(q, DEV) for q in qs], want_state=True, **kw)
        _check_all(out, qs, refs, "peek %d" % seed)
        assert sent == [len(q) for q in qs] and sum(answered) == sum(sent)

    apply()
    peek(900)
    receive()
    peek(910)
    apply()
    peek(920)
    assert _union(g.repos, world) == o.dump()
    g.close()


# ------------------------------------------------------------ result columns --
PEEK_DT = dict(status=np.dtype(np.uint8), remaining=np.dtype(np.uint64), have=np.dtype(np.uint64),
               retry_at=np.dtype(np.int64), state=CO.REPLY_DT)
PEEK_SHIFT = dict(status=1, remaining=8, have=8, retry_at=8, state=8)


class _Column:
    """n entries of one peek column on the device between GUARD bytes, the
    whole buffer POISON (tests/_columns.py's Column, for the peek columns)."""

    def __init__(self, name, n, misaligned):
        self.name, self.n, self.dtype = name, n, PEEK_DT[name]
        self.off = CO.GUARD + (PEEK_SHIFT[name] if misaligned else 0)
        self.nbytes = n * self.dtype.itemsize
        self.buf = torch.full((self.off + self.nbytes + CO.GUARD,), POISON, dtype=torch.uint8,
                              device=DEV)
        assert self.buf.data_ptr() % CO.BASE_ALIGN == 0
        self.ptr = self.buf.data_ptr() + self.off

    def check(self):
        """Asserts both guards are intact; -> the n entries."""
        b = self.buf.cpu().numpy()
        assert (b[:self.off] == POISON).all(), "%s: written before the column" % self.name
        assert (b[self.off + self.nbytes:] == POISON).all(), "%s: written after the column" % self.name
        return np.frombuffer(b[self.off:self.off + self.nbytes].tobytes(), self.dtype, self.n)


def _raw_call(g, ds, cols, flags):
    """phip_group_peek with the caller's own column pointers (cols[i]: name ->
    _Column or absent)."""
    from patrol_amd import _lib
    k = len(ds)
    ops = (_lib.phip_ops * k)()
    res = (_lib.phip_peek_results * k)()
    for i, d in enumerate(ds):
        n = d["name_offs"].numel() - 1
        ops[i] = _lib.phip_ops(n, d["names"].numel(), None, d["names"].data_ptr(),
                               d["name_offs"].data_ptr(), d["now"].data_ptr(), d["freq"].data_ptr(),
                               d["per"].data_ptr(), d["count"].data_ptr(), None, None, None)
        res[i] = _lib.phip_peek_results(*[cols[i][c].ptr if c in cols[i] else None
                                          for c in GP.COLUMNS])
    torch.cuda.synchronize()
    return g.L.phip_group_peek(g.g, ops, res, None, None, flags)


def _want(refs, n):
    w = dict(status=np.array([r["status"] for r in refs], np.uint8),
             remaining=np.array([r["remaining"] for r in refs], np.uint64),
             have=np.array([r["have"] for r in refs], np.uint64),
             state=np.array([r["s"] for r in refs], CO.REPLY_DT))
    assert all(len(v) == n for v in w.values())
    return w


@pytest.mark.parametrize("misaligned", [False, True])
def test_group_peek_result_columns_every_subset(pa, tab, pair, misaligned):
    """Every subset of the five columns NULL on both members of a world-2
    group (513 and 300 queries), the passed ones poisoned between guards: all
    n entries are written, bit-equal to the reference, the guards are intact."""
    from patrol_amd import _lib
    qs, refs = _case(tab, 2, (2700, 0))
    parts = [(qs[0][:513], refs[0][:513]), (qs[0][600:900], refs[0][600:900])]
    ds = [GP.device_batch(q, DEV) for q, _ in parts]
    for mask in range(32):
        names = [c for b, c in enumerate(GP.COLUMNS) if mask >> b & 1]
        cols = [{c: _Column(c, len(q), misaligned) for c in names} for q, _ in parts]
        flags = _lib.DEVICE_PTRS | _lib.GROUP_PEEK_STATE
        assert _raw_call(pair, ds, cols, flags) == 0, mask
        for i, (q, r) in enumerate(parts):
            got = {c: col.check() for c, col in cols[i].items()}
            want = _want(r, len(q))
            for c in got:
                if c == "retry_at":
                    for j in range(len(q)):
                        PC.check_retry(r[j], (None,) + q[j][1:], int(got[c][j]))
                else:
                    assert got[c].tobytes() == want[c].tobytes(), (mask, i, c)


def test_group_peek_rejects_corrupted_offsets(pa, tab, pair):
    """One entry of member 1's name_offs past names_len: PHIP_ERR_INVALID
    naming member 1 and the query, every passed status 0, the other columns
    still poison; a following valid call is right."""
    from patrol_amd import _lib
    qs, refs = _case(tab, 2, (2700, 0))
    parts = [(qs[0][:1000], refs[0][:1000]), (qs[0][1000:2700], refs[0][1000:2700])]
    ds = [GP.device_batch(q, DEV) for q, _ in parts]
    k = 777
    good = int(ds[1]["name_offs"][k])
    ds[1]["name_offs"][k] = 0x7FFF0000   # entries k-1 and k are malformed
    cols = [{c: _Column(c, len(q), True) for c in GP.COLUMNS} for q, _ in parts]
    assert _raw_call(pair, ds, cols, _lib.DEVICE_PTRS | _lib.GROUP_PEEK_STATE) == -1
    err = pair.L.phip_group_last_error(pair.g).decode()
    assert "member 1" in err and "query %d " % (k - 1) in err, err
    for c in cols:
        assert not c["status"].check().any()
        for name in GP.COLUMNS[1:]:
            assert (c[name].check().view(np.uint8) == POISON).all(), name
    with pytest.raises(pa.PatrolHipError) as ei:
        pair.peek(ds)
    assert ei.value.code == -1 and "member 1" in str(ei.value)
    ds[1]["name_offs"][k] = good
    out, _, _ = pair.peek(ds, want_state=True)
    _check_all(out, [q for q, _ in parts], [r for _, r in parts], "repaired")


def test_group_peek_flags(pa, tab, pair):
    """PHIP_DEVICE_PTRS is required; PHIP_ROUTE_COMBINE, PHIP_RECV_ASYNC and
    a state column without PHIP_GROUP_PEEK_STATE are refused:
    PHIP_ERR_INVALID, the columns untouched."""
    from patrol_amd import _lib
    qs, refs = _case(tab, 2, (2700, 0))
    parts = [qs[0][:100], qs[0][100:200]]
    ds = [GP.device_batch(q, DEV) for q in parts]
    D = _lib.DEVICE_PTRS
    for flags, names in ((0, GP.COLUMNS[:4]), (_lib.GROUP_RCCL_SELF, GP.COLUMNS[:4]),
                         (D | _lib.ROUTE_COMBINE, GP.COLUMNS[:4]),
                         (D | _lib.RECV_ASYNC, GP.COLUMNS[:4]),
                         (D | _lib.GROUP_PEEK_STATE | _lib.RECV_CLASSIFY, GP.COLUMNS),
                         (D, GP.COLUMNS), (D | _lib.GROUP_SMALL_CHUNKS, GP.COLUMNS)):
        cols = [{c: _Column(c, 100, False) for c in names} for _ in parts]
        assert _raw_call(pair, ds, cols, flags) == -1, flags
        for c in cols:
            for col in c.values():
                assert (col.check().view(np.uint8) == POISON).all(), (flags, col.name)
    cols = [{c: _Column(c, 100, False) for c in GP.COLUMNS[:4]} for _ in parts]
    assert _raw_call(pair, ds, cols, D) == 0
    assert all(bool(c["status"].check().all()) for c in cols)


# ------------------------------------------------------------ the query pack --
@pytest.fixture(scope="module")
def pack_repo(pa):
    repo = pa.GPURepo(log2_slots=10)
    yield repo
    repo.close()


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 2700])
def test_query_pack_is_stable_owner_partition(pa, tab, pack_repo, n, world):
    """phip_route_pack_ops without a kind column on either side: send_src is
    the stable argsort of the owners, every send column the input gathered
    through it with x0 / x1 / x2 = freq / per / count whatever the batch would
    have been as ops, counts / name_bytes the per-owner sums, the packed names
    byte-identical.  Once more with the operand columns NULL: zeros."""
    qs, _ = _case(tab, 2, (2700, 0))
    q = qs[0][:n]
    d = GP.device_batch(q, DEV)
    names, now, freq, per, count = PC.columns(q)
    own = GO.owners(names, world)
    src = np.argsort(own, kind="stable")
    lens = np.array([len(x) for x in names], np.int64)
    for tag, drop in (("all columns", ()), ("NULL operands", ("freq", "per", "count"))):
        db = {k: (None if k in drop else v) for k, v in d.items()}
        out = pack_repo.route_pack_ops_device(n, world, None, **db)
        assert out["kind"] is None
        assert np.array_equal(out["src"].cpu().numpy()[:n], src), tag
        zero = np.zeros(n, np.int64)
        want = dict(now=now, lens=lens, x0=zero if drop else freq, x1=zero if drop else per,
                    x2=zero if drop else count.view(np.int64))
        for c, w in want.items():
            assert np.array_equal(out[c].cpu().numpy()[:n].astype(np.int64), w[src]), (tag, c)
        assert np.array_equal(out["counts"].cpu().numpy(), np.bincount(own, minlength=world)), tag
        assert np.array_equal(out["name_bytes"].cpu().numpy(),
                              np.bincount(own, weights=lens, minlength=world).astype(np.int64)), tag
        packed = b"".join(names[j] for j in src)
        assert out["names"].cpu().numpy()[:len(packed)].tobytes() == packed, tag
