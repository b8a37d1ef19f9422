"""phip_export_sweep on the GPU (include/patrolhip.h "Anti-entropy sweep"),
through the C ABI via the binding.

What a sweep must write is computed in Python from the table's dump
(tests/_sweep_cases.py: MarshalBinary of every bucket but zero states and,
under a filter, the eviction rule's idle ones); what a peer ends with is an
oracle Repo that received the same datagrams.  Bit-exact throughout.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _sweep_cases as SC  # noqa: E402

T0, SEC = _gen.T0, _gen.SEC
I64MAX, I64MIN = SC.I64MAX, SC.I64MIN
LENGTHS = [0, 1, 14, 15, 22, 23, 40, 231]
NAN, NAN2, NZERO = 0x7FF8000000000000, 0xFFF8000000000001, 1 << 63
PINF, NINF = 0x7FF0000000000000, 0xFFF0000000000000


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


def seed(repo, rows):
    ks = list(rows)
    repo.seed(ks, *[[rows[k][j] for k in ks] for j in range(4)])


def make_names(count, lengths=LENGTHS):
    """About `count` distinct names cycling through the lengths (one empty
    name, single bytes while they last)."""
    out = []
    for k in range(count):
        L = lengths[k % len(lengths)]
        if L == 0:
            nm = b""
        elif L == 1:
            nm = bytes([33 + (k // len(lengths)) % 200])
        else:
            nm = (b"%05d" % k).ljust(L, b"n")[:L]
        out.append(nm)
    return list(dict.fromkeys(out))


def special_rows(names, rng, p_special=0.25):
    """Dirty states (NaN, -0.0, negatives, a few zeros) plus the extremes."""
    a, t, e = _gen.dirty_states(rng, len(names), p_special=p_special)
    rows = {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)}
    ext = [(PINF, NINF, I64MIN), (NINF, PINF, I64MAX), (NAN, NAN2, -1), (NZERO, NZERO, 1),
           (NZERO, 0, 0), (0, NZERO, I64MIN), (NAN2, 0, 0), (1, 0x8000000000000001, 0)]
    for k, st in enumerate(ext):
        rows[names[7 * k + 3]] = st + (T0,)
    if b"" in rows:
        rows[b""] = (SC.A1, NZERO, 7, T0)     # the one empty name always has something to export
    return rows


def kinds_table(pa, log2_slots=10, count=620, zeros=50, **kw):
    """Every kind of record: the name lengths, the special states, and zero
    states left behind by zero-state Receives (incast requests)."""
    repo = pa.GPURepo(log2_slots=log2_slots, arena_bytes=1 << 15, **kw)
    names = make_names(count)
    seed(repo, special_rows(names, np.random.default_rng(17)))
    zn = [(b"z%03d" % k).ljust(LENGTHS[2 + k % 6], b"z") for k in range(zeros)]
    out = repo.receive_soa(zn, [0] * zeros, [0] * zeros, [0] * zeros, T0 + 1)
    assert (out["status"] & 0x80).all()
    return repo


def check_call(dgs, st, max_msgs, out_cap):
    offs = st["offs"]
    assert st["n"] == len(dgs) <= max_msgs
    assert offs[0] == 0 and int(offs[-1]) == st["bytes"] <= out_cap
    assert (np.diff(offs.astype(np.int64)) >= SC.FIXED).all()          # strictly increasing
    assert [len(d) for d in dgs] == list(np.diff(offs.astype(np.int64)))
    assert st["slots_scanned"] <= SC.window(max_msgs)


def sweep_all(repo, max_msgs, out_cap=None, now=0, idle_ns=0, cursor=None, max_calls=100000):
    """Loop to done -> (datagrams in order, calls, stats of every call)."""
    cap = out_cap if out_cap is not None else 256 * max_msgs
    got, sts = [], []
    while True:
        dgs, cursor, st = repo.export_sweep(cursor, max_msgs, out_cap, now, idle_ns)
        check_call(dgs, st, max_msgs, cap)
        got += dgs
        sts.append(st)
        assert len(sts) <= max_calls
        if st["done"]:
            return got, len(sts), sts


def name_of(dg):
    assert len(dg) == SC.FIXED + dg[24]
    return dg[SC.FIXED:]


def assert_exact(got, model):
    """The datagrams are exactly the model's, each once."""
    names = [name_of(d) for d in got]
    assert len(names) == len(set(names)), "a bucket was exported twice"
    assert len(got) == len(model), (len(got), len(model))
    bad = [n for n, d in zip(names, got) if model.get(n) != d]
    assert not bad, bad[:5]


def test_one_call_every_kind_of_record(pa):
    repo = kinds_table(pa)
    rows = gpu_dump(repo)
    model = SC.exported(rows)
    assert len(rows) >= 590 and 50 <= len(rows) - len(model) <= 120
    assert {len(k) for k in model} == set(LENGTHS)
    dgs, cur, st = repo.export_sweep(None, max_msgs=1024)
    check_call(dgs, st, 1024, 256 * 1024)
    assert st["done"] == 1 and st["restarted"] == 0 and st["slots_scanned"] == 1024
    assert cur[0] == repo.capacity == 1024
    assert_exact(dgs, model)
    # each is MarshalBinary of the dumped state, and what the by-name export gives
    names = [name_of(d) for d in dgs]
    for nm, d in zip(names, dgs):
        assert d == pa.marshal(nm, pa.BucketState(*rows[nm])), nm
    by_name, found = repo.export_datagrams(names)
    assert found.all() and by_name == dgs
    # slot order: a second sweep gives the same sequence
    assert repo.export_sweep(None, max_msgs=1024)[0] == dgs
    # count mode: the same totals, the cursor untouched
    cnt = repo.sweep_count()
    assert (cnt["n"], cnt["bytes"]) == (st["n"], st["bytes"]) == (len(model), sum(map(len, dgs)))
    c, s = pa._lib.phip_sweep_cursor(5, 7), pa._lib.phip_sweep_stats()
    assert repo.L.phip_export_sweep(repo.h, C.byref(c), 0, 0, None, 0, None, 0, C.byref(s), 0x200) == 0
    assert (c.slot, c.layout, s.n, s.bytes) == (5, 7, st["n"], st["bytes"])
    # the generator
    assert [d for ds, _ in repo.sweep(max_msgs=100) for d in ds] == dgs
    # a call on a finished cursor writes nothing and stays done
    d2, cur2, st2 = repo.export_sweep(cur, max_msgs=8)
    assert d2 == [] and st2["n"] == 0 and st2["done"] == 1 and cur2 == cur
    repo.close()


def test_resumable_one_message_a_call(pa):
    repo = kinds_table(pa)
    model = SC.exported(gpu_dump(repo))
    one = repo.export_sweep(None, max_msgs=1024)[0]
    got, calls, sts = sweep_all(repo, 1)
    assert got == one
    assert_exact(got, model)
    assert calls <= len(model) + 1024 // 4096 + 1
    assert all(s["restarted"] == 0 for s in sts)
    repo.close()


def test_resumable_byte_cap_binds(pa):
    """max_msgs = 7, out_cap = 256: a 231-byte name fills a call, short names
    go several at a time, and the cut falls wherever the bytes run out."""
    repo = pa.GPURepo(log2_slots=10, arena_bytes=1 << 16)
    names = make_names(400, [231, 1, 14, 231, 23, 100, 231, 40])
    seed(repo, special_rows(names, np.random.default_rng(5), p_special=0.1))
    model = SC.exported(gpu_dump(repo))
    assert sum(len(k) == 231 for k in model) >= 100
    got, calls, sts = sweep_all(repo, 7, out_cap=256)
    assert_exact(got, model)
    assert calls <= len(model) + 1
    assert max(s["n"] for s in sts) > 1 and max(s["bytes"] for s in sts) == 256
    repo.close()


def test_resumable_windows_and_cuts_inside_a_tile(pa):
    """2^14 slots, max_msgs = 64: W = 4096, four windows, ~20 cuts in each."""
    repo = pa.GPURepo(log2_slots=14, arena_bytes=1 << 18)
    rng = np.random.default_rng(9)
    names = make_names(5000)
    a, t, e = _gen.clean_states(rng, len(names))
    seed(repo, {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)})
    zn = [b"zz-%d" % k for k in range(300)]
    repo.receive_soa(zn, [0] * 300, [0] * 300, [0] * 300, T0)
    assert repo.capacity == 1 << 14
    model = SC.exported(gpu_dump(repo))
    assert len(model) == len(names)
    got, calls, sts = sweep_all(repo, 64)
    assert_exact(got, model)
    assert len(model) // 64 <= calls <= len(model) + (1 << 14) // 4096 + 1
    assert sum(s["slots_scanned"] == 4096 and s["n"] == 64 for s in sts) >= 40
    got2, calls2, _ = sweep_all(repo, 3000)               # W = 12288: two windows
    assert got2 == got and calls2 >= 2
    assert repo.sweep_count()["n"] == len(model)
    repo.close()


def test_empty_and_zero_only(pa):
    repo = pa.GPURepo(log2_slots=10)
    for _ in range(2):
        dgs, cur, st = repo.export_sweep(None, max_msgs=16)
        assert dgs == [] and st["n"] == 0 and st["bytes"] == 0 and st["done"] == 1
        assert list(st["offs"]) == [0] and st["slots_scanned"] == 1024
        assert repo.sweep_count()["n"] == 0
        zn = [b"only-zero-%d" % k for k in range(100)] + [b"a-long-zero-state-bucket-name-%d" % k
                                                          for k in range(20)]
        repo.receive_soa(zn, [0] * 120, [NZERO] * 120, [0] * 120, T0)   # (-0.0 is zero too)
    assert len(repo) == 120
    repo.close()
    # a sparse table: a window ends before max_msgs is reached, done == 0 with fewer datagrams
    repo = pa.GPURepo(log2_slots=13)
    rows = {b"sparse-%d" % k: (SC.A1, SC.T1, k, T0) for k in range(200)}
    seed(repo, rows)
    got, calls, sts = sweep_all(repo, 512)
    assert_exact(got, SC.exported(rows))
    assert calls == 2 and sts[0]["done"] == 0 and 0 < sts[0]["n"] < 512
    assert [s["slots_scanned"] for s in sts] == [4096, 4096]
    repo.close()


def test_filter_is_the_eviction_rule(pa):
    repo = pa.GPURepo(log2_slots=10, arena_bytes=1 << 12)
    rows = SC.filter_rows()
    seed(repo, rows)
    assert gpu_dump(repo) == rows
    sizes = set()
    for idle_ns in [0] + SC.IDLE_NS:
        model = SC.exported(rows, SC.NOW, idle_ns)
        got, _, _ = sweep_all(repo, 16, now=SC.NOW, idle_ns=idle_ns)
        assert_exact(got, model)
        cnt = repo.sweep_count(SC.NOW, idle_ns)
        assert (cnt["n"], cnt["bytes"]) == (len(model), sum(map(len, got)))
        if idle_ns:   # the same buckets phip_evict_idle would leave
            assert repo.evict_idle(SC.NOW, idle_ns, dry_run=True)["idle"] == len(rows) - len(model)
        sizes.add(len(model))
    assert len(sizes) >= 5


def test_invalid_arguments(pa):
    import torch
    repo = kinds_table(pa, count=80, zeros=4)
    L, lib = repo.L, pa._lib
    out, offs = np.zeros(4096, np.uint8), np.zeros(9, np.uint64)

    def call(idle_ns=0, max_msgs=8, out_cap=4096, flags=0, o=out, f=offs, cur=None):
        c, s = cur or lib.phip_sweep_cursor(), lib.phip_sweep_stats()
        p = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data   # noqa: E731
        return L.phip_export_sweep(repo.h, C.byref(c), 0, idle_ns, p(o), out_cap, p(f), max_msgs,
                                   C.byref(s), flags), c, s

    assert call()[0] == 0
    assert call(out_cap=256, max_msgs=1)[0] == 0
    for kw in (dict(idle_ns=-1), dict(idle_ns=I64MIN), dict(max_msgs=0), dict(out_cap=255),
               dict(flags=0x2), dict(flags=0x40), dict(flags=0x80), dict(flags=0x400),
               dict(flags=0x80000000), dict(flags=0x200)):       # (count mode takes no buffer)
        rc, c, s = call(**kw)
        assert rc == -1, kw
        assert (c.slot, c.layout) == (0, 0), kw                  # a refused call moves nothing
    dev = torch.device("cuda", 0)
    d_out = torch.zeros(4096 + 16, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(9, dtype=torch.int64, device=dev)
    assert call(flags=1, o=d_out, f=d_offs)[0] == 0
    assert call(flags=1, o=d_out[1:], f=d_offs)[0] == -1        # misaligned
    assert call(flags=1, o=d_out, f=d_offs, out_cap=4092)[0] == -1   # not a multiple of 8
    assert call(flags=1, o=d_out, f=d_offs, out_cap=256)[0] == -1    # budget below one datagram
    assert call(flags=1, o=d_out, f=d_offs, out_cap=264, max_msgs=1)[0] == 0
    repo.close()


def device_round_trip(pa, a_rows, b_rows):
    import torch
    dev = torch.device("cuda", 0)
    A = pa.GPURepo(log2_slots=12, arena_bytes=1 << 16, hash_seed=1)
    B = pa.GPURepo(log2_slots=11, arena_bytes=1 << 16, hash_seed=2)
    seed(A, a_rows)
    seed(B, b_rows)
    o = O.Repo()
    ks = list(b_rows)
    o.seed(ks, *[[b_rows[k][j] for k in ks] for j in range(4)])
    model = SC.exported(gpu_dump(A))
    max_msgs = 192
    out = torch.zeros(8192, dtype=torch.uint8, device=dev)      # the byte cap binds too
    offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
    cursor, sent, now, calls = None, [], T0 + 77, 0
    while True:
        n, cursor, st = A.export_sweep_device(out, offs, cursor, max_msgs)
        calls += 1
        assert n <= max_msgs and st["bytes"] <= out.numel() - 8
        h_offs = offs[:n + 1].cpu().numpy()
        assert h_offs[0] == 0 and h_offs[-1] == st["bytes"]
        raw = out[:st["bytes"]].cpu().numpy().tobytes()
        dgs = [raw[h_offs[i]:h_offs[i + 1]] for i in range(n)]
        # the tensors go to the peer as they are
        assert B.receive_datagrams_device(out, offs, n, now) == n
        rs = o.receive(dgs, now)
        assert rs[4] == n and ((rs[0] & 0x7F) == 1).all()
        sent += dgs
        if st["done"]:
            break
    assert_exact(sent, model)
    assert calls > len(model) // max_msgs
    got = gpu_dump(B)
    assert got == o.dump()
    assert len(got) == len(set(b_rows) | set(model))
    A.close()
    B.close()


def ab_rows(rng, dirty):
    names = make_names(1500)
    gen = (lambda n: _gen.dirty_states(rng, n, p_special=0.3)) if dirty else \
        (lambda n: _gen.clean_states(rng, n))
    a, t, e = gen(len(names))
    a_rows = {nm: (int(a[i]), int(t[i]), int(e[i]), T0) for i, nm in enumerate(names)}
    b_names = names[::2] + [b"B-only-%d" % k for k in range(200)]
    a, t, e = gen(len(b_names))
    b_rows = {nm: (int(a[i]), int(t[i]), int(e[i]), T0 - 5) for i, nm in enumerate(b_names)}
    return a_rows, b_rows


@pytest.mark.parametrize("dirty", [False, True])
def test_device_round_trip(pa, dirty):
    """A swept with device pointers straight into B's receive: B ends as the
    oracle that received the same datagrams in the same order (with -0.0 and
    NaN fields in A: the receiver's ordered path)."""
    device_round_trip(pa, *ab_rows(np.random.default_rng(23 + dirty), dirty))


def finish_after_rebuild(repo, cursor, part):
    """The call after a rebuild restarts; looping on exports every non-zero
    bucket of the final table at least once, each datagram right."""
    dgs, cursor, st = repo.export_sweep(cursor, 64)
    assert st["restarted"] == 1
    check_call(dgs, st, 64, 256 * 64)
    rest = list(dgs)
    while not st["done"]:
        dgs, cursor, st = repo.export_sweep(cursor, 64)
        assert st["restarted"] == 0
        rest += dgs
    model = SC.exported(gpu_dump(repo))
    assert_exact(rest, model)            # the restarted sweep alone is complete and exact
    assert len(part) == 64
    return model


def partly_swept(pa):
    repo = kinds_table(pa, count=500, zeros=20)
    before = SC.exported(gpu_dump(repo))
    part, cursor, st = repo.export_sweep(None, 64)
    assert st["n"] == 64 and st["done"] == 0 and 0 < cursor[0] < 1024
    assert all(before[name_of(d)] == d for d in part)
    return repo, cursor, part, before


def test_rebuild_by_growth(pa):
    repo, cursor, part, before = partly_swept(pa)
    more = [b"grown-%d" % k for k in range(500)]
    a, t, e = _gen.clean_states(np.random.default_rng(2), 500)
    repo.receive_soa(more, a, t, e, T0 + 9)
    assert repo.capacity > 1024
    model = finish_after_rebuild(repo, cursor, part)
    assert set(before) | set(more) == set(model)
    repo.close()


def test_rebuild_by_eviction_moves_long_names(pa):
    repo, cursor, part, before = partly_swept(pa)
    # age out the 40-byte names: the 231-byte ones move down in the new arena
    # (elapsed is within 2^40 ns of zero but for the extremes: created 2^42 ns back is idle)
    old = {k: v[:3] + (T0 - (1 << 42),) for k, v in gpu_dump(repo).items() if len(k) == 40}
    seed(repo, old)
    rows = gpu_dump(repo)
    now, idle_ns = T0 + (1 << 41), 1 << 42
    st = repo.evict_idle(now, idle_ns)
    gone = {k for k, v in rows.items() if SC.idle_of(v[3], v[2], now) >= idle_ns}
    assert st["evicted"] == len(gone) >= len(old) - 2 > 40 and st["arena_freed"] > 0
    model = finish_after_rebuild(repo, cursor, part)
    assert sum(len(k) == 231 for k in model) >= 40 and not any(k in model for k in gone)
    repo.close()


def test_rebuild_by_restore(pa):
    repo, cursor, part, before = partly_swept(pa)
    img = repo.snapshot()
    repo.restore(img)                                   # same size: reloaded in place
    model = finish_after_rebuild(repo, cursor, part)
    assert model == before
    big = pa.GPURepo(log2_slots=12, arena_bytes=1 << 15)
    seed(big, {b"other-%d" % k: (SC.A1, SC.T1, k, T0) for k in range(50)})
    _, c2, s2 = big.export_sweep(None, 8)
    assert s2["done"] == 0
    big.restore(img)                                    # another size: the table is replaced
    assert big.capacity == 1024
    assert finish_after_rebuild(big, c2, part) == before
    big.close()
    repo.close()


def test_collisions(pa):
    """Three tag bits and a fixed seed: eight homes, every probe chain long;
    the sweep walks slots, so nothing changes."""
    repo = kinds_table(pa, log2_slots=9, count=240, zeros=10, debug_tag_bits=3, hash_seed=0)
    assert repo.table_stats()["max_probe"] >= 20
    model = SC.exported(gpu_dump(repo))
    assert len(model) >= 180
    one = repo.export_sweep(None, 512)[0]
    assert_exact(one, model)
    got, _, _ = sweep_all(repo, 16)
    assert got == one
    repo.close()


# ------------------------------------- a window of more than 512 tiles ----
@pytest.fixture(scope="module")
def chunk_table(pa):
    """SC.chunk_repo's table and its datagrams in slot order, taken in windows
    of 64 tiles: each is one chunk of the tile scan, none needs a carry.
    Shared, never changed."""
    repo = SC.chunk_repo(pa)
    model = SC.exported(gpu_dump(repo))
    assert len(model) == len(SC.chunk_rows()) and {len(k) for k in model} >= {0, 5, 22, 23, 231}
    ref, calls, sts = sweep_all(repo, 1 << 16, out_cap=SC.CHUNK_CAP)
    assert calls == 16 and all(s["slots_scanned"] == 64 * SC.TILE for s in sts)
    assert_exact(ref, model)
    yield repo, ref, sum(s["n"] for s in sts[:SC.CHUNK_TILES // 64])
    repo.close()


def one_call(repo, dev, cursor, max_msgs):
    """export_sweep with host or device pointers -> (datagrams, cursor, stats)."""
    if not dev:
        dgs, cursor, st = repo.export_sweep(cursor, max_msgs, out_cap=SC.CHUNK_CAP)
        check_call(dgs, st, max_msgs, SC.CHUNK_CAP)
        return dgs, cursor, st
    import torch
    out = torch.zeros(SC.CHUNK_CAP, dtype=torch.uint8, device="cuda:0")
    offs = torch.full((max_msgs + 1,), -1, dtype=torch.int64, device="cuda:0")
    n, cursor, st = repo.export_sweep_device(out, offs, cursor, max_msgs)
    st["offs"] = offs[:n + 1].cpu().numpy().view(np.uint64)
    raw = out[:st["bytes"]].cpu().numpy().tobytes()
    dgs = [raw[int(st["offs"][i]):int(st["offs"][i + 1])] for i in range(n)]
    check_call(dgs, st, max_msgs, SC.CHUNK_CAP - 8)
    return dgs, cursor, st


@pytest.mark.parametrize("dev", [False, True])
def test_window_past_one_chunk_of_the_tile_scan(chunk_table, dev):
    """max_msgs = 525312: one window of 513 tiles, so tile 512's rank and byte
    bases, and the totals, come through the scan's carry."""
    repo, ref, before512 = chunk_table
    first, cur, st = one_call(repo, dev, None, SC.CHUNK_MSGS)
    assert st["slots_scanned"] == (SC.CHUNK_TILES + 1) * SC.TILE > SC.CHUNK_TILES * SC.TILE
    assert (st["done"], st["restarted"], cur[0]) == (0, 0, st["slots_scanned"])
    # tile 512 alone (a window of one tile) holds records, and they end the call
    in512 = repo.export_sweep((SC.CHUNK_TILES * SC.TILE, cur[1]), 1024)[0]
    assert in512 and first[before512:] == in512
    assert first == ref[:len(first)]
    rest, cur, st = one_call(repo, dev, cur, SC.CHUNK_MSGS)
    assert (st["done"], cur[0]) == (1, repo.capacity)
    assert first + rest == ref
