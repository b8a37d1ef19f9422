"""PHIP_CFG_TRACK_CHANGES and phip_export_changed on the GPU (include/
patrolhip.h "Change set"), through the binding.

Every case runs its batches on a tracking handle and on tests/
_changes_cases.py's model over the oracle, drains, and compares the requests
and the states by name with the model (each section a name -> datagram map
with no name twice, offsets monotone from 0: _egress_cases.sections), and the
table dump with the oracle's.  Bit-exact throughout.
"""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _changes_cases as CC  # noqa: E402
from tests import _egress_cases as EC  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _group_ops as GO  # noqa: E402

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


def plain(repo, ops, **kw):
    return repo.apply_mixed(ops["kind"], ops["names"], ops["now"], ops["freq"], ops["per"],
                            ops["count"], ops["added"], ops["taken"], ops["elapsed"], **kw)


def apply(repo, m, ops):
    """A marking batch on the handle and on the model; the statuses agree."""
    res = plain(repo, ops)
    ref = m.batch(ops)
    assert np.array_equal(res["status"], ref["status"])
    return res


def check_call(d, max_msgs, out_cap):
    assert d["n"] <= max_msgs and d["bytes"] <= out_cap and d["n_incast"] <= d["n"]
    assert d["bytes"] == len(d["data"]) == int(d["offs"][d["n"]])
    assert d["done"] == (d["pending"] == 0)


def drain(repo, max_msgs=1 << 12, out_cap=None):
    """Loop export_changed until done -> (requests by name, states by name,
    calls); every request comes before any state across the loop, and no name
    twice in a section."""
    cap = 256 * max_msgs if out_cap is None else out_cap
    req, st, calls = {}, {}, []
    while True:
        d = repo.export_changed(max_msgs, out_cap)
        check_call(d, max_msgs, cap)
        r, s = EC.sections(d)
        assert not (set(r) & set(req)) and not (set(s) & set(st))
        assert not (r and st), "a request after a state"
        if s:
            assert d["pending"] == 0 or d["n_incast"] == len(r), d
        req.update(r)
        st.update(s)
        calls.append(d)
        assert len(calls) < 100000
        if d["done"]:
            return req, st, calls


def check_drain(repo, m, **kw):
    """Count mode, a full drain against the model, and an empty second call."""
    want_req, want_st = m.expected()
    cnt = repo.changes_count()
    assert cnt["n"] == len(want_req) + len(want_st) and cnt["n_incast"] == len(want_req)
    assert cnt["bytes"] == sum(map(len, want_req.values())) + sum(map(len, want_st.values()))
    assert cnt["pending"] == m.pending() and cnt["done"] == (m.pending() == 0)
    assert repo.changes_count() == cnt          # count mode clears nothing
    req, st, calls = drain(repo, **kw)
    print("drain: %d calls, %d requests + %d states (want %d + %d), %d marks"
          % (len(calls), len(req), len(st), len(want_req), len(want_st), cnt["pending"]))
    assert req == want_req
    assert st == want_st
    assert sum(d["n"] for d in calls) == cnt["n"] and sum(d["bytes"] for d in calls) == cnt["bytes"]
    assert sum(d["n_incast"] for d in calls) == cnt["n_incast"]
    again = repo.export_changed(16)
    assert (again["n"], again["n_incast"], again["bytes"], again["pending"], again["done"]) == \
        (0, 0, 0, 0, 1) and list(again["offs"]) == [0]
    m.drained()
    return calls


def tracked(pa, **kw):
    kw.setdefault("log2_slots", 12)
    return pa.GPURepo(track_changes=True, **kw), CC.Model(O.Repo())


# 1 ------------------------------------------------------------- small path --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_small_path(pa, n):
    rng = np.random.default_rng(n)
    g, m = tracked(pa)
    apply(g, m, EC.gen_ops(rng, n, EC.name_pool(40)))
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 2 ------------------------------------------------------------- large path --
@pytest.mark.parametrize("all_take", [False, True])
def test_large_path_host(pa, all_take):
    """5000 host ops on the multi-launch path; all TAKE: the uniform form."""
    rng = np.random.default_rng(200 + all_take)
    pool = EC.name_pool(400)
    g, m = tracked(pa, small=False)
    apply(g, m, EC.gen_ops(rng, 300, pool))
    check_drain(g, m)
    ops = EC.gen_ops(rng, 5000, pool, t0=T0 + 400 * SEC, all_take=all_take)
    g.set_timing(True)
    apply(g, m, ops)
    assert "k_changes_mark" in [k for k, _ in g.timings()]
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


def test_large_path_host_uniform_without_status(pa):
    """An all-TAKE host batch passed with no result columns at all."""
    from patrol_amd import _lib
    from patrol_amd.engine import names_blob
    rng = np.random.default_rng(210)
    ops = EC.gen_ops(rng, 5000, EC.name_pool(400), all_take=True)
    g, m = tracked(pa, small=False)
    blob, offs = names_blob(ops["names"])
    cols = {c: np.ascontiguousarray(ops[c]) for c in COLS}
    o = _lib.phip_ops(len(ops["names"]), 0, cols["kind"].ctypes.data, blob.ctypes.data,
                      offs.ctypes.data, *[cols[c].ctypes.data for c in COLS[1:]])
    assert g.L.phip_apply_mixed(g.h, C.byref(o), None, 0) == 0
    m.batch(ops)
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


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


def device_apply(repo, m, ops, with_status=True, names_len=None):
    import torch
    n = len(ops["names"])
    t = to_device(ops)
    status = torch.zeros(n, dtype=torch.uint8, device=t["names"].device) if with_status else None
    repo.apply_mixed_device(n, t["kind"], t["names"], t["name_offs"], t["now"], freq=t["freq"],
                            per=t["per"], count=t["count"], added=t["added"], taken=t["taken"],
                            elapsed=t["elapsed"], status=status, names_len=names_len)
    ref = m.batch(ops)
    if with_status:
        assert np.array_equal(status.cpu().numpy(), ref["status"])


def device_drain(repo, max_msgs=1 << 14, cap=None):
    """export_changed_device until done -> (requests, states, calls, last out, offs)."""
    import torch
    dev = torch.device("cuda", 0)
    cap = 256 * max_msgs + 8 if cap is None else cap
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    offs = torch.zeros(max_msgs + 1, dtype=torch.int64, device=dev)
    req, st, calls = {}, {}, []
    while True:
        d = repo.export_changed_device(out, offs, max_msgs)
        ho = offs.cpu().numpy().view(np.uint64)
        d["data"], d["offs"] = out.cpu().numpy()[:d["bytes"]], ho[:d["n"] + 1]
        check_call(d, max_msgs, cap - 8)
        r, s = EC.sections(d)
        assert not (set(r) & set(req)) and not (set(s) & set(st)) and not (r and st)
        req.update(r)
        st.update(s)
        calls.append(d)
        assert len(calls) < 100000
        if d["done"]:
            return req, st, calls, out, offs


@pytest.mark.parametrize("with_status,names_len", [(True, None), (False, None), (True, 0)])
def test_large_path_device(pa, with_status, names_len):
    rng = np.random.default_rng(21)
    pool = EC.name_pool(400)
    g, m = tracked(pa)
    apply(g, m, EC.gen_ops(rng, 300, pool))
    device_apply(g, m, EC.gen_ops(rng, 5000, pool, t0=T0 + 400 * SEC), with_status, names_len)
    want_req, want_st = m.expected()
    cnt = g.changes_count()
    req, st, calls, _, _ = device_drain(g)
    assert len(calls) == 1 and (req, st) == (want_req, want_st)
    assert (calls[0]["n"], calls[0]["n_incast"], calls[0]["bytes"]) == \
        (cnt["n"], cnt["n_incast"], cnt["bytes"])
    assert g.changes_count()["pending"] == 0
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 3 -------------------------------------------------------- segment classes --
def interleave(rng, seqs):
    labels = np.repeat(np.arange(len(seqs)), [len(s) for s in seqs])
    rng.shuffle(labels)
    pos = [0] * len(seqs)
    out = []
    for b in labels:
        out.append(seqs[b][pos[b]])
        pos[b] += 1
    return out


def build_ops(rng, stream, t0=T0):
    """[(name, kind)] -> ops: takes at 100:1s, replicas with clean non-zero states."""
    n = len(stream)
    a, t, e = _gen.clean_states(rng, n)
    return dict(names=[s[0] for s in stream], kind=np.array([s[1] for s in stream], np.uint8),
                now=t0 + np.cumsum(rng.integers(0, 2_000_000, n)).astype(np.int64),
                freq=np.full(n, 100, np.int64), per=np.full(n, SEC, np.int64),
                count=rng.integers(1, 3, n).astype(np.uint64), added=a, taken=t, elapsed=e)


def test_segment_classes(pa):
    """A bucket of 33 ops (one wave) and one of 32769 (one workgroup), every op
    a RECEIVE but the last, a TAKE; RECEIVE-only buckets of both classes; a
    bucket a TAKE created and 40 RECEIVEs merged into; thread-folded buckets of
    every kind beside them."""
    rng = np.random.default_rng(32)
    sizes = (33, 32769)
    seqs = [[(b"seg%d" % c, EC.RECEIVE)] * (c - 1) + [(b"seg%d" % c, EC.TAKE)] for c in sizes]
    seqs += [[(b"quiet40", EC.RECEIVE)] * 40, [(b"quiet33000", EC.RECEIVE)] * 33000]
    seqs += [[(b"made", EC.TAKE)] + [(b"made", EC.RECEIVE)] * 40]
    seqs += [[(b"one%d" % i, (EC.TAKE, EC.RECEIVE, EC.UPSERT)[i % 3])] for i in range(99)]
    g, m = tracked(pa, log2_slots=10)
    apply(g, m, build_ops(rng, interleave(rng, seqs)))
    want_req, want_st = m.expected()
    assert b"quiet40" not in want_st and b"quiet33000" not in want_st
    assert all(b"seg%d" % c in want_st and b"seg%d" % c not in want_req for c in sizes)
    assert b"made" in want_req and b"made" in want_st
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 4 ------------------------------------------------- dense words, tile edges --
def tile_names(k):
    L = (5, 14, 22, 23, 40)[k % 5]
    return (b"%05d" % k).ljust(L, b"t")


@pytest.mark.parametrize("small", [True, False])
def test_dense_words(pa, small):
    """About 100 buckets in 128 slots: most lanes of a marking wave share their
    word with their neighbours."""
    rng = np.random.default_rng(40)
    names = [tile_names(k) for k in range(100)]
    kinds = [(EC.TAKE, EC.TAKE, EC.UPSERT, EC.RECEIVE)[k % 4] for k in range(100)]
    g, m = tracked(pa, log2_slots=7, hash_seed=12345, small=small, max_load_pct=95)
    order = rng.permutation(100)
    apply(g, m, build_ops(rng, [(names[k], kinds[k]) for k in order]))
    assert g.capacity == 128
    assert m.pending() == 75 + 50
    check_drain(g, m)
    g.close()


@pytest.mark.parametrize("K", [4095, 4096, 4097, 8193])
def test_tile_edges(pa, K):
    """K distinct buckets named once each in 2^15 slots, every other one new."""
    rng = np.random.default_rng(K)
    names = [tile_names(k) for k in range(K)]
    g, m = tracked(pa, log2_slots=15, hash_seed=777)
    apply(g, m, build_ops(rng, [(nm, EC.TAKE) for nm in names[::2]]))
    check_drain(g, m)
    kinds = [(EC.UPSERT if k % 7 == 3 else EC.TAKE) for k in range(K)]
    order = rng.permutation(K)
    apply(g, m, build_ops(rng, [(names[k], kinds[k]) for k in order], t0=T0 + 100 * SEC))
    want_req, want_st = m.expected()
    assert len(want_st) == K and len(want_req) == sum(1 for k in range(1, K, 2) if kinds[k] == EC.TAKE)
    check_drain(g, m)
    assert g.capacity == 1 << 15
    g.close()


@pytest.mark.parametrize("log2_slots", [21, 22])
def test_scan_past_one_chunk_of_the_tile_scan(pa, log2_slots):
    """k_egress_scan walks 2 * ntiles entries in chunks of 512, the requests'
    tiles in front, and stores the requests' total from entry ntiles.  2^21
    slots are 512 tiles: the requests fill the first chunk, and entry 512, the
    first of the second, is the carry itself.  2^22 slots: the requests' tiles
    lie on both sides of a chunk's edge and the boundary opens the third chunk.
    One mixed batch that leaves requests and states pending, count mode, one
    export_changed of everything."""
    rng = np.random.default_rng(log2_slots)
    g, m = tracked(pa, log2_slots=log2_slots)
    apply(g, m, EC.gen_ops(rng, 5000, EC.name_pool(3000)))
    want_req, want_st = m.expected()
    assert len(want_req) >= 100 and len(want_st) >= 200
    ntiles = g.capacity // 4096
    assert g.capacity == 1 << log2_slots and 2 * ntiles > 512
    # the table's upper half in slot order (one sweep window): requests are
    # pending in tiles on both sides of ntiles / 2 (2^22 slots: of tile 512)
    half = g.capacity // 2
    layout = g.export_sweep(None, 1)[1][1]
    dgs, cur, st = g.export_sweep((half, layout), half // 4, out_cap=1 << 20)
    assert (st["slots_scanned"], st["done"]) == (half, 1)
    upper = {d[EC.FIXED:] for d in dgs}
    assert 20 <= len(upper & set(want_req)) <= len(want_req) - 20
    calls = check_drain(g, m, max_msgs=1 << 13)
    assert len(calls) == 1 and calls[0]["n_incast"] == len(want_req)
    assert g.changes_count()["pending"] == 0
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 5 ----------------------------------------------------------- accumulation --
def test_accumulation_with_receives_between(pa):
    """Three apply_mixed batches with receive_soa batches between them: merges
    that raise marked and unmarked buckets, incasts, and buckets only Receive
    ever names.  One drain equals the model."""
    rng = np.random.default_rng(50)
    pool = EC.name_pool(120)
    g, m = tracked(pa, log2_slots=10)
    t0 = T0
    only = [b"only-received-%d" % i for i in range(30)]
    for k in range(3):
        ops = EC.gen_ops(rng, 700, pool[:40 * (k + 1)], t0=t0)
        t0 = int(ops["now"][-1]) + 1
        apply(g, m, ops)
        names = [pool[int(i)] for i in rng.integers(0, len(pool), 300)] + only
        a, t, e = _gen.clean_states(rng, len(names))
        z = rng.random(len(names)) < 0.1   # incasts
        a[z], t[z], e[z] = 0, 0, 0
        got = g.receive_soa(names, a, t, e, t0)
        ref = m.receive_soa(names, a, t, e, t0)
        assert np.array_equal(got["status"], ref[0])
    req, st = m.expected()
    assert not any(nm in req or nm in st for nm in only)
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 6 --------------------------------------------------------- bounded drains --
@pytest.mark.parametrize("max_msgs,out_cap", [(1, None), (7, None), (64, None), (4096, 256)])
def test_bounded_drains_host(pa, max_msgs, out_cap):
    rng = np.random.default_rng(60)
    g, m = tracked(pa, log2_slots=10)
    apply(g, m, EC.gen_ops(rng, 1500, EC.name_pool(150)))
    calls = check_drain(g, m, max_msgs=max_msgs, out_cap=out_cap)
    assert len(calls) > 1
    pend = [d["pending"] for d in calls]
    assert pend == sorted(pend, reverse=True) and pend[-1] == 0
    g.close()


@pytest.mark.parametrize("max_msgs,cap", [(7, None), (4096, 256 + 8)])
def test_bounded_drains_device(pa, max_msgs, cap):
    rng = np.random.default_rng(61)
    g, m = tracked(pa, log2_slots=10)
    apply(g, m, EC.gen_ops(rng, 1500, EC.name_pool(150)))
    want_req, want_st = m.expected()
    cnt = g.changes_count()
    req, st, calls, _, _ = device_drain(g, max_msgs, cap)
    assert (req, st) == (want_req, want_st) and len(calls) > 1
    assert sum(d["n"] for d in calls) == cnt["n"] and sum(d["bytes"] for d in calls) == cnt["bytes"]
    assert calls[-1]["pending"] == 0
    g.close()


def test_argument_errors_clear_nothing(pa):
    import torch
    rng = np.random.default_rng(62)
    g, m = tracked(pa, log2_slots=10)
    apply(g, m, EC.gen_ops(rng, 300, EC.name_pool(40)))
    before = g.changes_count()
    dev = torch.device("cuda", 0)
    out = torch.zeros(4096, dtype=torch.uint8, device=dev)
    offs = torch.zeros(17, dtype=torch.int64, device=dev)
    for call in (lambda: g.export_changed(0), lambda: g.export_changed(4, out_cap=255),
                 lambda: g.export_changed_device(out[1:1025], offs, 16),
                 lambda: g.export_changed_device(out[:260], offs, 16),
                 lambda: g.export_changed_device(out[:256], offs, 16)):
        with pytest.raises(pa.PatrolHipError) as e:
            call()
        assert e.value.code == -1
    from patrol_amd import _lib
    st = _lib.phip_changes_stats()
    assert g.L.phip_export_changed(g.h, None, 0, None, 0, C.byref(st), 0x40) == -1   # unknown flag
    assert g.changes_count() == before and int(out.sum()) == 0
    check_drain(g, m)
    g.close()


# 7 ----------------------------------------------------------------- growth --
def test_growth_between_mark_and_drain(pa):
    """16 slots at open: the first batch names 300 buckets and rehashes the
    table inside the batch, the second grows it again; the marks moved along."""
    rng = np.random.default_rng(70)
    g, m = tracked(pa, log2_slots=4)
    assert g.capacity == 16
    apply(g, m, EC.gen_ops(rng, 3000, EC.name_pool(300)))
    cap1 = g.capacity
    pool2 = [b"second-%d" % i for i in range(2000)]
    apply(g, m, EC.gen_ops(rng, 4000, pool2, t0=T0 + 400 * SEC))
    assert g.capacity > cap1 > 16
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


def test_growth_on_the_small_path_between_mark_and_drain(pa):
    """Small batches mark; a later batch over the load limit rehashes."""
    rng = np.random.default_rng(71)
    g, m = tracked(pa, log2_slots=6)
    t0 = T0
    for k in range(6):
        ops = EC.gen_ops(rng, 40, [b"g%d-%d" % (k, i) for i in range(30)], t0=t0)
        t0 = int(ops["now"][-1]) + 1
        apply(g, m, ops)
    assert g.capacity > 64
    check_drain(g, m)
    g.close()


# 8 --------------------------------------------------------------- eviction --
def test_eviction_between_mark_and_drain_then_restore(pa):
    rng = np.random.default_rng(80)
    g, m = tracked(pa, log2_slots=10)
    old = [b"old-%d" % i for i in range(150)] + [b"O" * 40 + b"%d" % i for i in range(20)]
    new = [b"new-%d" % i for i in range(200)] + [b"N" * 40 + b"%d" % i for i in range(20)]
    apply(g, m, build_ops(rng, [(nm, EC.TAKE) for nm in old]))
    apply(g, m, build_ops(rng, [(nm, (EC.TAKE, EC.UPSERT)[i % 2]) for i, nm in enumerate(new)],
                          t0=T0 + 1000 * SEC))
    snap = g.snapshot()
    before = gpu_dump(g)
    # the upserted states carry elapsed values of their own: the rule decides who goes
    st = g.evict_idle(T0 + 1001 * SEC, 500 * SEC)
    after = gpu_dump(g)
    gone = set(before) - set(after)
    assert st["evicted"] == len(gone) and set(old) <= gone and 0 < len(after) < len(before)
    assert {nm for i, nm in enumerate(new) if i % 2 == 0} <= set(after)   # fresh takes stay
    m.evict(gone)
    want_req, want_st = m.expected()
    assert set(want_st) <= set(after) and set(want_req) <= set(after)
    check_drain(g, m)
    # marks again, then a restore clears the set
    apply(g, m, build_ops(rng, [(b"new-%d" % i, EC.TAKE) for i in range(0, 200, 2)],
                          t0=T0 + 1002 * SEC))
    assert g.changes_count()["pending"] > 0
    g.restore(snap)
    assert gpu_dump(g) == before
    d = g.export_changed(64)
    assert (d["n"], d["pending"], d["done"]) == (0, 0, 1)
    g.close()


def test_restore_of_another_table_size_clears_the_set(pa):
    rng = np.random.default_rng(81)
    src = pa.GPURepo(log2_slots=8)
    plain(src, EC.gen_ops(rng, 200, EC.name_pool(100)))
    snap = src.snapshot()
    src.close()
    g, m = tracked(pa, log2_slots=10)
    apply(g, m, EC.gen_ops(rng, 300, EC.name_pool(40)))
    g.restore(snap)
    assert g.capacity == 256
    d = g.export_changed(64)
    assert (d["n"], d["pending"], d["done"]) == (0, 0, 1)
    ops = build_ops(rng, [(b"after-restore", EC.TAKE)], t0=T0 + 900 * SEC)
    plain(g, ops)
    req, st, _ = drain(g)
    assert list(req) == [b"after-restore"] and list(st) == [b"after-restore"]
    g.close()


# 9 --------------------------------------------------------- tag collisions --
def test_tag_collisions(pa):
    rng = np.random.default_rng(90)
    g, m = tracked(pa, debug_tag_bits=3)
    apply(g, m, EC.gen_ops(rng, 900, EC.name_pool(200)))
    apply(g, m, EC.gen_ops(rng, 3000, EC.name_pool(200), t0=T0 + 400 * SEC))
    check_drain(g, m)
    assert gpu_dump(g) == m.o.dump()
    g.close()


# 10 ------------------------------------------------------------ off and on --
def kernel_names(repo, ops):
    repo.set_timing(True)
    plain(repo, ops)
    names = [k for k, _ in repo.timings()]
    repo.set_timing(False)
    return names


def test_untracked_handle_is_unchanged(pa):
    rng = np.random.default_rng(100)
    pool = EC.name_pool(200)
    small_ops = EC.gen_ops(rng, 500, pool)
    large_ops = EC.gen_ops(rng, 5000, pool, t0=T0 + 400 * SEC)
    off, (on, m) = pa.GPURepo(log2_slots=12), tracked(pa)
    with pytest.raises(pa.PatrolHipError) as e:
        off.export_changed(16)
    assert e.value.code == -1
    with pytest.raises(pa.PatrolHipError):
        off.changes_count()
    s_off, s_on = kernel_names(off, small_ops), kernel_names(on, small_ops)
    assert s_off == ["k_small_mixed"] and s_on == ["k_small_mixed"]
    l_off, l_on = kernel_names(off, large_ops), kernel_names(on, large_ops)
    assert not any(k.startswith("k_change") or k.startswith("k_egress") for k in l_off), l_off
    assert "k_changes_mark" in l_on
    extra = [k for k in l_on if k not in ("k_changes_mark", "k_egress_wants")]
    assert sorted(extra) == sorted(l_off), (l_off, l_on)   # the marks are all that was added
    m.batch(small_ops)
    m.batch(large_ops)
    check_drain(on, m)
    assert gpu_dump(on) == gpu_dump(off)
    off.close()
    on.close()


def test_egress_call_marks_nothing(pa):
    rng = np.random.default_rng(101)
    pool = EC.name_pool(200)
    for small in (True, False):
        g, m = tracked(pa, small=small)
        apply(g, m, EC.gen_ops(rng, 200, pool[:50]))
        ops = EC.gen_ops(rng, 900, pool, t0=T0 + 400 * SEC)
        res = plain(g, ops, egress=True)
        m.unmarked(ops)
        assert res["egress"]["n"] > 0
        check_drain(g, m)
        g.close()


def test_upsert_soa_seed_and_receive_mark_nothing(pa):
    rng = np.random.default_rng(102)
    g = pa.GPURepo(log2_slots=10, track_changes=True)
    names = [b"u%d" % i for i in range(300)]
    a, t, e = _gen.clean_states(rng, 300)
    g.upsert_soa(names, a, t, e, T0)
    g.seed([b"s%d" % i for i in range(50)], a[:50], t[:50], e[:50], np.full(50, T0))
    g.receive_soa([b"r%d" % i for i in range(300)], a, t, e, T0)
    g.receive_datagrams([EC.marshal(b"d%d" % i, a[i], t[i], e[i]) for i in range(100)], T0)
    assert len(g) == 750
    d = g.export_changed(64)
    assert (d["n"], d["pending"], d["done"]) == (0, 0, 1)
    g.close()


def test_refused_batch_marks_nothing(pa):
    """PHIP_CFG_NO_GROW: a batch whose new buckets pass the load limit is
    refused before any claim, on both paths, and leaves no mark."""
    rng = np.random.default_rng(103)
    for small in (True, False):
        g, m = tracked(pa, log2_slots=6, grow=False, small=small)
        apply(g, m, build_ops(rng, [(b"fits-%d" % i, EC.TAKE) for i in range(20)]))
        check_drain(g, m)
        with pytest.raises(pa.PatrolHipError) as e:
            plain(g, build_ops(rng, [(b"fits-%d" % (i % 20), EC.TAKE) for i in range(40)] +
                                    [(b"too-many-%d" % i, EC.TAKE) for i in range(100)],
                               t0=T0 + 400 * SEC))
        assert e.value.code == -3
        d = g.export_changed(64)
        assert (d["n"], d["pending"], d["done"]) == (0, 0, 1)
        g.close()


# 11 ------------------------------------------------------------ round trip --
def test_round_trip_into_a_peer(pa):
    """Three monotone TAKE-only batches (tests/test_changes_abi.py shows the
    premise on the oracle), one device drain, its buffers unchanged into a
    second handle's receive_datagrams_device: the peer equals an oracle peer
    that received the reference's per-op broadcasts."""
    rng = np.random.default_rng(110)
    ops = EC.monotone_takes(rng, 6000, 800)
    whole = EC.call(O.Repo(), ops)
    EC.assert_monotone(ops, whole)
    g, m = tracked(pa)
    peer = pa.GPURepo(log2_slots=12)
    for b in CC.split(ops, [1000, 2500]):
        apply(g, m, b)
    want_req, want_st = m.expected()
    req, st, calls, out, offs = device_drain(g)
    assert (req, st) == (want_req, want_st) and len(calls) == 1
    now = int(ops["now"][-1]) + 1
    assert peer.receive_datagrams_device(out, offs, calls[0]["n"], now) == calls[0]["n"]
    want = O.Repo()
    per_op = EC.per_op_broadcasts(ops, whole)
    assert want.receive(per_op, now)[4] == len(per_op)
    assert gpu_dump(peer) == want.dump()
    g.close()
    peer.close()


# 12 ----------------------------------------------------------------- group --
def _owners(names, world):
    import torch
    from oracle import go_semantics as G
    from patrol_amd import shard
    h = np.array([G.fnv1a64(nm) for nm in names], np.uint64).view(np.int64)
    return shard.owner_of(torch.from_numpy(h), world).numpy().astype(np.int64)


def _dev_batch(b):
    import torch
    from patrol_amd.engine import names_blob
    dev = torch.device("cuda", 0)
    blob, offs = names_blob(b["names"])
    d = dict(names=torch.from_numpy(blob).to(dev),
             name_offs=torch.from_numpy(offs.view(np.int32)).to(dev))
    for c in GO.COLS:
        x = np.ascontiguousarray(b[c])
        d[c] = torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    return d


@pytest.mark.parametrize("world", [2, 1])
def test_group_owners_egress(pa, world):
    """A shared-device group with track_changes: ops for every owner arrive at
    every member, in rounds of 4096; each member's drain holds only buckets it
    owns and the union is the model's.  World 1 runs through the RCCL
    self-exchange."""
    rng = np.random.default_rng(120 + world)
    pool = GO.name_pool(300)
    g = pa.GPUGroup.open_all([0] * world, log2_slots=12, track_changes=True)
    batches = [GO.gen_ops(rng, 6000, pool) for _ in range(world)]
    sizes = [len(b["names"]) for b in batches]
    order = GO.apply_order(sizes, GO.SMALL_CHUNK)
    m = CC.Model(O.Repo())
    m.batch(GO.sorted_ops(batches, order))
    g.apply_mixed([_dev_batch(b) for b in batches], rccl_self=(world == 1), small_chunks=True)
    want_req, want_st = m.expected()
    got_req, got_st = {}, {}
    for r, repo in enumerate(g.repos):
        req, st, _ = drain(repo)
        for nm in list(req) + list(st):
            assert _owners([nm], world)[0] == r, (nm, r)
        assert not (set(req) & set(got_req)) and not (set(st) & set(got_st))
        got_req.update(req)
        got_st.update(st)
        assert repo.changes_count()["pending"] == 0
    assert got_req == want_req
    assert got_st == want_st
    if world > 1:
        assert all(len(repo) for repo in g.repos)
    g.close()


# 13 --------------------------------------------------------------- batcher --
def test_batcher_marks(pa):
    """8 threads x 100 takes over 60 names through a TakeBatcher on a tracked
    repo, 20 of the names present before: after close() the drain's states are
    exactly the names taken from and its requests exactly the names created."""
    threads, per_thread = 8, 100
    repo = pa.GPURepo(log2_slots=10, track_changes=True)
    known = [b"b%d" % i for i in range(20)]
    a, t, e = _gen.clean_states(np.random.default_rng(1), 20)
    repo.upsert_soa(known, a, t, e, T0)          # marks nothing
    b = pa.TakeBatcher(repo, window_us=200, max_batch=256)
    rng = np.random.default_rng(130)
    plan = [[(b"b%d" % int(i), T0 + int(k) * 1000, 100, SEC, 1)
             for k, i in enumerate(rng.integers(0, 60, per_thread))] for _ in range(threads)]
    created = [[] for _ in range(threads)]

    def worker(tid):
        for req in plan[tid]:
            r = b.take_reply(*req)
            if r["created"]:
                created[tid].append(req[0])

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(threads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert b.stats()["errors"] == 0
    b.close()
    taken = {req[0] for p in plan for req in p}
    made = sorted(nm for c in created for nm in c)
    assert made == sorted(taken - set(known))
    cnt = repo.changes_count()
    assert cnt["pending"] == len(taken) + len(made)
    req, st, _ = drain(repo)
    dump = gpu_dump(repo)
    assert sorted(req) == made
    assert st == {nm: EC.marshal(nm, *dump[nm][:3]) for nm in taken}
    repo.close()
