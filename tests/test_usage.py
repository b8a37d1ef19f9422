"""phip_usage_mark, metric PHIP_TOP_SINCE_MARK and PHIP_TOP_MARK on the GPU
(include/patrolhip.h "Windowed top talkers"), through the binding.

What a call must report is tests/_usage_cases.py's reference: the contract
restated in Python over two dumps of the table, the rows at the mark and the
rows now -- never the library.  The slot tie-break does not show in a dump, so
a result is checked by the prefix property (top(k) is the head of top(k')) and
by UC.check()'s set conditions.  Tables of 2^10 slots under 3-bit tags.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import _top_cases as TP  # noqa: E402
from tests import _usage_cases as UC  # noqa: E402

T0, SEC = TP.T0, TP.SEC
FILL = 0x5A
FILL64 = 0x5A5A5A5A5A5A5A5A
INVALID = -1
KS = [1, 7, 64, 600, 4096]


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def gpu_rows(repo):
    d = TP.rows_of(repo.dump())
    assert len(repo) == len(d), (len(repo), len(d))
    return d


def seeded(pa, names, cols, **kw):
    kw.setdefault("log2_slots", 10)
    kw.setdefault("hash_seed", 11)
    kw.setdefault("debug_tag_bits", 3)
    kw.setdefault("track_usage", True)
    g = pa.GPURepo(**kw)
    g.seed(names, *cols)
    assert len(g) == len(names)
    return g


def device_top(g, k, cap, prefix=b"", now=0, idle_ns=0, metric=1, mark=False):
    import torch
    dev = torch.device("cuda", 0)
    names = torch.full((cap,), FILL, dtype=torch.uint8, device=dev)
    offs = torch.full((k + 1,), FILL64, dtype=torch.int64, device=dev)
    taken = torch.full((k,), FILL64, dtype=torch.int64, device=dev)
    state = torch.full((k, 4), FILL64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    st = g.top_device(k, names, offs, taken, state, prefix, now, idle_ns, metric=metric, mark=mark)
    torch.cuda.synchronize()
    return (st, names.cpu().numpy(), offs.cpu().numpy().view(np.uint64),
            taken.cpu().numpy().view(np.uint64), state.cpu().numpy())


def device_entries(st, names, offs, taken, state):
    n = st["n"]
    raw = names.tobytes()
    return [(raw[int(offs[i]):int(offs[i + 1])], int(taken[i]),
             (int(state[i][0]) & (2**64 - 1), int(state[i][1]) & (2**64 - 1), int(state[i][2]),
              int(state[i][3]))) for i in range(n)]


def assert_untouched_past(st, names, offs, taken, state):
    n = st["n"]
    assert offs[0] == 0 and int(offs[n]) == st["bytes"]
    assert (names[st["bytes"]:] == FILL).all() and (offs[n + 1:] == FILL64).all()
    assert (taken[n:] == FILL64).all() and (state[n:] == FILL64).all()


def top1(g, k, *a, **kw):
    kw.setdefault("state", True)
    return g.top(k, *a, metric=1, **kw)


# ------------------------------------------------------ 1. before any mark ----
@pytest.mark.parametrize("k", [1, 64, 4096])
def test_before_any_mark_metric_1_is_metric_0(pa, k):
    names, cols, rows = TP.distinct_table(7, 600)
    g = seeded(pa, names, cols)
    assert gpu_rows(g) == rows
    m0, m1 = g.top(k, state=True), top1(g, k)
    assert TP.entries(m1) == TP.entries(m0) == TP.check(m0, rows, k)
    UC.check(m1, {}, rows, k)
    for f in ("n", "bytes", "population", "truncated"):
        assert m1[f] == m0[f], f
    d0, d1 = device_top(g, k, 231 * min(k, 700), metric=0), device_top(g, k, 231 * min(k, 700))
    assert device_entries(*d1) == device_entries(*d0) == TP.entries(m0)
    assert_untouched_past(*d1)
    assert g.top_count(metric=1)["population"] == g.top_count()["population"] == 600
    g.close()


# --------------------------------------------------------- 2. activity parity ----
P_ORG = b"org:"
IDLE_NOW, IDLE_NS = UC.TAKE_NOW, 4500 * SEC
FILTERS = [(b"", 0, 0), (P_ORG, 0, 0), (b"", IDLE_NOW, IDLE_NS)]


@pytest.fixture(scope="module")
def active(pa):
    """The recipe of tests/_usage_cases.plan through real calls: seed, mark,
    then receive merges, takes and one mixed batch.  Shared, never changed."""
    names, cols, rows, steps = UC.plan()
    g = seeded(pa, names, cols)
    assert g.capacity == 1024 and gpu_rows(g) == rows
    st = g.usage_mark()
    # nothing was marked before: every seeded bucket took something since its beginning
    assert st == dict(buckets=600, active=UC.active({}, rows))
    assert g.top_count(metric=1)["population"] == 0
    UC.apply_steps(g, steps)
    now_rows = gpu_rows(g)
    assert g.capacity == 1024
    model = UC.run_model(rows, steps)
    assert {nm: r[1] for nm, r in now_rows.items()} == {nm: r[1] for nm, r in model.items()}
    yield g, rows, now_rows
    g.close()


@pytest.mark.parametrize("flt", FILTERS, ids=["all", "prefix", "idle"])
def test_activity_parity(active, flt):
    g, rows, now_rows = active
    ref = UC.reference(rows, now_rows, *flt)
    assert len(ref) >= 20
    longest = UC.check(top1(g, 4096, *flt), rows, now_rows, 4096, *flt)
    assert len(longest) == len(ref)
    for k in KS:
        d = top1(g, k, *flt)
        got = UC.check(d, rows, now_rows, k, *flt)
        assert got == longest[:k]                       # the prefix property
        assert 1 <= d["passes"] <= 8
        # state is the record: its taken is the current total, not the difference
        assert all(s[1] == now_rows[nm][1] for nm, _, s in got)
        # the device form: the same list, nothing written past it
        dv = device_top(g, k, 231 * min(k, 700), *flt)
        assert device_entries(*dv) == got
        assert_untouched_past(*dv)
    cnt = g.top_count(*flt, metric=1)
    assert (cnt["population"], cnt["passes"], cnt["n"], cnt["bytes"]) == (len(ref), 1, 0, 0)
    # metric 0 is what it was: the lifetime totals
    TP.check(g.top(64, *flt, state=True), now_rows, 64, *flt)


# --------------------------------------------------------------- 3. edges ----
@pytest.mark.parametrize("s", TP.SHIFTS)
def test_edges(pa, s):
    names, base, taken = UC.edge_table(s)
    g = seeded(pa, names, UC.edge_cols(base), hash_seed=5 + s, debug_tag_bits=0)
    mark_rows = gpu_rows(g)
    assert mark_rows == UC.edge_rows(names, base)
    g.usage_mark()
    g.seed(names, *UC.edge_cols(taken))        # (seed overwrites: NaN and +Inf go in as they are)
    now_rows = gpu_rows(g)
    assert now_rows == UC.edge_rows(names, taken)
    want = UC.edge_expected(s)
    full = top1(g, 4096)
    got = UC.check(full, mark_rows, now_rows, 4096)
    assert [(nm, t) for nm, t, _ in got] == want
    assert full["population"] == len(want) == 19
    assert got[0][:2] == (b"inf-finite", TP.INF) and got[-1][:2] == (b"denormal", 1)
    for k in range(1, len(want) + 1):           # every cut
        d = top1(g, k)
        assert [(nm, t) for nm, t, _ in UC.check(d, mark_rows, now_rows, k)] == want[:k]
        assert d["passes"] <= 8
    st = g.usage_mark()
    assert st == dict(buckets=len(names), active=len(want))
    g.close()


# ---------------------------------------------------------------- 4. ties ----
def test_ties_every_cut_inside_a_group(active):
    g, rows, now_rows = active
    ref = UC.reference(rows, now_rows)
    full = UC.check(top1(g, 4096), rows, now_rows, 4096)
    keys = [e[1] for e in full]
    groups = UC.tie_groups(ref)
    assert len(groups) >= 10
    cuts = set()
    for key, members in groups.items():
        lo = keys.index(key)
        assert keys[lo:lo + len(members)] == [key] * len(members)
        assert {e[0] for e in full[lo:lo + len(members)]} == set(members)
        cuts.update(range(lo, lo + len(members) + 1))
    assert len(cuts) >= 100
    for k in sorted(cuts | {c + 1 for c in cuts}):         # top(k) and top(k + 1) at every cut
        if 1 <= k <= len(full):
            assert TP.entries(top1(g, k)) == full[:k], k


# ----------------------------------------------- 5. rebuilds carry the baseline ----
@pytest.mark.parametrize("shrink", [False, True])
def test_rebuilds_carry_the_baseline(pa, shrink):
    names, cols, rows, steps = UC.plan()
    g = seeded(pa, names, cols)
    g.usage_mark()
    UC.apply_steps(g, steps)
    before = UC.check(top1(g, 4096), rows, gpu_rows(g), 4096)
    # growth: 2 000 new names, received with an old clock so that they idle later
    m = 2000
    more = [b"grown-%d" % i for i in range(m)]
    tm = (np.arange(m) % 97 + 1).astype(np.float64)
    g.receive_soa(more, (tm + 1).view(np.uint64).copy(), tm.view(np.uint64).copy(),
                  np.ones(m, np.int64), T0)
    assert g.last_stats()[3] >= 1 and g.capacity > 1024          # the table was rehashed
    grown_rows = gpu_rows(g)
    assert len(grown_rows) == 650 + m
    after = UC.check(top1(g, 4096), rows, grown_rows, 4096)
    # the old buckets kept their differences through the rehash, name by name
    old = {nm: t for nm, t, _ in before}
    assert {nm: t for nm, t, _ in after if nm in old} == old
    assert sum(nm.startswith(b"grown-") for nm, _, _ in after) == m
    # eviction: everything last touched before T0 + 4000 s goes (the untouched,
    # the receive-merged and the grown ones); the takes' buckets stay
    cap0 = g.capacity
    ev = g.evict_idle(T0 + 6000 * SEC, 2000 * SEC, shrink=shrink)
    kept_rows = gpu_rows(g)
    assert ev["evicted"] == 650 + m - len(kept_rows) and 100 <= len(kept_rows) <= 200
    assert g.capacity == (1024 if shrink else cap0)
    kept_mark = {nm: r for nm, r in rows.items() if nm in kept_rows}
    got = UC.check(top1(g, 4096), kept_mark, kept_rows, 4096)
    assert {nm: t for nm, t, _ in got} == {nm: t for nm, t in old.items() if nm in kept_rows}
    assert len(got) == len(kept_rows)
    # an evicted bucket that is taken again counts from zero, not from its old baseline
    back = names[0]
    assert back in rows and back not in kept_rows and TP.qualifies(back, rows[back])
    g.take([back], [T0 + 6001 * SEC], [UC.FREQ], [UC.PER], [2])
    rows2 = gpu_rows(g)
    assert rows2[back][1] == TP.f2b(2.0)
    got2 = UC.check(top1(g, 4096), kept_mark, rows2, 4096)
    assert dict((nm, t) for nm, t, _ in got2)[back] == TP.f2b(2.0)
    g.close()


# -------------------------------------------------------- 6. restore clears ----
def test_restore_clears_the_baseline(pa):
    names, cols, rows, steps = UC.plan()
    g = seeded(pa, names, cols)
    plain = seeded(pa, names, cols, track_usage=False)
    snap = g.snapshot()
    assert snap.size == plain.snapshot().size          # the image does not hold the column
    plain.close()
    g.usage_mark()
    UC.apply_steps(g, steps)
    assert 0 < top1(g, 4096)["population"] < 600
    g.restore(snap)
    assert gpu_rows(g) == rows
    for k in (1, 64, 4096):
        m0, m1 = g.top(k, state=True), top1(g, k)
        assert TP.entries(m1) == TP.entries(m0) == TP.check(m0, rows, k)
    assert g.snapshot().size == snap.size
    g.close()


# ------------------------------------------------------------ 7. mark=True ----
def test_mark_in_the_same_call(pa):
    names, cols, rows, steps = UC.plan()
    g = seeded(pa, names, cols)
    g.usage_mark()
    UC.apply_steps(g, steps)
    rows1 = gpu_rows(g)
    plain = TP.entries(top1(g, 64))
    marked = top1(g, 64, mark=True)
    assert TP.entries(marked) == plain == UC.check(marked, rows, rows1, 64)
    again = top1(g, 64, mark=True)
    assert (again["n"], again["population"], again["names"]) == (0, 0, [])
    # more activity: only that shows
    five = sorted(names, key=len)[-5:]                     # long names: 231 bytes hold one of them
    assert min(map(len, five)) > 231 // 2
    g.take(five, [UC.TAKE_NOW + 5] * 5, [UC.FREQ] * 5, [UC.PER] * 5, [1, 2, 3, 4, 5])
    rows2 = gpu_rows(g)
    d = top1(g, 64)
    UC.check(d, rows1, rows2, 64)
    assert set(d["names"]) == set(five) and [int(x) for x in d["taken"]] == \
        [TP.f2b(float(c)) for c in (5, 4, 3, 2, 1)]
    # a truncated call still marks; so does one ranked by metric 0 (the whole table, whatever the prefix)
    cut = top1(g, 64, names_cap=231, mark=True)
    assert cut["truncated"] == 1 and 1 <= cut["n"] < 5
    assert top1(g, 64)["population"] == 0
    g.take(five, [UC.TAKE_NOW + 6] * 5, [UC.FREQ] * 5, [UC.PER] * 5, [1] * 5)
    rows3 = gpu_rows(g)
    assert top1(g, 64)["population"] == 5
    m0 = g.top(64, b"nobody-has-this", state=True, mark=True)
    assert m0["n"] == 0 and top1(g, 64)["population"] == 0
    TP.check(g.top(64, state=True, mark=True), rows3, 64)
    # the device form marks too
    g.take(five, [UC.TAKE_NOW + 7] * 5, [UC.FREQ] * 5, [UC.PER] * 5, [1] * 5)
    dv = device_top(g, 8, 231 * 8, mark=True)
    assert dv[0]["n"] == 5
    assert_untouched_past(*dv)
    assert top1(g, 64)["population"] == 0
    g.close()


# ------------------------------------------------ 8. a mark writes nothing else ----
def test_a_mark_writes_nothing_else(pa):
    names, cols, rows, steps = UC.plan()
    g = seeded(pa, names, cols, track_changes=True)
    UC.apply_steps(g, steps)
    whole = g.export_sweep(None, max_msgs=1024)[0]
    head, cur, st0 = g.export_sweep(None, max_msgs=8)
    assert len(head) == 8 and not st0["done"]
    before = (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity)
    assert before[2]["n"] > 0
    dump = gpu_rows(g)
    st = g.usage_mark()
    assert st["buckets"] == len(dump) == 650
    top1(g, 64, mark=True)
    device_top(g, 64, 231 * 64, mark=True)
    assert (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity) == before
    assert gpu_rows(g) == dump
    tail, _, st1 = g.export_sweep(cur, max_msgs=1024)        # the sweep cursor's layout still holds
    assert st1["restarted"] == 0 and st1["done"] == 1 and head + tail == whole
    g.close()


# ------------------------------------------------- 9. refusals touch nothing ----
def test_refusals_touch_nothing(pa):
    names, cols, rows, steps = UC.plan()
    lib = pa._lib
    K = 16
    bufs = dict(names=np.full(231 * K, FILL, np.uint8), offs=np.full(K + 1, FILL64, np.uint64),
                taken=np.full(K, FILL64, np.uint64), state=np.full((K, 4), FILL64, np.int64))

    def call(g, metric=0, flags=0, out=True):
        q, s = lib.phip_top_query(), lib.phip_top_stats(7, 7, 7, 7, 7)
        q.k, q.metric = K, metric
        o = lib.phip_top_out(bufs["names"].ctypes.data, 231 * K, bufs["offs"].ctypes.data,
                             bufs["taken"].ctypes.data, bufs["state"].ctypes.data)
        rc = g.L.phip_export_top(g.h, C.byref(q), C.byref(o) if out else None, C.byref(s), flags)
        assert (s.n, s.bytes, s.population, s.passes, s.truncated) == (7, 7, 7, 7, 7)
        for name, b in bufs.items():
            assert (b == (FILL if b.dtype == np.uint8 else FILL64)).all(), name
        return rc

    def mark(g, flags=0):
        s = lib.phip_usage_stats(7, 7)
        rc = g.L.phip_usage_mark(g.h, C.byref(s), flags)
        assert (s.buckets, s.active) == (7, 7)
        return rc

    plain = seeded(pa, names, cols, track_usage=False)
    assert mark(plain) == INVALID
    assert call(plain, metric=1) == INVALID
    assert call(plain, flags=lib.TOP_MARK) == INVALID
    assert call(plain, metric=1, flags=lib.TOP_MARK) == INVALID
    assert call(plain, metric=1, flags=lib.SWEEP_COUNT, out=False) == INVALID
    with pytest.raises(pa.PatrolHipError):
        plain.usage_mark()
    with pytest.raises(pa.PatrolHipError):
        plain.top(5, metric=1)
    TP.check(plain.top(64, state=True), rows, 64)           # and it serves metric 0 as before
    tracked = seeded(pa, names, cols)
    tracked.usage_mark()
    UC.apply_steps(tracked, steps)
    pop = tracked.top_count(metric=1)["population"]
    assert pop > 0
    for g in (plain, tracked):
        assert call(g, metric=2) == INVALID
        assert call(g, metric=0xFFFFFFFF) == INVALID
        assert mark(g, flags=1) == INVALID
        assert call(g, flags=lib.TOP_MARK | lib.SWEEP_COUNT, out=False) == INVALID
        assert call(g, metric=1, flags=lib.TOP_MARK | lib.SWEEP_COUNT, out=False) == INVALID
        assert call(g, flags=lib.TOP_MARK | 0x800) == INVALID
    assert tracked.top_count(metric=1)["population"] == pop    # no refused call marked
    plain.close()
    tracked.close()


# --------------------------------------------------------------- 10. group ----
def test_group(pa):
    import torch
    dev = torch.device("cuda", 0)
    world = 2
    g = pa.GPUGroup.open_all([0] * world, log2_slots=11, track_usage=True)
    names, cols, rows0 = TP.distinct_table(7, 600)
    batches = []
    for r in range(world):
        part = list(range(r, 600, world))
        nm = [names[i] for i in part]
        offs = np.zeros(len(nm) + 1, np.int32)
        offs[1:] = np.cumsum([len(x) for x in nm])
        blob = np.frombuffer(b"".join(nm) + b"\0" * 64, np.uint8).copy()
        batches.append(tuple(torch.from_numpy(x).to(dev) for x in (
            blob, offs, cols[0][part].view(np.int64).copy(), cols[1][part].view(np.int64).copy(),
            cols[2][part].copy())))
    torch.cuda.synchronize()
    _, merged = g.receive(batches, T0)
    assert sum(merged) == 600

    def union():
        rows = {}
        for r in g.repos:
            part = gpu_rows(r)
            assert not set(part) & set(rows)
            rows.update(part)
        return rows

    mark_rows = union()
    assert len(mark_rows) == 600 and all(len(gpu_rows(r)) >= 100 for r in g.repos)
    st = g.usage_mark()
    assert (st["buckets"], st["active"], len(st["members"])) == (600, 600, world)
    assert g.top(64, metric=1)["population"] == 0

    # routed takes: member r receives the ops on names r, r + 2, ... of the first 120, plus new names
    def ops(nm, cnt):
        n = len(nm)
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(x) for x in nm])
        blob = np.frombuffer(b"".join(nm) + b"\0" * 64, np.uint8).copy()
        col = dict(kind=np.zeros(n, np.uint8), names=blob, name_offs=offs,
                   now=np.full(n, UC.TAKE_NOW, np.int64), freq=np.full(n, UC.FREQ, np.int64),
                   per=np.full(n, UC.PER, np.int64), count=np.array(cnt, np.int64))
        return {key: torch.from_numpy(v).to(dev) for key, v in col.items()}

    taken_from = []
    obatches = []
    for r in range(world):
        nm = [names[i] for i in range(r, 120, world)] + [b"group-new-%d-%d" % (r, i) for i in range(10)]
        taken_from += nm
        obatches.append(ops(nm, [1 + (i % 7) for i in range(len(nm))]))
    torch.cuda.synchronize()
    res, sent, applied = g.apply_mixed(obatches)
    assert sum(applied) == len(taken_from) == 140
    assert all(int(x) & 0x7F == pa._lib.ST_TAKE_OK for r in res for x in r["status"].cpu().numpy())
    now_rows = union()
    assert len(now_rows) == 620
    ref = UC.reference(mark_rows, now_rows)
    assert set(ref) == set(taken_from)
    longest = None
    for k in (4096, 1, 50, 140):
        d = g.top(k, state=True, metric=1)
        got = UC.check(d, mark_rows, now_rows, k)
        longest = longest or got
        assert got == longest[:k] and len(d["members"]) == world
    d = g.top(4096, state=True, metric=1, mark=True)
    assert UC.check(d, mark_rows, now_rows, 4096) == longest
    d = g.top(4096, state=True, metric=1, mark=True)
    assert (d["n"], d["population"], d["names"]) == (0, 0, [])
    g.close()
