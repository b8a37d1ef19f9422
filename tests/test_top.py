"""phip_export_top on the GPU (include/patrolhip.h "Top talkers"), through the
binding.

What a call must report is tests/_top_cases.py's reference: the contract
restated in Python over the table's dump -- never the library.  The slot
tie-break does not show in a dump, so a result is checked by the prefix
property (top(k) is the head of top(k')) and by TP.check()'s set conditions.
"""
import ctypes as C
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import _top_cases as TP  # noqa: E402

T0, SEC = TP.T0, TP.SEC
FILL = 0x5A
FILL64 = 0x5A5A5A5A5A5A5A5A
INVALID = -1
MAX_PASSES = 8     # six 12-bit digits, the tie count, the collect (patrolhip.h "Stats")


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
    g = pa.GPURepo(**kw)
    g.seed(names, *cols)
    assert len(g) == len(names)
    return g


def device_top(g, k, cap, prefix=b"", now=0, idle_ns=0):
    """The PHIP_DEVICE_PTRS form over prefilled buffers -> (stats, names, offs,
    taken, state) as host arrays, whole."""
    import torch
    dev = torch.device("cuda", 0)
    names = torch.full((cap,), FILL, dtype=torch.uint8, device=dev)
    offs = torch.full((k + 1,), FILL64, dtype=torch.int64, device=dev)
    taken = torch.full((k,), FILL64, dtype=torch.int64, device=dev)
    state = torch.full((k, 4), FILL64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    st = g.top_device(k, names, offs, taken, state, prefix, now, idle_ns)
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


# ------------------------------------------------------------- 1. parity ----
@pytest.fixture(scope="module")
def small(pa):
    """600 buckets over the throttled recipe's name classes, distinct taken, in
    2^10 slots under 3-bit tags (forced collisions).  Shared, never changed."""
    names, cols, rows = TP.distinct_table(7, 600)
    assert sum(len(n) == 0 for n in names) == 1 and max(map(len, names)) >= 200
    assert len(set(int(t) for t in cols[1])) == 600
    g = seeded(pa, names, cols, debug_tag_bits=3)
    assert g.capacity == 1024 and gpu_rows(g) == rows
    yield g, rows
    g.close()


@pytest.mark.parametrize("k", [1, 7, 64, 600, 4096])
def test_parity(pa, small, k):
    g, rows = small
    host = g.top(k, state=True)
    got = TP.check(host, rows, k)
    # distinct keys: the list is the reference's, name by name
    ref = TP.reference(rows)
    assert [e[0] for e in got] == sorted(ref, key=lambda nm: -ref[nm])[:k]
    assert host["n"] == min(k, 600) and host["population"] == 600
    assert 1 <= host["passes"] <= MAX_PASSES
    # the device form: the same list, nothing written past it
    dv = device_top(g, k, 231 * min(k, 700))
    assert device_entries(*dv) == got
    assert {f: dv[0][f] for f in ("n", "bytes", "population", "truncated")} == \
        {f: host[f] for f in ("n", "bytes", "population", "truncated")}
    assert_untouched_past(*dv)
    # without the optional columns
    bare = g.top(k)
    assert bare["state"] is None and bare["names"] == host["names"]
    # the prefix property against the longest list
    assert TP.entries(g.top(4096, state=True))[:k] == got


# --------------------------------------------------- 2. digit boundaries ----
@pytest.mark.parametrize("s", TP.SHIFTS)
def test_digit_boundaries(pa, s):
    names, cols, rows = TP.boundary_table(s)
    g = seeded(pa, names, cols, hash_seed=5 + s)
    assert gpu_rows(g) == rows
    order = [b"inf"] + [b"fam-%d" % i for i in range(8, 0, -1)] + [b"denormal"]
    full = g.top(len(order), state=True)
    TP.check(full, rows, len(order))
    assert full["names"] == order and full["population"] == 10
    assert int(full["taken"][0]) == TP.INF and int(full["taken"][-1]) == 1
    for k in range(1, 11):            # every cut inside the family, and around it
        d = g.top(k, state=True)
        TP.check(d, rows, k)
        assert d["names"] == order[:k] and d["passes"] <= MAX_PASSES
    d = g.top(4096)
    assert d["names"] == order and d["n"] == 10
    g.close()


# --------------------------------------------------------------- 3. ties ----
def tie_table(n_above, n_tied, tied=7.0):
    names = [b"t%d" % i for i in range(n_above + n_tied)]
    n = len(names)
    t = np.array([TP.f2b(1000.0 + i) for i in range(n_above)] + [TP.f2b(tied)] * n_tied, np.uint64)
    cols = [np.full(n, TP.f2b(1e6), np.uint64), t, np.ones(n, np.int64), np.full(n, T0, np.int64)]
    rows = {nm: (TP.f2b(1e6), int(t[i]), 1, T0) for i, nm in enumerate(names)}
    return names, cols, rows


@pytest.mark.parametrize("n_above", [0, 300])
def test_ties(pa, n_above):
    """5000 buckets in 2^13 slots (two tiles).  All tied; then 300 distinct
    keys above 4700 tied ones, so that every cut past 300 falls inside a tie
    group that spans the tile boundary and is larger than the candidate cap."""
    names, cols, rows = tie_table(n_above, 5000 - n_above)
    g = seeded(pa, names, cols, log2_slots=13, hash_seed=3)
    assert g.capacity == 1 << 13
    longest = g.top(4096, state=True)
    head = TP.check(longest, rows, 4096)
    assert longest["passes"] == MAX_PASSES      # every digit, the tie count, the collect
    for k in [1, 10, 300, 301, 3000, 4096]:
        d = g.top(k, state=True)
        got = TP.check(d, rows, k)
        assert got == head[:k], k               # the prefix property
        assert d["passes"] <= MAX_PASSES and d["population"] == 5000
        assert TP.entries(g.top(k, state=True)) == got      # and the same list again
    # a cut among the distinct keys needs no tie pass
    if n_above:
        assert g.top(10)["passes"] < MAX_PASSES
        assert g.top(10)["names"] == [b"t%d" % i for i in range(299, 289, -1)]
    # the device form agrees at a cut inside the ties
    dv = device_top(g, 3000, 8 * 3000)
    assert device_entries(*dv) == head[:3000]
    assert_untouched_past(*dv)
    g.close()


# ------------------------------------------------------------ 4. filters ----
P16 = b"org:acme:0123456"
NOW = T0 + 1000 * SEC
IDLE = 100 * SEC
FILTERS = [(b"", 0, 0), (b"u", 0, 0), (P16, 0, 0), (b"", NOW, IDLE), (b"idle", NOW, IDLE),
           (b"idle", NOW, 0), (b"", NOW, 1), (b"nobody", 0, 0)]


def datagram(name, a, t, e):
    return struct.pack(">QQq", a, t, e) + bytes([len(name)]) + name


@pytest.fixture(scope="module")
def filtered(pa):
    names = [b"", b"u", b"u:alice", b"x", P16, P16 + b"tail", P16[:15], P16 + b"z" * 40,
             P16[:15] + b"_" + b"z" * 40, b"U:upper",
             b"idle-below", b"idle-at", b"idle-above", b"idle-ahead", b"idle-long-" + b"q" * 60]
    n = len(names)
    t = np.array([TP.f2b(10.0 + i) for i in range(n)], np.uint64)
    e = np.full(n, NOW - T0 - 10 * IDLE, np.int64)       # idle for 10 * IDLE at NOW
    for nm, idle in ((b"idle-below", IDLE - 1), (b"idle-at", IDLE), (b"idle-above", IDLE + 1),
                     (b"idle-ahead", -5 * SEC), (b"idle-long-" + b"q" * 60, 3)):
        e[names.index(nm)] = NOW - T0 - idle             # (ahead: created + elapsed > NOW)
    e[names.index(b"u:alice")] = NOW - T0 - 7            # one active bucket outside the idle names
    cols = [np.full(n, TP.f2b(1e6), np.uint64), t, e, np.full(n, T0, np.int64)]
    g = seeded(pa, names, cols, hash_seed=9)
    # a 240-byte name, which only a datagram brings in, with the largest taken
    giant = b"u" + b"G" * 239
    g.receive_datagrams([datagram(giant, TP.f2b(1e9), TP.f2b(1e8), 5)], NOW)
    rows = gpu_rows(g)
    assert giant in rows and rows[giant][1] == TP.f2b(1e8) and len(rows) == n + 1
    yield g, rows
    g.close()


@pytest.mark.parametrize("flt", FILTERS, ids=lambda f: "%s-%d" % (f[0].decode(), f[2]))
def test_filters(filtered, flt):
    g, rows = filtered
    prefix, now, idle_ns = flt
    ref = TP.reference(rows, prefix, now, idle_ns)
    for k in (1, 3, 4096):
        d = g.top(k, prefix, now, idle_ns, state=True)
        got = TP.check(d, rows, k, prefix, now, idle_ns)
        assert [e[0] for e in got] == sorted(ref, key=lambda nm: -ref[nm])[:k]
    # 8. count mode: the population of the full call, in one pass
    cnt = g.top_count(prefix, now, idle_ns)
    assert (cnt["population"], cnt["passes"], cnt["n"], cnt["bytes"]) == (len(ref), 1, 0, 0)


def test_filter_cases_hold_what_they_should(filtered):
    g, rows = filtered
    every = set(g.top(4096)["names"])
    assert len(every) == 15 and not any(len(nm) > 231 for nm in every)     # the 240-byte name never ranks
    assert set(g.top(4096, b"u")["names"]) == {b"u", b"u:alice"}             # not b"U:upper", not the giant
    # 16 bytes: the name itself, a tail, a long name; not the 15-byte head, not byte 16 differing
    assert set(g.top(4096, P16)["names"]) == {P16, P16 + b"tail", P16 + b"z" * 40}
    # idle == idle_ns - 1 stays, idle_ns and idle_ns + 1 go; an elapsed ahead of now is idle 0
    assert set(g.top(4096, b"idle", NOW, IDLE)["names"]) == \
        {b"idle-below", b"idle-ahead", b"idle-long-" + b"q" * 60}
    assert len(g.top(4096, b"idle", NOW, 0)["names"]) == 5                  # idle_ns = 0: no filter
    assert set(g.top(4096, b"", NOW, 1)["names"]) == {b"idle-ahead"}         # everything else idles >= 1 ns
    d = g.top(5, b"nobody")
    assert (d["n"], d["population"], d["names"], d["truncated"]) == (0, 0, [], 0)


# ------------------------------------------------------------- 5. bounds ----
def test_names_cap_cuts_at_an_entry(pa):
    rng = random.Random(4)
    names = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(200, 232))) for _ in range(100)]
    n = len(names)
    t = np.array([TP.f2b(1.0 + i) for i in range(n)], np.uint64)
    cols = [np.full(n, TP.f2b(1e6), np.uint64), t, np.ones(n, np.int64), np.full(n, T0, np.int64)]
    g = seeded(pa, names, cols, hash_seed=2)
    rows = gpu_rows(g)
    uncut = TP.check(g.top(64, state=True), rows, 64)
    for cap in (231, 500, 231 * 10, 231 * 64):
        d = g.top(64, names_cap=cap, state=True)
        got = TP.check(d, rows, 64, cut=cap < 231 * 64)
        # the longest prefix of the uncut list that fits
        fit, used = 0, 0
        while fit < 64 and used + len(uncut[fit][0]) <= cap:
            used += len(uncut[fit][0])
            fit += 1
        assert got == uncut[:fit] and d["bytes"] == used and fit >= 1
        assert d["truncated"] == int(fit < 64)
    assert g.top(64, names_cap=231)["truncated"] == 1
    # the device form under the cut: nothing past the cut list
    dv = device_top(g, 64, 500)
    assert device_entries(*dv) == uncut[:dv[0]["n"]] and dv[0]["truncated"] == 1
    assert_untouched_past(*dv)
    # k above the population
    d = g.top(4096)
    assert (d["n"], d["truncated"], d["population"]) == (100, 0, 100)
    g.close()


def test_empty_table_and_host_buffers(pa):
    g = pa.GPURepo(log2_slots=10, hash_seed=1)
    d = g.top(16, state=True)
    assert (d["n"], d["bytes"], d["population"], d["truncated"], d["names"]) == (0, 0, 0, 0, [])
    dv = device_top(g, 16, 231 * 16)
    assert dv[0]["n"] == 0
    assert_untouched_past(*dv)
    # host pointers, prefilled: a call copies back what was written, nothing more
    g.seed([b"a", b"bb", b"ccc"], *[np.array(c, dt) for c, dt in (
        ([TP.f2b(9.0)] * 3, np.uint64), ([TP.f2b(1.0), TP.f2b(3.0), TP.f2b(2.0)], np.uint64),
        ([1, 2, 3], np.int64), ([T0] * 3, np.int64))])
    lib = pa._lib
    K = 8
    names, offs = np.full(231 * K, FILL, np.uint8), np.full(K + 1, FILL64, np.uint64)
    taken, state = np.full(K, FILL64, np.uint64), np.full((K, 4), FILL64, np.int64)
    q, st = lib.phip_top_query(), lib.phip_top_stats()
    q.k = K
    out = lib.phip_top_out(names.ctypes.data, names.size, offs.ctypes.data, taken.ctypes.data,
                           state.ctypes.data)
    assert g.L.phip_export_top(g.h, C.byref(q), C.byref(out), C.byref(st), 0) == 0
    assert (st.n, st.bytes, st.population, st.truncated) == (3, 6, 3, 0)
    assert names[:6].tobytes() == b"bbccca" and list(offs[:4]) == [0, 2, 5, 6]
    assert [int(x) for x in taken[:3]] == [TP.f2b(3.0), TP.f2b(2.0), TP.f2b(1.0)]
    assert [int(x) for x in state[0]] == [TP.f2b(9.0), TP.f2b(3.0), 2, T0]
    assert (names[6:] == FILL).all() and (offs[4:] == FILL64).all()
    assert (taken[3:] == FILL64).all() and (state[3:] == FILL64).all()
    g.close()


def test_refusals_touch_nothing(pa, small):
    g, _ = small
    L, lib = g.L, pa._lib
    K = 16
    bufs = dict(names=np.full(231 * K, FILL, np.uint8), offs=np.full(K + 1, FILL64, np.uint64),
                taken=np.full(K, FILL64, np.uint64), state=np.full((K, 4), FILL64, np.int64))

    def out_struct(**kw):
        f = dict(names=bufs["names"].ctypes.data, names_cap=231 * K, offs=bufs["offs"].ctypes.data,
                 taken=bufs["taken"].ctypes.data, state=bufs["state"].ctypes.data)
        f.update(kw)
        return lib.phip_top_out(f["names"], f["names_cap"], f["offs"], f["taken"], f["state"])

    def call(k=K, prefix_len=0, metric=0, idle_ns=0, out="default", flags=0, q="default", st="default"):
        qq, s = lib.phip_top_query(), lib.phip_top_stats(7, 7, 7, 7, 7)
        qq.k, qq.prefix_len, qq.metric, qq.idle_ns = k, prefix_len, metric, idle_ns
        o = out_struct() if out == "default" else out
        rc = L.phip_export_top(g.h, C.byref(qq) if q == "default" else None,
                               C.byref(o) if o is not None else None,
                               C.byref(s) if st == "default" else None, flags)
        assert (s.n, s.bytes, s.population, s.passes, s.truncated) == (7, 7, 7, 7, 7)
        for name, b in bufs.items():
            assert (b == (FILL if b.dtype == np.uint8 else FILL64)).all(), name
        return rc

    assert call(k=0) == INVALID
    assert call(k=4097) == INVALID
    assert call(prefix_len=17) == INVALID
    assert call(metric=1) == INVALID
    assert call(idle_ns=-1) == INVALID
    assert call(q=None) == INVALID
    assert call(st=None) == INVALID
    assert call(flags=0x2) == INVALID
    assert call(flags=lib.SWEEP_COUNT | 0x40) == INVALID
    assert call(out=None) == INVALID                         # outside count mode
    assert call(out=out_struct(names=None)) == INVALID
    assert call(out=out_struct(offs=None)) == INVALID
    assert call(out=out_struct(names_cap=230)) == INVALID
    assert call(flags=lib.SWEEP_COUNT) == INVALID            # count mode takes no output
    assert call(k=0, out=None, flags=lib.SWEEP_COUNT) == INVALID
    with pytest.raises(pa.PatrolHipError):
        g.top(5, b"seventeen bytes!!")


# ----------------------------------------------------- 6. a larger table ----
def test_larger_table_with_repeats_and_growth(pa):
    n = 40000
    rng = np.random.default_rng(12)
    names = [b"b%d" % i for i in range(n)]
    tk = rng.integers(1, 2001, n).astype(np.float64)
    cols = [(tk + 5).view(np.uint64).copy(), tk.view(np.uint64).copy(),
            rng.integers(0, 1 << 40, n, dtype=np.int64), np.full(n, T0, np.int64)]
    g = seeded(pa, names, cols, log2_slots=16, hash_seed=21)
    assert g.capacity == 1 << 16
    rows = gpu_rows(g)
    assert len(set(r[1] for r in rows.values())) <= 2000
    d = g.top(4096, state=True)
    head = TP.check(d, rows, 4096)
    assert d["passes"] <= MAX_PASSES
    assert TP.check(g.top(500, state=True), rows, 500) == head[:500]
    pre = TP.check(g.top(4096, b"b1", state=True), rows, 4096, b"b1")
    assert len(pre) == 4096 and all(e[0].startswith(b"b1") for e in pre)
    # a batch that grows the table: a new layout, new slots, more buckets
    m = 25000
    more = [b"n%d" % i for i in range(m)]
    tm = rng.integers(1, 2001, m).astype(np.float64)
    g.receive_soa(more, (tm + 1).view(np.uint64).copy(), tm.view(np.uint64).copy(),
                  np.ones(m, np.int64), T0)
    assert g.capacity > 1 << 16
    rows2 = gpu_rows(g)
    assert len(rows2) == n + m
    d2 = g.top(4096, state=True)
    head2 = TP.check(d2, rows2, 4096)
    assert TP.check(g.top(77, state=True), rows2, 77) == head2[:77]
    g.close()


# ------------------------------------------- 7. read-only, queued batches ----
def test_nothing_is_written_to_the_handle(pa):
    names, cols, rows = TP.distinct_table(7, 600)
    g = seeded(pa, names, cols, debug_tag_bits=3, track_changes=True)
    tk = names[:40]
    g.apply_mixed(np.zeros(40, np.uint8), tk, np.full(40, T0, np.int64), np.full(40, 100, np.int64),
                  np.full(40, SEC, np.int64), np.ones(40, np.uint64),
                  *[np.zeros(40, t) for t in (np.uint64, np.uint64, np.int64)])
    whole = g.export_sweep(None, max_msgs=1024)[0]
    head, cur, st0 = g.export_sweep(None, max_msgs=8)
    assert len(head) == 8 and not st0["done"]
    before = (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity)
    assert before[2]["n"] > 0
    rows = gpu_rows(g)
    for k in (1, 64, 4096):
        TP.check(g.top(k, state=True), rows, k)
    TP.check(g.top(64, b"org:", T0, 5 * SEC, state=True), rows, 64, b"org:", T0, 5 * SEC)
    assert g.top_count()["population"] == len(TP.reference(rows))
    device_top(g, 64, 231 * 64)
    assert (g.snapshot().tobytes(), len(g), g.changes_count(), g.capacity) == before
    assert gpu_rows(g) == rows
    tail, _, st = g.export_sweep(cur, max_msgs=1024)        # the sweep cursor's layout still holds
    assert st["restarted"] == 0 and st["done"] == 1 and head + tail == whole
    g.close()


def test_sees_a_queued_batch(pa):
    """A PHIP_RECV_ASYNC batch is finished first: the list sees its merges."""
    import torch
    dev = torch.device("cuda", 0)
    names0, cols, rows0 = TP.distinct_table(7, 600)
    g = seeded(pa, names0, cols, log2_slots=18)
    hit = [nm for nm in names0 if nm][::5]
    n = 1 << 16
    names = [hit[(i // 3) % len(hit)] if i % 3 == 0 else b"filler-%d" % (i % 5000) for i in range(n)]
    a = np.zeros(n, np.float64)
    t = np.where(np.arange(n) % 3 == 0, 1e6, 1.0)
    e = np.ones(n, np.int64)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in names])
    blob = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()).to(dev)
    to = torch.from_numpy(offs).to(dev)
    ta, tt, te = (torch.from_numpy(x.view(np.int64).copy()).to(dev) for x in (a, t, e))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.receive_soa(blob, ta, tt, te, T0, name_offs=to, n=n, status=status, device=True, queue=True)
    d = g.top(len(hit), state=True)
    rows = gpu_rows(g)
    assert len(rows) == 600 + 5000
    TP.check(d, rows, len(hit))
    assert set(d["names"]) == set(hit) and set(int(x) for x in d["taken"]) == {TP.f2b(1e6)}
    g.close()


# -------------------------------------------------------------- 9. group ----
def test_group_top(pa):
    import torch
    dev = torch.device("cuda", 0)
    world = 3
    g = pa.GPUGroup.open_all([0] * world, log2_slots=11)
    rng = random.Random(17)
    names = TP.name_classes(rng, 900)
    vals = [rng.randrange(1, 400) for _ in names]          # repeats: ties across the members
    batches = []
    for r in range(world):
        part = list(range(r, 900, world))
        nm = [names[i] for i in part]
        t = np.array([float(vals[i]) for i in part])
        offs = np.zeros(len(nm) + 1, np.int32)
        offs[1:] = np.cumsum([len(x) for x in nm])
        blob = np.frombuffer(b"".join(nm) + b"\0" * 64, np.uint8).copy()
        batches.append(tuple(torch.from_numpy(x).to(dev) for x in (
            blob, offs, (t + 3).view(np.int64).copy(), t.view(np.int64).copy(),
            np.ones(len(nm), np.int64))))
    torch.cuda.synchronize()
    sent, merged = g.receive(batches, T0)
    assert sum(merged) == 900
    rows = {}
    for r in g.repos:
        part = gpu_rows(r)
        assert len(part) >= 200 and not set(part) & set(rows)      # owner-routed, disjoint
        rows.update(part)
    assert len(rows) == 900
    longest = None
    for k in (4096, 1, 50, 333):
        d = g.top(k, state=True)
        got = TP.check(d, rows, k)
        if longest is None:
            longest = got
        assert got == longest[:k]
        assert len(d["members"]) == world
    pre = g.top(4096, b"org:", state=True)
    TP.check(pre, rows, 4096, b"org:")
    assert pre["n"] >= 50
    g.close()
