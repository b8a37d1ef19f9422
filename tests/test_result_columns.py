"""Poisoned result columns on cuda:0 (tests/_columns.py): every call that
fills caller-provided per-op columns is handed columns full of a poison byte,
between guard bytes, aligned and misaligned, through the C ABI.  Each case
compares every entry of every passed column with the oracle bit for bit under
the header's contract (include/patrolhip.h, "Result columns": all n entries
written, zero where the column does not apply), checks the guards, the whole
table, that no device input changed, and that the kernel or pass it was
written for ran (set_timing / timings(), last_stats()).

tests/test_columns_cases.py shows on the CPU that the streams hold enough
default and enough non-default entries for a missing store to show.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import _columns as RC  # noqa: E402
from tests._gen import SEC, T0  # noqa: E402

DEVICE_PTRS = 0x1
RECV_ASYNC = 0x20
ERR_INVALID, ERR_SHORT = -1, -5
ALL = 15
# aligned as well: the full set, and the two a caller saving bandwidth would pick
LAYOUTS = [(m, True) for m in range(16)] + [(m, False) for m in (2, 9, 15)]
RECV_MASKS = [0, 1, 8, 9]      # the subsets of {status, reply}
# ... and all four (remaining / have read zero), and two aligned layouts
RECV_LAYOUTS = [(m, True) for m in RECV_MASKS + [ALL]] + [(9, False), (ALL, False)]


def layout_id(p):
    return "cols%d%s" % (p[0], "" if p[1] else "-aligned")


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


# ---------------------------------------------------------------- plumbing --
def gpu_dump(g):
    d = {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}
    assert len(g) == len(d)
    return d


def same_table(g, want):
    got = gpu_dump(g)
    assert len(got) == len(want)
    bad = [k for k in want if got.get(k) != want[k]]
    assert not bad, [(k, got.get(k), want[k]) for k in bad[:5]]


def kernels(g):
    return [nm for nm, _ in g.timings()]


class Inputs:
    """Input columns on the host (numpy) or the device (torch), kept alive
    for the call; unchanged(): every device tensor equals the clone taken
    when it was made."""

    def __init__(self, where):
        self.where, self.cols, self.clones = where, {}, {}

    def add(self, key, arr):
        if arr is None:
            self.cols[key] = None
            return None
        arr = np.ascontiguousarray(arr)
        if self.where == "device":
            import torch
            a = arr.view(np.int64) if arr.dtype == np.uint64 else \
                arr.view(np.int32) if arr.dtype == np.uint32 else arr
            t = torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
            self.cols[key], self.clones[key] = t, t.clone()
            return t.data_ptr()
        self.cols[key] = arr
        self.clones[key] = arr.copy()
        return arr.ctypes.data

    def unchanged(self):
        for key, c in self.clones.items():
            x = self.cols[key]
            same = bool((x == c).all())
            assert same, "input column %s was written" % key

    @property
    def flags(self):
        return DEVICE_PTRS if self.where == "device" else 0


def make_ops(args, where):
    """oracle-style apply_mixed arguments -> (phip_ops, Inputs)."""
    from patrol_amd import _lib
    from patrol_amd.engine import names_blob
    kind, names, now, freq, per, count, added, taken, elapsed = args
    blob, offs = names_blob(names)
    inp = Inputs(where)
    p = {k: inp.add(k, v) for k, v in (("kind", kind), ("names", blob), ("name_offs", offs),
                                       ("now", now), ("freq", freq), ("per", per),
                                       ("count", count), ("added", added), ("taken", taken),
                                       ("elapsed", elapsed))}
    ops = _lib.phip_ops(len(names), len(blob) if where == "device" else 0, p["kind"], p["names"],
                        p["name_offs"], p["now"], p["freq"], p["per"], p["count"], p["added"],
                        p["taken"], p["elapsed"])
    return ops, inp


def make_msgs(names, a, t, e, where, names_len=None):
    from patrol_amd import _lib
    from patrol_amd.engine import names_blob
    blob, offs = names_blob(names)
    inp = Inputs(where)
    p = [inp.add(k, v) for k, v in (("names", blob), ("name_offs", offs), ("added", a),
                                    ("taken", t), ("elapsed", e))]
    nl = (len(blob) if names_len is None else names_len) if where == "device" else 0
    return _lib.phip_msgs(len(names), nl, *p), inp


def stain(g, n):
    """A host call of n ops that leaves non-default values in every entry of
    every staged column of the handle (RC.stain_ops)."""
    out = g.apply_mixed(*RC.stain_ops(n))
    assert (out["status"] == RC.ST_TAKE_OK | RC.ST_CREATED).sum() == min(n, 2000)
    assert out["remaining"].all() and out["have"].all() and out["reply"]["a"].all()


# ------------------------------------------------------------- apply_mixed --
@functools.lru_cache(maxsize=None)
def stream(size):
    return {"small": RC.small_stream, "medium": RC.medium_stream, "large": RC.large_stream}[size]()


@functools.lru_cache(maxsize=None)
def mixed_reference(size, stained):
    """(expected columns, oracle table) of the stream applied to its seeded
    buckets, after the staining call where the host form makes one."""
    s = stream(size)
    o = O.Repo()
    s.seed_into(o)
    if stained:
        o.apply_mixed(*RC.stain_ops(s.n))
    want = RC.expected_mixed(s.kind, o.apply_mixed(*s.args))
    RC.assert_shares(RC.shares(s.kind, want), size)
    return want, o.dump()


def ran_for(size, where, launched):
    """The kernels each size and form was written for."""
    if size == "small" and where == "host":
        assert launched == ["k_small_mixed"], launched
        return
    need = ["k_fold_thread", "k_fold_wave"]
    huge = ["k_fold_block", "k_huge_outputs"]
    assert all(k in launched for k in need) and "k_small_mixed" not in launched, launched
    assert all((k in launched) == (size == "large") for k in huge), launched


def open_for(pa, size, where):
    s = stream(size)
    g = pa.GPURepo(log2_slots=13 if size == "small" else 15)
    s.seed_into(g)
    if where == "host":
        stain(g, s.n)   # at least as long as the call under test
    return s, g


def run_mixed(pa, size, where, mask, misaligned=True, null_res=False, egress=False):
    from patrol_amd import _lib
    s, g = open_for(pa, size, where)
    want, table = mixed_reference(size, where == "host")
    ops, inp = make_ops(s.args, where)
    res = RC.Results(s.n, mask, where, misaligned)
    pres = None if null_res else res.byref()
    g.set_timing(True)
    if not egress:
        rc = g.L.phip_apply_mixed(g.h, C.byref(ops), pres, inp.flags)
    else:
        nb = int(inp.cols["names"].numel() if where == "device" else inp.cols["name_offs"][-1])
        max_msgs, cap = g.egress_caps(s.n, nb, device=where == "device")
        out = RC.Column("status", cap, where, misaligned=False)        # cap poisoned bytes
        offs = RC.Column("remaining", max_msgs + 1, where, misaligned=False)
        eg = _lib.phip_egress(out.ptr, cap, offs.ptr, max_msgs, 0, 0, 0, 0)
        rc = g.L.phip_apply_mixed_egress(g.h, C.byref(ops), pres, C.byref(eg), inp.flags)
    assert rc == 0, (rc, g.L.phip_last_error(g.h))
    launched = kernels(g)
    got = res.check()
    assert set(got) == {c for c in RC.COLUMNS if mask & RC.BIT[c]}
    RC.compare(got, want)
    inp.unchanged()
    same_table(g, table)
    ran_for(size, where, launched)
    if egress:
        assert eg.n > 0 and eg.bytes > 0
        o = offs.check()
        out.check()
        assert int(o[0]) == 0 and int(o[eg.n]) == eg.bytes
        if not (size == "small" and where == "host"):
            assert "k_egress_write" in launched, launched
    g.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", ["small", "medium", "large"])
def test_apply_mixed(pa, size, where, layout):
    """All 16 column subsets (PHIP_OUT_DISPATCH) in both forms, the host form
    behind a staining call on the same handle: under kSmallMax (from host
    arrays k_small_mixed, its thread and its wave fold), just over it (the
    ordered path's thread and wave folds with no huge bucket beside them) and
    at 36k ops with a bucket over kHugeSeg (k_fold_block, k_huge_outputs)."""
    run_mixed(pa, size, where, *layout)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", ["small", "large"])
def test_apply_mixed_without_results(pa, size, where):
    """res == NULL (subset 0 with four NULLs is cols0 above): the table alone."""
    run_mixed(pa, size, where, 0, null_res=True)


@pytest.mark.parametrize("mask", [0, 1, 14, 15])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("size", ["small", "large"])
def test_apply_mixed_egress(pa, size, where, mask):
    """The same batches with their egress: without a status column the
    library keeps one of its own, which must not leak into the caller's."""
    run_mixed(pa, size, where, mask, egress=True)


# -------------------------------------------------------------------- take --
@pytest.mark.parametrize("n,misaligned", [(1, True), (65, True), (65, False), (5000, True),
                                          (5000, False)])
def test_take(pa, n, misaligned):
    """phip_take (host arrays only: it refuses device pointers) with poisoned
    remaining_out / ok_out at one op, one past a wave and a large-path batch,
    behind a staining call.  Rate 5/s on 40 buckets: most takes are denied."""
    from patrol_amd.engine import names_blob
    rng = np.random.default_rng(4300 + n)
    names = [b"tk%d" % i for i in rng.integers(0, 40, n)]
    now = T0 + np.arange(n, dtype=np.int64) * 1000
    freq, per = np.full(n, RC.FREQ, np.int64), np.full(n, SEC, np.int64)
    count = rng.choice(np.array([1, 1, 2, 5], np.uint64), n)
    g, o = pa.GPURepo(log2_slots=13), O.Repo()
    stain(g, n)
    o.apply_mixed(*RC.stain_ops(n))
    z64, zi = np.zeros(n, np.uint64), np.zeros(n, np.int64)
    ref = o.apply_mixed(np.zeros(n, np.uint8), names, now, freq, per, count, z64, z64, zi)
    if n > 1000:
        assert (ref["remaining"] == 0).sum() >= 64 and (ref["remaining"] != 0).sum() >= 64
    blob, offs = names_blob(names)
    rem = RC.Column("remaining", n, "host", misaligned)
    ok = RC.Column("status", n, "host", misaligned)
    g.set_timing(True)
    rc = g.L.phip_take(g.h, blob.ctypes.data, offs.ctypes.data, n, now.ctypes.data,
                       freq.ctypes.data, per.ctypes.data, count.ctypes.data, rem.ptr, ok.ptr, 0)
    assert rc == 0, g.L.phip_last_error(g.h)
    launched = kernels(g)
    RC.compare(dict(remaining=rem.check(), status=ok.check()),
               dict(remaining=ref["remaining"],
                    status=((ref["status"] & 0x7F) == RC.ST_TAKE_OK).astype(np.uint8)))
    assert ("k_small_mixed" in launched) == (n <= RC.SMALL_MAX), launched
    assert ("k_fold_wave" in launched) == (n > RC.SMALL_MAX), launched
    same_table(g, o.dump())
    g.close()


# ------------------------------------------------------------------ upsert --
@pytest.mark.parametrize("layout", RECV_LAYOUTS, ids=layout_id)
@pytest.mark.parametrize("where,n", [("host", 700), ("host", 5000), ("device", 5000)])
def test_upsert_soa(pa, where, n, layout):
    """phip_upsert_soa on the small and the large path: the subsets of
    {status, reply}, and all four columns (remaining / have read zero).
    Half the buckets exist: MERGED (the default) and UPSERT_INSERTED both show."""
    rng = np.random.default_rng(4400 + n)
    K = 300
    ids = rng.integers(0, K, n)
    names = [b"up%d" % i for i in ids]
    a = rng.integers(1, 50, n).astype(np.float64).view(np.uint64)
    t = rng.integers(1, 50, n).astype(np.float64).view(np.uint64)
    e = rng.integers(1, SEC, n)
    now = T0 + 77
    g, o = pa.GPURepo(log2_slots=13), O.Repo()
    if where == "host":
        stain(g, n)
        o.apply_mixed(*RC.stain_ops(n))
    kind = np.full(n, RC.UPSERT, np.uint8)
    zi = np.zeros(n, np.int64)
    ref = o.apply_mixed(kind, names, np.full(n, now, np.int64), zi, zi, zi.astype(np.uint64), a, t, e)
    want = RC.expected_mixed(kind, ref)
    d = RC.is_default("status", want["status"])
    assert d.sum() >= 64 and (~d).sum() >= 64
    assert not want["remaining"].any() and not RC.is_default("reply", want["reply"]).any()
    m, inp = make_msgs(names, a, t, e, where)
    res = RC.Results(n, layout[0], where, layout[1])
    g.set_timing(True)
    rc = g.L.phip_upsert_soa(g.h, C.byref(m), now, res.byref(), inp.flags)
    assert rc == 0, g.L.phip_last_error(g.h)
    launched = kernels(g)
    RC.compare(res.check(), want)
    inp.unchanged()
    if where == "host" and n <= RC.SMALL_MAX:
        assert launched == ["k_small_mixed"], launched
    else:
        assert "k_fold_thread" in launched and "k_small_mixed" not in launched, launched
    same_table(g, o.dump())
    g.close()


# ------------------------------------------------------------------- group --
@functools.lru_cache(maxsize=None)
def group_stream():
    """About 5000 ops: two wave-fold buckets, thin ones, half of them new."""
    rng = np.random.default_rng(4500)
    sizes = [600, 100, 40] + [3] * 800 + [2] * 700 + [1] * 460
    s = RC.Stream(rng, sizes, [1, 0, 1] + [i % 2 for i in range(1960)], prefix=b"g")
    o = O.Repo()
    s.seed_into(o)
    want = RC.expected_mixed(s.kind, o.apply_mixed(*s.args))
    RC.assert_shares(RC.shares(s.kind, want), "group stream")
    return s, want, o.dump()


GROUP_COLS = {"all": (ALL, True), "no_reply": (7, True), "status": (1, True),
              "all-aligned": (ALL, False)}
GROUP_CHUNK = 4096     # PHIP_GROUP_SMALL_CHUNKS: ops of a member's batch per round


@pytest.mark.parametrize("cols", list(GROUP_COLS))
@pytest.mark.parametrize("shape", ["world1_self", "world1_self_small_chunks", "two_shards"])
def test_group_apply_mixed(pa, shape, cols):
    """phip_group_apply_mixed into the caller's poisoned tensors (results=):
    a world of one through the RCCL exchange to itself, once in rounds of 4096
    ops, and two shards on one GPU, member 0 holding the stream's first 3000
    ops and member 1 the rest (the order rule then is the stream's order).
    The results come back over the exchange and k_route_results_scatter, one
    round at a time: every round is one pack on the source (k_route_ops_scatter)
    and one ordered apply on the owner (k_fold_thread), which the members' own
    kernel timings count."""
    import torch
    from tests import _group_ops as GO
    s, want, table = group_stream()
    world = 2 if shape == "two_shards" else 1
    cuts = [0, 3000, s.n] if world == 2 else [0, s.n]
    g = pa.GPUGroup.open_all([0] * world, log2_slots=13)
    for r in g.repos:
        s.seed_into(r)   # (a bucket is found on its owner alone; the others' copies are dropped below)
    batches, inputs, results = [], [], []
    for i in range(world):
        lo, hi = cuts[i], cuts[i + 1]
        args = tuple(a[lo:hi] for a in s.args)
        _, inp = make_ops(args, "device")
        inputs.append(inp)
        batches.append({k: inp.cols[k] for k in pa.GPUGroup._OPS_KEYS})
        results.append(RC.Results(hi - lo, GROUP_COLS[cols][0], "device", GROUP_COLS[cols][1]))
    g.set_timing(True)
    for r in g.repos:
        r.set_timing(True, accumulate=True)
    out, sent, applied = g.apply_mixed(
        batches, rccl_self=world == 1, small_chunks=shape.endswith("small_chunks"),
        results=[{c: col.tensor() for c, col in r.cols.items()} for r in results])
    torch.cuda.synchronize()
    assert sent == [cuts[i + 1] - cuts[i] for i in range(world)] and sum(applied) == s.n
    assert all(x > 0 for x in applied)
    for i in range(world):
        lo, hi = cuts[i], cuts[i + 1]
        got = results[i].check()
        assert set(got) == set(results[i].cols) and set(out[i]) == set(RC.COLUMNS)
        RC.compare(got, {c: want[c][lo:hi] for c in RC.COLUMNS})
        inputs[i].unchanged()
        ms = g.stage_ms(i)
        assert ms["pack"] > 0 and ms["merge"] > 0, ms     # routed, not handed straight on
    # the rounds: the longest batch in chunks of 4096 with small_chunks, else one
    chunked = shape.endswith("small_chunks")
    rounds = -(-max(np.diff(cuts)) // GROUP_CHUNK) if chunked else 1
    assert rounds == (2 if chunked else 1)
    for i, r in enumerate(g.repos):
        ran = kernels(r)
        assert ran.count("k_route_ops_scatter") == rounds, (i, ran)
        assert ran.count("k_fold_thread") == rounds, (i, ran)
    # the tables together: each bucket's copy on its owner is the oracle's
    # (the seeds were given to every member; only an owner's copy is ever named)
    _owners = GO.owners
    got = {}
    for r, repo in enumerate(g.repos):
        d = gpu_dump(repo)
        keys = list(d)
        own = _owners(keys, world)
        got.update({k: d[k] for k, w in zip(keys, own) if w == r})
    g.close()
    assert len(got) == len(table)
    bad = [k for k in table if got.get(k) != table[k]]
    assert not bad, [(k, got.get(k), table[k]) for k in bad[:5]]


# ----------------------------------------------------------------- receive --
K = 4000                       # seeded buckets b0 .. b3999
NHOT = (1 << 16) + 65          # the smallest batch with a hot directory, a tail chunk of one
DIRTY_CAP = 4096               # kDirtyCap: more dirty messages take the prefix rule


def key_names(ids):
    return [b"b%d" % int(i) for i in ids]


def seeded_pair(pa, rng, **kw):
    from tests._gen import clean_states
    names = key_names(np.arange(K))
    a, t, e = clean_states(rng, K)
    created = T0 - rng.integers(1, SEC, K)
    g, o = pa.GPURepo(log2_slots=17, **kw), O.Repo()
    for r in (g, o):
        r.seed(names, a, t, e, created)
    return g, o


class Msgs:
    """A Receive batch: clean states later than every state of the steps
    before (each batch raises the buckets it names), then made dirty."""

    def __init__(self, rng, ids, step):
        n = len(ids)
        self.n, self.names, self.now = n, key_names(ids), T0 + step * SEC
        taken = rng.integers(0, 10**6, n).astype(np.float64) + step * 2e6
        self.a = (taken + rng.random(n) * 100.0).view(np.uint64).copy()
        self.t = taken.view(np.uint64).copy()
        self.e = rng.integers(0, 1 << 40, n, dtype=np.int64) + step * (1 << 40)

    def incast(self, idx):
        self.a[idx], self.t[idx], self.e[idx] = 0, 0, 0
        return self

    def neg_zero(self, idx):
        self.a[idx] = RC.NEG_ZERO
        return self

    def wire(self, short_at=None):
        """-> (datagram bytes with 8 bytes of slack, offsets); the datagram at
        short_at cut below its fixed 25 bytes."""
        import struct
        ds = [struct.pack(">QQqB", int(a), int(t), int(e), len(nm)) + nm
              for a, t, e, nm in zip(self.a, self.t, self.e, self.names)]
        if short_at is not None:
            ds[short_at] = ds[short_at][:20]
        offs = np.zeros(self.n + 1, np.uint64)
        offs[1:] = np.cumsum([len(d) for d in ds])
        return np.frombuffer(b"".join(ds) + b"\0" * 8, np.uint8).copy(), offs


def zipf(rng, n):
    from tests._gen import zipf_ids
    return zipf_ids(rng, n, K)


def recv(g, form, where, b, res, flags=0, stop_at=None, rq=None):
    """One Receive call through the C ABI -> (rc, stop index or None, Inputs).
    form "soa": phip_receive_soa[_replies] (stop_at: a malformed checked
    offset entry there); "wire": phip_receive_datagrams[_replies] (stop_at: a
    short datagram there)."""
    from patrol_amd import _lib
    from patrol_amd.engine import names_blob
    fl = flags | (DEVICE_PTRS if where == "device" else 0)
    pres = res.byref() if res is not None else None
    inp = Inputs(where)
    if form == "soa":
        blob, offs = names_blob(b.names)
        if stop_at is not None:
            assert where == "device" and offs[stop_at] > 0
            offs[stop_at + 1] = offs[stop_at] - 1
        p = [inp.add(k, v) for k, v in (("names", blob), ("name_offs", offs), ("added", b.a),
                                        ("taken", b.t), ("elapsed", b.e))]
        m = _lib.phip_msgs(b.n, len(blob) if where == "device" else 0, *p)
        if rq is None:
            return g.L.phip_receive_soa(g.h, C.byref(m), b.now, pres, fl), None, inp
        return g.L.phip_receive_soa_replies(g.h, C.byref(m), b.now, pres, C.byref(rq), fl), None, inp
    data, offs = b.wire(stop_at)
    pd, po = inp.add("bytes", data), inp.add("offs", offs)
    assert pd % 8 == 0
    stop = C.c_uint32(0xABABABAB)
    if rq is None:
        rc = g.L.phip_receive_datagrams(g.h, pd, po, b.n, b.now, pres, C.byref(stop), fl)
    else:
        rc = g.L.phip_receive_datagrams_replies(g.h, pd, po, b.n, b.now, pres, C.byref(stop),
                                                C.byref(rq), fl)
    return rc, stop.value, inp


def expect(o, b, stop=None):
    return RC.expected_receive(o, b.names, b.a, b.t, b.e, b.now, stop)


def settle(res, want, inp, mask):
    got = res.check()
    assert set(got) == {c for c in RC.COLUMNS if mask & RC.BIT[c]}
    RC.compare(got, want)
    inp.unchanged()


def dirty_few(rng, b, new_ids=()):
    """A few incasts (on hot, cold and batch-created buckets) and -0.0 fields."""
    idx = rng.choice(b.n, 14, replace=False)
    b.incast(idx[:9]).neg_zero(idx[9:])
    for j, i in enumerate(new_ids):
        b.names[int(idx[j])] = b"b%d" % i
    return b


@pytest.mark.parametrize("mask", RECV_MASKS + [ALL])
@pytest.mark.parametrize("form", ["soa", "wire"])
def test_receive_clean_batches_build_and_keep_the_directory(pa, form, mask):
    """Four clean batches naming the same ids: the first passes build the hot
    directory (k_hot_dir, which also fills the status column), the decoded
    form's later ones take the kept one (last_stats()[7] >= 1) and fill the
    column from the fast kernel; the wire form builds one for every batch.
    Every entry is a default here (MERGED, a zero reply, zero remaining / have
    in the full set): only the poison tells a store from none."""
    rng = np.random.default_rng(4600)
    g, o = seeded_pair(pa, rng)
    ids = zipf(rng, NHOT)
    g.set_timing(True, accumulate=True)
    ages = []
    for step in (1, 2, 3, 4):
        b = Msgs(rng, ids, step)
        res = RC.Results(b.n, mask, "device")
        rc, stop, inp = recv(g, form, "device", b, res)
        assert rc == 0 and stop in (None, b.n), (rc, stop, g.L.phip_last_error(g.h))
        want = expect(o, b)
        assert (want["status"] == RC.ST_MERGED).all()
        settle(res, want, inp, mask)
        stats = g.last_stats()
        assert stats[0] > 0 and stats[1] > 0, stats     # a directory, messages folded through it
        ages.append(stats[7])
    ran = kernels(g)
    assert ran.count("k_receive_fast") == 4, ran
    if form == "soa":
        assert ages[-1] >= 1 and ran.count("k_hot_dir") < 4, (ages, ran)
    else:
        assert ran.count("k_hot_dir") == 4, ran
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("layout", RECV_LAYOUTS, ids=layout_id)
@pytest.mark.parametrize("n", [1, 63, 65, 5000])
@pytest.mark.parametrize("form,where", [("soa", "host"), ("wire", "host"), ("soa", "device"),
                                        ("wire", "device")])
def test_receive_small_batches(pa, form, where, n, layout):
    """1, 63 and 65 messages (from host arrays: one launch of k_small_mixed)
    and 5000 (the staged large path), with incasts, -0.0 fields and buckets
    the batch creates; the host form behind a staining call.  With all four
    columns remaining and have read zero, not the stain."""
    rng = np.random.default_rng(4700 + n)
    g, o = seeded_pair(pa, rng)
    if where == "host":
        stain(g, n)
        o.apply_mixed(*RC.stain_ops(n))
    ids = rng.integers(0, 200, n)
    ids[rng.random(n) < 0.2] += K                      # new buckets
    b = Msgs(rng, ids, 1)
    if n > 1:
        dirty = rng.choice(n, max(2, n // 8), replace=False)
        b.incast(dirty[::2]).neg_zero(dirty[1::2])
    else:
        b.incast(np.array([0]))
    mask = layout[0]
    res = RC.Results(n, mask, where, layout[1])
    g.set_timing(True)
    rc, stop, inp = recv(g, form, where, b, res)
    assert rc == 0 and stop in (None, n), (rc, stop, g.L.phip_last_error(g.h))
    ran = kernels(g)
    want = expect(o, b)
    if n >= 63:
        for c in ("status", "reply"):
            d = RC.is_default(c, want[c])
            assert d.sum() >= 3 and (~d).sum() >= 3, c
    settle(res, want, inp, mask)
    if where == "host" and n <= RC.SMALL_MAX:
        assert ran == ["k_small_mixed"], ran
    else:
        assert "k_small_mixed" not in ran and "k_fold_thread" in ran, ran
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS)
@pytest.mark.parametrize("form", ["soa", "wire"])
def test_receive_batch_that_creates_buckets(pa, form, mask):
    """3000 of the batch's messages name buckets it creates: the fast pass
    lists them as misses and k_receive_list / k_mark_created rewrite their
    statuses over the fill."""
    rng = np.random.default_rng(4800)
    g, o = seeded_pair(pa, rng)
    ids = zipf(rng, NHOT)
    ids[rng.choice(NHOT, 3000, replace=False)] = K + rng.integers(0, 1000, 3000)
    b = Msgs(rng, ids, 1)
    res = RC.Results(b.n, mask, "device")
    g.set_timing(True)
    rc, stop, inp = recv(g, form, "device", b, res)
    assert rc == 0 and stop in (None, b.n), (rc, stop, g.L.phip_last_error(g.h))
    ran = kernels(g)
    want = expect(o, b)
    created = (want["status"] & RC.ST_CREATED) != 0
    assert 64 <= created.sum() <= 1000
    settle(res, want, inp, mask)
    assert g.last_stats()[2] >= 3000 and "k_receive_list" in ran and "k_mark_created" in ran, ran
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS)
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("form", ["soa", "wire"])
def test_receive_dirty_sub_batch(pa, form, where, mask):
    """A few incasts and -0.0 fields on a handle that sets dirty buckets
    apart: their messages go through the ordered path as a sub-batch and
    k_defer_scatter puts statuses and replies back (last_stats()[4]: the
    sub-batch's entries, far fewer than the batch)."""
    rng = np.random.default_rng(4900)
    g, o = seeded_pair(pa, rng, isolate=True)
    if where == "host":
        stain(g, NHOT)
        o.apply_mixed(*RC.stain_ops(NHOT))
    b = dirty_few(rng, Msgs(rng, zipf(rng, NHOT), 1), new_ids=(K + 1, K + 2))
    res = RC.Results(b.n, mask, where)
    g.set_timing(True)
    rc, stop, inp = recv(g, form, where, b, res)
    assert rc == 0 and stop in (None, b.n), (rc, stop, g.L.phip_last_error(g.h))
    ran = kernels(g)
    want = expect(o, b)
    assert ((want["status"] & 0x7F) == RC.ST_INCAST_REPLY).sum() >= 5
    settle(res, want, inp, mask)
    ordered = g.last_stats()[4]
    assert 14 <= ordered <= 5 * DIRTY_CAP and "k_dirty_pass" in ran and "k_fold_thread" in ran, \
        (ordered, ran)
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS)
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("form", ["soa", "wire"])
def test_receive_prefix_rule_seam(pa, form, where, mask):
    """More than kDirtyCap dirty messages, the first at the batch's middle:
    the fast pass merges the prefix, the ordered path applies everything from
    the first dirty message on and writes the tail of the columns
    (last_stats()[4] == n - first dirty)."""
    rng = np.random.default_rng(5000)
    g, o = seeded_pair(pa, rng, isolate=True)
    if where == "host":
        stain(g, NHOT)
        o.apply_mixed(*RC.stain_ops(NHOT))
    b = Msgs(rng, zipf(rng, NHOT), 1)
    first = NHOT // 2 + 1
    b.incast(np.arange(first, NHOT, 6))
    assert len(range(first, NHOT, 6)) > DIRTY_CAP
    res = RC.Results(b.n, mask, where)
    g.set_timing(True)
    rc, stop, inp = recv(g, form, where, b, res)
    assert rc == 0 and stop in (None, b.n), (rc, stop, g.L.phip_last_error(g.h))
    ran = kernels(g)
    want = expect(o, b)
    settle(res, want, inp, mask)
    assert g.last_stats()[4] == NHOT - first and "k_fold_wave" in ran, (g.last_stats(), ran)
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS + [ALL])
@pytest.mark.parametrize("n", [700, NHOT])
@pytest.mark.parametrize("form,where", [("wire", "host"), ("wire", "device"), ("soa", "device")])
def test_receive_batch_that_stops(pa, form, where, n, mask):
    """A short datagram on the wire (PHIP_ERR_SHORT_BUFFER) and a malformed
    checked offset on the decoded form (PHIP_ERR_INVALID), a third into the
    batch: the messages before it as usual, SHORT, NOT_PROCESSED after it,
    zero in every other column from the stop on (fill_stopped; from host
    arrays of at most kSmallMax datagrams, the small path's own fill).  The
    path: the stop index and the error text name message k; 700 host
    datagrams are one k_small_mixed launch; every other case classifies, runs
    the fast pass and sends 0 < last_stats()[4] <= k - 5 messages through the
    ordered path (the incast at message 5 up to the stop, none past it)."""
    rng = np.random.default_rng(5100 + n)
    g, o = seeded_pair(pa, rng)
    if where == "host":
        stain(g, n)
        o.apply_mixed(*RC.stain_ops(n))
    b = Msgs(rng, zipf(rng, n), 1)
    k = n // 3
    b.incast(np.array([5, k + 7]))
    res = RC.Results(n, mask, where)
    g.set_timing(True)
    rc, stop, inp = recv(g, form, where, b, res, stop_at=k)
    err = g.L.phip_last_error(g.h).decode()
    ran = kernels(g)
    assert rc == (ERR_SHORT if form == "wire" else ERR_INVALID), (rc, err)
    # where the library itself says the batch stopped
    if form == "wire":
        assert stop == k and ("datagram %d" % k) in err, (stop, err)
    else:
        assert ("message %d " % k) in err, err
    if where == "host" and n <= RC.SMALL_MAX:
        # the one launch over the prefix; small_datagrams fills the rest on the host
        assert ran == ["k_small_mixed"], ran
    else:
        # the classification finds the stop, the fast pass merges the clean
        # prefix, the incast at message 5 sends what lies between it and the
        # stop, and nothing past it, through the ordered path
        assert any(x.startswith("k_classify") for x in ran) and "k_receive_fast" in ran, ran
        assert "k_fold_thread" in ran and "k_small_mixed" not in ran, ran
        ordered = g.last_stats()[4]
        assert 0 < ordered <= k - 5, (ordered, k, ran)
    want = expect(o, b, stop=k)
    assert want["status"][k] == RC.ST_SHORT and (want["status"][k + 1:] == RC.ST_NOT_PROCESSED).all()
    settle(res, want, inp, mask)
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS)
@pytest.mark.parametrize("finish", ["flush", "next_call"])
@pytest.mark.parametrize("what", ["clean", "dirty", "stops"])
def test_receive_queued(pa, what, finish, mask):
    """PHIP_RECV_ASYNC: the batch's columns are final when flush(), or the
    handle's next call, has finished it; a stopping batch reports its error
    from there."""
    rng = np.random.default_rng(5200)
    g, o = seeded_pair(pa, rng, isolate=what == "dirty")
    b = Msgs(rng, zipf(rng, NHOT), 1)
    k = None
    if what == "dirty":
        dirty_few(rng, b)
    elif what == "stops":
        k = NHOT // 3
    res = RC.Results(b.n, mask, "device")
    g.set_timing(True, accumulate=True)
    rc, _, inp = recv(g, "soa", "device", b, res, flags=RECV_ASYNC, stop_at=k)
    assert rc == 0, g.L.phip_last_error(g.h)
    want = expect(o, b, stop=k)
    follow = None
    if finish == "flush":
        rc = g.L.phip_flush(g.h)
    else:
        b2 = Msgs(rng, zipf(rng, 3000), 2)
        res2 = RC.Results(b2.n, mask, "device")
        rc, _, inp2 = recv(g, "soa", "device", b2, res2)
        follow = (b2, res2, inp2)
    assert rc == (ERR_INVALID if what == "stops" else 0), (rc, g.L.phip_last_error(g.h))
    ran = kernels(g)
    settle(res, want, inp, mask)
    assert "k_receive_fast" in ran, ran
    if what == "dirty":     # (last_stats() speaks of the handle's last batch: the queued one after flush())
        assert "k_dirty_pass" in ran and "k_fold_thread" in ran, ran
        assert finish != "flush" or 14 <= g.last_stats()[4] <= 5 * DIRTY_CAP, g.last_stats()
    if follow and what != "stops":     # (the failed call applied nothing of its own)
        b2, res2, inp2 = follow
        settle(res2, expect(o, b2), inp2, mask)
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", [0, 1])
@pytest.mark.parametrize("form", ["soa", "wire"])
def test_receive_replies_columns(pa, form, mask):
    """The _replies forms with no column and with status only, their egress
    buffers poisoned too (tests/test_replies.py checks the egress itself):
    the datagrams end where offs says, nothing past them or past the caps is
    written, and the status column beside them is the plain call's."""
    from patrol_amd import _lib
    rng = np.random.default_rng(5300)
    g, o = seeded_pair(pa, rng, isolate=True)
    b = dirty_few(rng, Msgs(rng, zipf(rng, NHOT), 1))
    want = expect(o, b)
    nrep = int(((want["status"] & 0x7F) == RC.ST_INCAST_REPLY).sum())
    assert nrep >= 5
    max_msgs, cap = 64, 64 * 256
    out = RC.Column("status", cap, "device", misaligned=False)
    offs = RC.Column("remaining", max_msgs + 1, "device", misaligned=False)
    src = RC.Column("status", 4 * max_msgs, "device", misaligned=False)
    rq = _lib.phip_reply_egress(out.ptr, cap, offs.ptr, src.ptr, max_msgs, 7, 7, 7, 7)
    res = RC.Results(b.n, mask, "device")
    g.set_timing(True)
    rc, stop, inp = recv(g, form, "device", b, res, rq=rq)
    assert rc == 0 and stop in (None, b.n), (rc, stop, g.L.phip_last_error(g.h))
    ran = kernels(g)
    settle(res, want, inp, mask)
    assert (rq.n, rq.replies, rq.skipped) == (nrep, nrep, 0)
    eo = offs.check()
    assert int(eo[0]) == 0 and int(eo[rq.n]) == rq.bytes and (np.diff(eo[:rq.n + 1].astype(np.int64)) > 25).all()
    assert (eo[rq.n + 1:] == np.frombuffer(bytes([RC.POISON]) * 8, np.uint64)[0]).all()
    # past the last datagram's 8-byte word the buffer is untouched
    assert (out.check()[(rq.bytes + 7) // 8 * 8:] == RC.POISON).all()
    ids = src.check().view(np.uint32)
    assert (np.sort(ids[:rq.n]) == np.nonzero((want["status"] & 0x7F) == RC.ST_INCAST_REPLY)[0]).all()
    assert (src.check()[4 * rq.n:] == RC.POISON).all()
    assert any(k.startswith("k_reply") for k in ran), ran
    same_table(g, o.dump())
    g.close()


@pytest.mark.parametrize("mask", RECV_MASKS + [ALL])
@pytest.mark.parametrize("n", [65, 3000])
def test_ring_receive(pa, n, mask):
    """One ring slot through phip_ring_receive into poisoned host columns: a
    small slot merged from its pinned bytes in one launch, a larger one from
    its device copy."""
    rng = np.random.default_rng(5400 + n)
    g, o = seeded_pair(pa, rng)
    stain(g, n)
    o.apply_mixed(*RC.stain_ops(n))
    ids = rng.integers(0, 200, n)
    ids[rng.random(n) < 0.2] += K
    b = Msgs(rng, ids, 1)
    dirty = rng.choice(n, n // 8, replace=False)
    b.incast(dirty[::2]).neg_zero(dirty[1::2])
    data, offs = b.wire()
    ring = pa.Ring(g, nslots=2, max_msgs=4096)
    try:
        slot, bv, ov = ring.acquire()
        ov[:n + 1] = offs
        bv[:len(data)] = data
        ring.submit(slot, n)
        res = RC.Results(n, mask, "host")
        stop = C.c_uint32(0xABABABAB)
        g.set_timing(True)
        rc = g.L.phip_ring_receive(ring.r, slot, b.now, res.byref(), C.byref(stop))
        assert rc == 0 and stop.value == n, (rc, stop.value, g.L.phip_last_error(g.h))
        ran = kernels(g)
        got = res.check()
        RC.compare(got, expect(o, b))
        assert (ran == ["k_small_mixed"]) == (n <= RC.SMALL_MAX), ran
        same_table(g, o.dump())
    finally:
        ring.close()   # (before its repo, whatever the test's outcome)
        g.close()
