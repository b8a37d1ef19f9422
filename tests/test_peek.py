"""phip_peek on the GPU (include/patrolhip.h "Peek"), through the binding.

The reference is tests/_peek_cases.py's: the oracle's table (oracle.Repo.get)
and its pure Take on a copy; status, remaining and have bit-exact, retry_at by
its definition.  The host form, the device form and phip_peek_eval of the
returned state column must all agree, a peek must equal a real take on a copy
of the handle, and no peek may change anything the handle holds.
"""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import go_semantics as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import _gen  # noqa: E402
from tests import _peek_cases as PC  # noqa: E402

T0, SEC = PC.T0, PC.SEC
FILL = 0x5A


@pytest.fixture(scope="module")
def pa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import patrol_amd
    return patrol_amd


def seeded(pa, tab, names=None, cols=None, **kw):
    """A handle and an oracle holding the same buckets."""
    kw.setdefault("log2_slots", 10)
    kw.setdefault("debug_tag_bits", 3)
    kw.setdefault("hash_seed", 11)
    names = tab["names"] if names is None else names
    a, t, e, c = tab["cols"] if cols is None else cols
    g, o = pa.GPURepo(**kw), O.Repo()
    g.seed(names, a, t, e, c)
    o.seed(names, a, t, e, c)
    assert len(g) == len(o) == len(names)
    return g, o


@pytest.fixture(scope="module")
def table(pa):
    """The forced-collision table (8 tags over 600 buckets), its oracle, 3 000
    queries and their references: computed once, shared, never changed."""
    tab = PC.table_case(3)
    g, o = seeded(pa, tab)
    queries = PC.table_queries(4, tab, 3000)
    refs = [PC.reference(o.get(q[0]), *q[1:]) for q in queries]
    k, absent = PC.check_mix(refs)
    print("table mix: %s, %d absent of %d" % (k, absent, len(queries)))
    yield g, o, queries, refs
    g.close()


def device_cols(queries, slack=256):
    import torch
    dev = torch.device("cuda", 0)
    names, now, freq, per, count = PC.columns(queries)
    offs = np.zeros(len(names) + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in names])
    blob = np.zeros(int(offs[-1]) + slack, np.uint8)
    blob[:offs[-1]] = np.frombuffer(b"".join(names), np.uint8)
    t = {k: torch.from_numpy(v).to(dev) for k, v in
         dict(names=blob, name_offs=offs, now=now, freq=freq, per=per,
              count=count.view(np.int64)).items()}
    return t, int(offs[-1])


def device_outs(n, which=("status", "remaining", "have", "retry_at", "state")):
    import torch
    dev = torch.device("cuda", 0)
    z = max(n, 1)
    out = {}
    for k in which:
        if k == "status":
            out[k] = torch.full((z,), FILL, dtype=torch.uint8, device=dev)
        elif k == "state":
            out[k] = torch.full((z, 4), FILL, dtype=torch.int64, device=dev)
        else:
            out[k] = torch.full((z,), FILL, dtype=torch.int64, device=dev)
    return out


def peek_device(g, queries, names_len=None):
    """-> the host form's dict, from the device form."""
    n = len(queries)
    t, nb = device_cols(queries)
    out = device_outs(n)
    g.peek_device(n, names_len=nb if names_len is None else names_len, **t, **out)
    st = out["state"].cpu().numpy()[:n]
    return dict(status=out["status"].cpu().numpy()[:n],
                remaining=out["remaining"].cpu().numpy()[:n].view(np.uint64),
                have=out["have"].cpu().numpy()[:n].view(np.uint64),
                retry_at=out["retry_at"].cpu().numpy()[:n],
                state=dict(a=st[:, 0].view(np.uint64), t=st[:, 1].view(np.uint64), e=st[:, 2],
                           c=st[:, 3]))


def rows(res, i):
    s = res["state"]
    return ((int(res["status"][i]), int(res["remaining"][i]), int(res["have"][i]),
             int(res["retry_at"][i])),
            (int(s["a"][i]), int(s["t"][i]), int(s["e"][i]), int(s["c"][i])))


def check_parity(pa, g, o, queries, refs=None):
    """Host form and device form against the reference, each other, and
    phip_peek_eval of the state column they return."""
    names, now, freq, per, count = PC.columns(queries)
    host = g.peek(names, now, freq, per, count)
    devr = peek_device(g, queries)
    for i, q in enumerate(queries):
        ref = refs[i] if refs is not None else PC.reference(o.get(q[0]), *q[1:])
        got, state = rows(host, i)
        assert (got, state) == rows(devr, i), (i, q)
        assert got[:3] == (ref["status"], ref["remaining"], ref["have"]), (i, q, got, ref)
        PC.check_retry(ref, (None,) + q[1:], got[3])
        assert state == ref["s"], (i, q)
        ev = pa.peek_eval(state, *q[1:])
        assert (ev[0] | (got[0] & PC.ABSENT),) + ev[1:] == got, (i, q, ev, got)
    return host


# 1 ------------------------------------------------------------------ parity --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 3000])
def test_parity_on_a_forced_collision_table(pa, table, n):
    g, o, queries, refs = table
    lo = 0 if n == 3000 else 7 * n          # (different queries at every size)
    check_parity(pa, g, o, queries[lo:lo + n], refs[lo:lo + n])


# 2 ------------------------------------------------------- equals a real take --
def test_peek_equals_a_real_take_on_a_copy(pa, table):
    g, o, queries, refs = table
    queries, refs = queries[1000:1500], refs[1000:1500]
    names, now, freq, per, count = PC.columns(queries)
    res = g.peek(names, now, freq, per, count)
    img = g.snapshot()
    g2 = pa.GPURepo(log2_slots=10, debug_tag_bits=3)

    def take(i, at):
        g2.restore(img)
        r = g2.apply_mixed([0], [names[i]], [at], [freq[i]], [per[i]], [count[i]])
        return int(r["status"][0]) & 0x3F, int(r["remaining"][0]), int(r["have"][0])

    for i in range(len(queries)):
        assert take(i, now[i]) == (int(res["status"][i]) & 0x3F, int(res["remaining"][i]),
                                   int(res["have"][i])), (i, queries[i])
    # a present bucket's take at retry_at is granted, one reading earlier denied
    # (an absent one would be created at retry_at, not at the query's now)
    later = [i for i, r in enumerate(refs) if r["klass"] == "finite" and not r["status"] & PC.ABSENT]
    assert len(later) >= 50
    for i in later[:50]:
        at = int(res["retry_at"][i])
        assert take(i, at)[0] == PC.OK and take(i, at - 1)[0] == PC.DENIED, (i, queries[i], at)
    g2.close()


# 3 ---------------------------------------------------------- nothing written --
def test_peek_writes_nothing(pa):
    tab = PC.table_case(5, 300)
    g, o = seeded(pa, tab, track_changes=True)
    rng = np.random.default_rng(1)
    # takes first, so that marks are pending and some buckets are new
    tn = [tab["names"][i] for i in rng.integers(0, 300, 200)] + tab["absent"][:50]
    ops = dict(kind=np.zeros(250, np.uint8), now=T0 + np.arange(250, dtype=np.int64),
               freq=np.full(250, 100, np.int64), per=np.full(250, SEC, np.int64),
               count=np.ones(250, np.uint64))
    z = np.zeros(250, np.uint64)
    for r in (g, o):
        r.apply_mixed(ops["kind"], tn, ops["now"], ops["freq"], ops["per"], ops["count"], z, z,
                      z.view(np.int64))

    def held():
        # (a dump lists the buckets in no fixed order: by name)
        nb, offs, a, t, e, c = g.dump_arrays()
        raw = nb.tobytes()
        dump = {raw[int(offs[i]):int(offs[i + 1])]: (int(a[i]), int(t[i]), int(e[i]), int(c[i]))
                for i in range(len(a))}
        assert len(dump) == len(a)
        return (dump, len(g), g.capacity, g.snapshot().tobytes(), g.changes_count())
    before = held()
    assert before[4]["pending"] > 0
    queries = PC.table_queries(6, tab, 3000, p_absent=0.5)
    absent = sum(o.get(q[0]) is None for q in queries)
    assert 1200 <= absent <= 1800, absent
    names, now, freq, per, count = PC.columns(queries)
    host = g.peek(names, now, freq, per, count)
    devr = peek_device(g, queries)
    assert all(np.array_equal(host[k], devr[k]) for k in ("status", "remaining", "have", "retry_at"))
    assert int(((host["status"] & PC.ABSENT) != 0).sum()) == absent
    assert held() == before
    # a following batch equals the oracle that never saw the peeks
    tn2 = [q[0] for q in queries[:400]]
    a2 = (g.apply_mixed(np.zeros(400, np.uint8), tn2, now[:400], freq[:400], per[:400], count[:400]),
          o.apply_mixed(np.zeros(400, np.uint8), tn2, now[:400], freq[:400], per[:400], count[:400],
                        np.zeros(400, np.uint64), np.zeros(400, np.uint64), np.zeros(400, np.int64)))
    for k in ("status", "remaining", "have"):
        assert np.array_equal(a2[0][k], a2[1][k]), k
    assert {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()} == o.dump()
    g.close()


# 4 ------------------------------------------------------ after layout changes --
def test_parity_after_growth_and_eviction(pa):
    tab = PC.table_case(7, 600)
    # half of the buckets last touched 100 s before T0, half at T0
    a, t, e, c = (x.copy() for x in tab["cols"])
    e[:] = np.arange(600) * 1000
    old = np.arange(600) % 2 == 0
    c[:] = np.where(old, T0 - 100 * SEC, T0) - e
    g, o = seeded(pa, tab, cols=(a, t, e, c), log2_slots=8)
    assert g.capacity > 256                 # seeded past the load limit: the table grew
    tab = dict(tab, states=[(int(a[k]), int(t[k]), int(e[k]), int(c[k])) for k in range(600)])
    check_parity(pa, g, o, PC.table_queries(8, tab, 600))
    st = g.evict_idle(T0 + SEC, 50 * SEC)
    assert st["evicted"] == 300 and len(g) == 300
    keep = [k for k in range(600) if not old[k]]
    o2 = O.Repo()
    o2.seed([tab["names"][k] for k in keep], a[keep], t[keep], e[keep], c[keep])
    queries = PC.table_queries(9, tab, 600, p_absent=0.0)
    host = check_parity(pa, g, o2, queries)
    gone = np.array([o2.get(q[0]) is None for q in queries])
    assert 200 <= gone.sum() <= 400
    assert np.array_equal((host["status"] & PC.ABSENT) != 0, gone)
    g.close()


# 5 -------------------------------------------------------------- queued batch --
def test_peek_finishes_a_queued_batch_and_sees_its_merges(pa):
    import torch
    dev = torch.device("cuda", 0)
    n, K = 1 << 16, 100
    rng = np.random.default_rng(12)
    g, o = pa.GPURepo(log2_slots=10), O.Repo()
    names = _gen.key_names(rng.integers(0, K, n))
    a, t, e = _gen.clean_states(rng, n)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(x) for x in names])
    blob = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 8, np.uint8).copy()).to(dev)
    to = torch.from_numpy(offs).to(dev)
    ta, tt, te = (torch.from_numpy(x.view(np.int64).copy()).to(dev) for x in (a, t, e))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    g.receive_soa(blob, ta, tt, te, T0, name_offs=to, n=n, status=status, device=True, queue=True)
    # no flush: the peek finishes the batch
    queries = [(b"b%d" % k, T0 + SEC, 100, SEC, 1) for k in range(K)]
    res = peek_device(g, queries)
    want, _, _, _ = o.receive_soa(names, a, t, e, T0)
    assert np.array_equal(status.cpu().numpy(), want)
    for k, q in enumerate(queries):
        s = o.get(q[0])
        assert s is not None and rows(res, k)[1] == s, (k, q)
        PC.check_one((s,) + q[1:], rows(res, k)[0])
    g.flush()
    g.close()


# 6 ------------------------------------------------ NULL columns and n = 0 --
def test_null_result_columns_and_empty_batch(pa, table):
    g, o, queries, refs = table
    queries = queries[2000:2100]
    n = len(queries)
    full = peek_device(g, queries)
    names, now, freq, per, count = PC.columns(queries)
    t, nb = device_cols(queries)
    for col in ("status", "remaining", "have", "retry_at", "state"):
        out = device_outs(n, which=(col,))
        g.peek_device(n, names_len=nb, **t, **out)
        got = out[col].cpu().numpy()
        if col == "state":
            want = np.stack([full["state"][k].view(np.int64) for k in "atec"], axis=1)
        else:
            want = full[col].view(got.dtype)
        assert np.array_equal(got, want), col
    g.peek_device(n, names_len=nb, **t)          # no result column at all
    # no operand column: every one reads as zeros
    z = np.zeros(n, np.int64)
    out = device_outs(n)
    g.peek_device(n, t["names"], t["name_offs"], None, names_len=nb, **out)
    want = g.peek(names, z, z, z, z.view(np.uint64))
    assert np.array_equal(out["status"].cpu().numpy(), want["status"])
    assert np.array_equal(out["retry_at"].cpu().numpy(), want["retry_at"])
    # n = 0
    out = device_outs(0)
    g.peek_device(0, t["names"], t["name_offs"], t["now"], names_len=nb, **out)
    assert int(out["status"][0]) == FILL
    empty = g.peek([], [], [], [], [])
    assert all(len(empty[k]) == 0 for k in empty)
    assert g.L.phip_peek(g.h, None, None, 0) == -1


# 7 ------------------------------------------------------------ checked offsets --
@pytest.mark.parametrize("how", ["descending", "past_the_blob"])
def test_malformed_offsets_are_refused_untouched(pa, table, how):
    import torch
    g, o, queries, refs = table
    queries = queries[2200:2500]
    n = len(queries)
    t, nb = device_cols(queries, slack=256)     # 256 owned bytes past names_len
    offs = t["name_offs"].cpu().numpy().copy()
    if how == "descending":
        i = 150
        offs[i] = offs[i + 1] + 3                # offs[i] > offs[i + 1]
    else:
        offs[n] = nb + 5                         # a few bytes past names_len
    t["name_offs"] = torch.from_numpy(offs).to(t["names"].device)
    out = device_outs(n)
    with pytest.raises(pa.PatrolHipError) as err:
        g.peek_device(n, names_len=nb, **t, **out)
    assert err.value.code == -1
    for k, v in out.items():
        assert bool((v.cpu() == FILL).all()), k
    # the handle still answers
    check_parity(pa, g, o, queries[:10], refs[2200:2210])


def test_flags_and_long_names(pa, table):
    g, o, queries, refs = table
    import ctypes as C
    from patrol_amd import _lib
    blob, offs = pa.names_blob([b"a"])
    q = _lib.phip_ops(1, 0, None, blob.ctypes.data, offs.ctypes.data, None, None, None, None, None,
                      None, None)
    for fl in (0x2, 0x20, 0x100, 0x200):
        assert g.L.phip_peek(g.h, C.byref(q), None, fl) == -1, fl
    assert g.L.phip_peek(g.h, C.byref(q), None, 0) == 0
    with pytest.raises(pa.PatrolHipError) as err:
        g.peek([b"x" * 232], [T0], [1], [SEC], [1])
    assert err.value.code == -6


# 8 -------------------------------------------------------------------- api_peek --
def test_api_peek_matches_the_handler_on_a_copy(pa):
    with open(os.path.join(os.path.dirname(__file__), "golden", "api_table.json")) as f:
        gold = json.load(f)
    sb = gold["seed_bucket"]
    g = pa.GPURepo(log2_slots=10)
    g.seed([sb["name"].encode()], [0], [0], [0], [sb["created"]])
    repo = G.LocalRepo(G.Bucket(name=sb["name"], created=sb["created"]))

    def dump():
        return {k: (v.added, v.taken, v.elapsed, v.created) for k, v in g.dump().items()}
    # every row peeked on the table as seeded: nothing moves
    before = dump()
    for r in gold["requests"]:
        want = G.api_take(copy.deepcopy(repo), r["name"], r["rate"], r["count"], r["now"])
        code, body, after = g.api_peek(r["name"].encode(), r["rate"].encode(), r["count"].encode(),
                                       r["now"])
        assert (code, body) == want, r
    assert dump() == before and len(g) == 1
    # and row by row ahead of the real handler: the peek predicts it, and its
    # retry_after_ns is phip_peek's retry_at - now
    for r in gold["requests"]:
        name, rate, count = r["name"].encode(), r["rate"].encode(), r["count"].encode()
        before = dump()
        code, body, after = g.api_peek(name, rate, count, r["now"])
        assert dump() == before
        assert (code, body) == G.api_take(copy.deepcopy(repo), r["name"], r["rate"], r["count"],
                                          r["now"]), r
        assert (code, body) == (r["code"], r["body"]), r
        if code != 400:
            freq, per, _ = pa.parse_rate(rate)
            cnt = G.go_parse_uint10(r["count"])[0] or 1
            p = g.peek([name], [r["now"]], [freq], [per], [cnt])
            at = int(p["retry_at"][0])
            want = 0 if code == 200 else -1 if at == PC.NEVER else min(at - r["now"], PC.I64_MAX)
            assert after == want, (r, after, at)
            assert code == 429 or at == r["now"]
        else:
            assert after is None
        assert g.api_take(name, rate, count, r["now"]) == (r["code"], r["body"])
        assert G.api_take(repo, r["name"], r["rate"], r["count"], r["now"]) == (r["code"], r["body"])
    g.close()
