"""Group reply egress (include/patrolhip.h "Group reply egress"): the model and
the case builders of tests/test_group_replies.py.

The model feeds one oracle.Repo round by round, the sources in rank order, as
the group defines a bucket's order (round, source rank, index in the source's
batch).  The oracle's status and reply columns are kept per (member, round)
slice and concatenated per member; tests/_replies_cases.expected then gives the
datagrams member i must get back.  `replies` and `skipped` are counted in the
group form's terms from the same columns and the owner map: `replies` excludes
the answers no owner wrote (names over 231 bytes), `skipped` counts those at
the member that owns the bucket, whoever asked.

Each case is checked on the CPU, from the oracle's columns alone, for what it
is meant to hold (check_group_case)."""
import numpy as np

from oracle import go_semantics as G
from oracle import oracle as O
from tests import _gen
from tests import _replies_cases as RC

CHUNK = 4096   # PHIP_GROUP_SMALL_CHUNKS
NEG0 = RC.NEG0
REPLY, NOREPLY, CREATED = RC.REPLY, RC.NOREPLY, RC.CREATED
NOW = _gen.T0 + 5 * _gen.SEC

_owner_cache = {}


def owner(name: bytes, world: int) -> int:
    """The shard map of patrolhip.h: ((fnv1a64(name) >> 32) * world) >> 32."""
    h = _owner_cache.get(name)
    if h is None:
        h = _owner_cache[name] = G.fnv1a64(name)
    return ((h >> 32) * world) >> 32


def bucket_name(k: int) -> bytes:
    """Short names, and every seventh of arena length (over 22 bytes)."""
    return (b"an-arena-length-bucket-name-%d" % k) if k % 7 == 0 else b"b%d" % k


def rounds_of(sizes, chunk):
    return max(1, max((n + chunk - 1) // chunk for n in sizes))


def model(o, per, now, chunk, stops=None):
    """Feed oracle `o` the members' datagram lists round by round -> per member
    (st, ra, rt, re) over its datagrams before its stop."""
    sizes = [len(d) if stops is None else stops[i] for i, d in enumerate(per)]
    cols = [[] for _ in per]
    for c in range(rounds_of(sizes, chunk)):
        for i, d in enumerate(per):
            part = d[c * chunk:min(sizes[i], (c + 1) * chunk)]
            if part:
                st, ra, rt, re, stop = o.receive(part, now)
                assert stop == len(part)
                cols[i].append((st[:len(part)], ra[:len(part)], rt[:len(part)], re[:len(part)]))
    out = []
    for i, cs in enumerate(cols):
        if cs:
            out.append(tuple(np.concatenate([c[j] for c in cs]) for j in range(4)))
        else:
            out.append((np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint64),
                        np.zeros(0, np.int64)))
    return out


def expected(names_per, cols, world, max_msgs=None, budget=None):
    """-> one dict per member in the group form's terms."""
    skipped = [0] * world
    for names, (st, _, _, _) in zip(names_per, cols):
        for i in np.nonzero((st & 0x7F) == REPLY)[0]:
            if len(names[int(i)]) > 231:
                skipped[owner(names[int(i)], world)] += 1
    out = []
    for r, (names, (st, ra, rt, re)) in enumerate(zip(names_per, cols)):
        e = RC.expected(names[:len(st)], st, ra, rt, re, max_msgs, budget)
        e["replies"] -= e["skipped"]
        e["skipped"] = skipped[r]
        out.append(e)
    return out


def warm_batches(world, K, seed, zero=8, long_lens=()):
    """A first call that creates the K buckets with clean states, plus `zero`
    buckets z0.. that an (unanswered) request creates with the zero state and
    one bucket per entry of long_lens under a name of that length (232..255:
    only a datagram brings one in)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(K)
    per = []
    for r in range(world):
        mine = ids[r::world]
        names = [bucket_name(int(k)) for k in mine]
        a, t, e = _gen.clean_states(rng, len(names))
        if r == 0:
            names += [b"z%d" % k for k in range(zero)]
            a = np.concatenate([a, np.zeros(zero, np.uint64)])
            t = np.concatenate([t, np.zeros(zero, np.uint64)])
            e = np.concatenate([e, np.zeros(zero, np.int64)])
            la, lt, le = _gen.clean_states(rng, len(long_lens))
            names += [long_name(L) for L in long_lens]
            a, t, e = np.concatenate([a, la]), np.concatenate([t, lt]), np.concatenate([e, le])
        per.append(RC.wire(names, a, t, e))
    return per


def _pick(world, K, asker, own: bool, used, start=0):
    """A bucket id whose owner is (own) / is not (not own) the asking member."""
    for k in range(start, K):
        nm = bucket_name(k)
        if k not in used and (owner(nm, world) == asker) == own:
            used.add(k)
            return k
    raise AssertionError("no such bucket")


def make_group_case(world, sizes, seed, K=3000, extra=40, absent=6, zero=6, negzero=6,
                    long_names=0, chunk=CHUNK):
    """Member batches of `sizes` Zipf messages over the K warm buckets with
    requests planted:
      edge     at index 0, 4095, 4096 and the last index of every member that
               has them, alternately to a bucket the asker owns and to one it
               does not;
      shared   one bucket asked by members 0 and 1 in round 0, member 0 (the
               lower rank) raising it in between;
      again    one bucket asked by the last non-empty member in rounds 0 and 1
               with a raising merge in between (needs a batch over one chunk);
      extra    random requests, a third of them to arena-length names;
      absent / zero / negzero as tests/_replies_cases.make_case;
      long     requests under names of 232..255 bytes (brought in by the
               caller's warm call).
    -> dict(names, a, t, e per member, tags per member)."""
    rng = np.random.default_rng(seed)
    names, A, T, E, tags = [], [], [], [], []
    for n in sizes:
        ids = _gen.zipf_ids(rng, n, K) if n else np.zeros(0, np.int64)
        names.append([bucket_name(int(k)) for k in ids])
        a, t, e = _gen.clean_states(rng, n)
        A.append(a); T.append(t); E.append(e)
        tags.append({})
    used, taken_pos = set(), [set() for _ in sizes]

    def ask(r, kind, p, name, av=0, tv=0):
        assert p not in taken_pos[r], (r, p)
        taken_pos[r].add(p)
        names[r][p] = name
        A[r][p], T[r][p], E[r][p] = av, tv, 0
        tags[r].setdefault(kind, []).append(p)

    def raise_at(r, p, name, k):
        assert p not in taken_pos[r]
        taken_pos[r].add(p)
        names[r][p] = name
        A[r][p] = np.float64(3e6 + k).view(np.uint64)
        T[r][p] = np.float64(2e6 + k).view(np.uint64)
        E[r][p] = (1 << 41) + k

    flip = 0
    for r, n in enumerate(sizes):
        for p in sorted({0, 4095, 4096, n - 1}):
            if 0 <= p < n:
                k = _pick(world, K, r, own=bool(flip & 1) or world == 1, used=used)
                ask(r, "edge_own" if owner(bucket_name(k), world) == r else "edge_other", p,
                    bucket_name(k))
                flip += 1
    if world >= 2 and sizes[0] >= 300 and sizes[1] >= 3:
        k = _pick(world, K, 0, own=False, used=used)
        ask(0, "shared", 100, bucket_name(k))
        raise_at(0, 200, bucket_name(k), 1)
        ask(1, "shared", 1, bucket_name(k))
    big = [r for r, n in enumerate(sizes) if n > chunk + 100]
    if big:
        r = big[-1]
        k = _pick(world, K, r, own=world == 1, used=used)
        ask(r, "again", 300, bucket_name(k))
        raise_at(r, 400, bucket_name(k), 2)
        ask(r, "again", chunk + 50, bucket_name(k))
    for r, n in enumerate(sizes):
        if n < 1000:
            continue
        free = [p for p in rng.permutation(n).tolist() if p not in taken_pos[r]]
        for j in range(extra):
            ask(r, "extra", free.pop(), bucket_name(7 * int(rng.integers(0, K // 7)) if j % 3 == 0
                                                    else int(rng.integers(0, K))))
        for j in range(absent):
            ask(r, "absent", free.pop(), b"n%d-%d" % (r, j))
        for j in range(zero):
            ask(r, "zero", free.pop(), b"z%d" % j)
        for j in range(negzero):
            ask(r, "negzero", free.pop(), bucket_name(int(rng.integers(0, K))), NEG0,
                NEG0 if j % 2 else 0)
        for j in range(long_names):
            ask(r, "long", free.pop(), long_name(232 + (j * 5 + r) % 24))   # (warm: long_lens)
    return dict(names=names, a=A, t=T, e=E, tags=tags, world=world, sizes=list(sizes))


def long_name(length: int) -> bytes:
    return (b"%03d-a-name-MarshalBinary-refuses-" % length * 9)[:length]


def datagrams(case):
    return [RC.wire(case["names"][r], case["a"][r], case["t"][r], case["e"][r])
            for r in range(len(case["names"]))]


def check_group_case(case, cols, *, edge_own=0, edge_other=0, shared=False, again=False,
                     answered=4, absent=4, zero=4, negzero=4, long=0):
    """What the case is for, from the oracle's columns alone."""
    world = case["world"]
    n_rep = n_abs = n_zero = n_neg = n_long = n_eo = n_ex = 0
    for r, (st, ra, rt, re) in enumerate(cols):
        st7 = st & 0x7F
        tg = case["tags"][r]
        n_rep += int((st7 == REPLY).sum())
        n_abs += sum(1 for p in tg.get("absent", []) if st[p] == NOREPLY | CREATED)
        n_zero += sum(1 for p in tg.get("zero", []) if st[p] == NOREPLY)
        n_neg += sum(1 for p in tg.get("negzero", []) if st7[p] in (REPLY, NOREPLY))
        n_long += sum(1 for p in tg.get("long", []) if st7[p] == REPLY and len(case["names"][r][p]) > 231)
        for p in tg.get("edge_own", []):
            assert owner(case["names"][r][p], world) == r and st7[p] == REPLY
            n_eo += 1
        for p in tg.get("edge_other", []):
            assert owner(case["names"][r][p], world) != r and st7[p] == REPLY
            n_ex += 1
    assert n_rep >= answered and n_abs >= absent and n_zero >= zero and n_neg >= negzero
    assert n_long >= long and n_eo >= edge_own and n_ex >= edge_other
    if shared:   # member 1's answer holds what member 0 raised after its own request
        p0, p1 = case["tags"][0]["shared"][0], case["tags"][1]["shared"][0]
        s0, s1 = cols[0], cols[1]
        assert (s0[0][p0] & 0x7F) == REPLY and (s1[0][p1] & 0x7F) == REPLY
        assert case["names"][0][p0] == case["names"][1][p1]
        assert p0 < CHUNK and p1 < CHUNK
        assert (s0[1][p0], s0[2][p0], s0[3][p0]) != (s1[1][p1], s1[2][p1], s1[3][p1])
        assert s1[3][p1] == (1 << 41) + 1
    if again:
        r = [i for i, tg in enumerate(case["tags"]) if "again" in tg][-1]
        p1, p3 = case["tags"][r]["again"]
        st, ra, rt, re = cols[r]
        assert p1 < CHUNK <= p3 and (st[p1] & 0x7F) == REPLY and (st[p3] & 0x7F) == REPLY
        assert re[p3] == (1 << 41) + 2 and re[p1] != re[p3]


def build(world, sizes, seed, chunk=CHUNK, K=3000, **kw):
    """The warm call, the case, the oracle after both and the model's columns."""
    warm = warm_batches(world, K, seed, long_lens=range(232, 256) if kw.get("long_names") else ())
    case = make_group_case(world, sizes, seed + 1, K=K, chunk=chunk, **kw)
    per = datagrams(case)
    o = O.Repo()
    model(o, warm, _gen.T0, 1 << 24)
    cols = model(o, per, NOW, chunk)
    return dict(warm=warm, case=case, per=per, oracle=o, cols=cols)
