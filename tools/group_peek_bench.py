#!/usr/bin/env python3
"""Owner-routed peek over the shard group, timed (not the bench).

The table is C2's: 10M buckets b"b%d", each holding 7 tokens of a 100:1s rate
(tools/peek_bench.py's).  2^24 queries drawn as C3 draws names (Zipf 1.1), once
all granted (count 1) and once all denied with a later answer (count 50: every
lane bisects), through

  (a) phip_peek on one handle: the yardstick;
  (b) GPUGroup.peek at world 1 with PHIP_GROUP_RCCL_SELF: the query pack, the
      RCCL exchange to itself, the owner's phip_peek, the answers' way back;
  (c) GPUGroup.peek over two shards on one GPU (device copies), each member
      submitting half of the queries;
  (d) GPUGroup.apply_mixed of the same names and operands as TAKE ops, at
      world 1 self and over two shards, on groups of their own seeded alike
      (the takes drain them): until phip_group_peek the only group call that
      reached another member's bucket;
  (p) phip_group_apply_mixed of (d) in the parent commit's library
      (--parent-lib, loaded beside this one), to show the ops path did not move.

All forms alternate in one run, rotating which goes first; a step's time is a
host clock around the call, which ends in a stream synchronise; every figure
is the median of --reps steps after --warmup.  (b) and (c) also report
phip_group_stage_ms of the last step.  Beside them the pack alone for 8
owners: the query pack and phip_route_pack_ops over the same names, from
phip_last_timings (HIP events).

Writes profiles/group_peek_bench.json (--out) with the library's build id.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.evict_bench import make_names  # noqa: E402

SEC = 10**9
T0 = bench.T0


def med(xs):
    return float(statistics.median(xs)) if xs else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="one table holding every bucket")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--route-world", type=int, default=8)
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "var", "libpatrolhip_parent.so"),
                   help="the parent commit's libpatrolhip.so ('' or missing: (p) is not measured)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_peek_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib, shard
    from patrol_amd.engine import GPUGroup, phip_config, phip_ops, phip_results
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    n, K, L, W, R = args.queries, args.buckets, args.log2_slots, args.warmup, args.reps
    out = dict(tool="tools/group_peek_bench.py", build_id=_lib.build_id(), queries=n, buckets=K,
               zipf=1.1, reps=R, warmup=W, device=torch.cuda.get_device_name(0))
    Lp = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        cur, _lib._lib = _lib._lib, None
        try:
            Lp = _lib.load(args.parent_lib)
        finally:
            _lib._lib = cur
        out["parent_build_id"] = Lp.phip_build_id().decode()
        assert out["parent_build_id"] != out["build_id"], "--parent-lib is this build"

    # C2's table, and its split over two owners
    kb, ko = make_names(torch, K, 0.0, dev)

    def states(ids):
        st = torch.zeros((ids.numel(), 4), dtype=torch.int64, device=dev)
        st[:, 0] = 0x4024000000000000            # added 10.0
        st[:, 1] = 0x4008000000000000            # taken 3.0
        st[:, 2] = ids                           # elapsed: bucket b%d has refilled for d ns
        st[:, 3] = T0
        return st
    every = torch.arange(K, dtype=torch.int64, device=dev)
    repo = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20, max_load_pct=45)
    repo.seed_device(kb, ko, states(every), K)
    assert len(repo) == K
    own = shard.owner_of(shard.hash_names(kb, ko, repo), 2)[:K]
    halves = []
    for r in range(2):
        ids = torch.nonzero(own == r).flatten()
        hb, ho = bench.names_for_ids(torch, ids)
        halves.append((hb, ho, ids))
    del own

    def open_parent(devices, log2):
        cfg = phip_config(0, log2, 1 << 20, 45, 0, 0, 0, 0)
        devs = (C.c_int32 * len(devices))(*devices)
        g = C.c_void_p()
        assert Lp.phip_group_open_all(C.byref(cfg), devs, len(devices), C.byref(g)) == 0
        repos = [patrol_amd.GPURepo.wrap(Lp.phip_group_handle(g, i), devices[i])
                 for i in range(len(devices))]
        for r in repos:   # a parent handle is the parent library's to touch
            r.L = Lp
        return GPUGroup(g, Lp, repos)

    def group(world, parent=False):
        devices, log2 = [0] * world, L - (world - 1)
        g = open_parent(devices, log2) if parent else \
            GPUGroup.open_all(devices, log2_slots=log2, arena_bytes=1 << 20, max_load_pct=45)
        if world == 1:
            g.repos[0].seed_device(kb, ko, states(every), K)
        else:
            for r, (hb, ho, ids) in enumerate(halves):
                g.repos[r].seed_device(hb, ho, states(ids), int(ids.numel()))
        assert sum(len(r) for r in g.repos) == K
        g.set_timing(True)
        return g

    forms = ["a_peek_one_handle", "b_peek_world1_rccl_self", "c_peek_shared_world2",
             "d_take_world1_rccl_self", "d_take_shared_world2"]
    if Lp is not None:
        forms += ["p_take_world1_rccl_self", "p_take_shared_world2"]
    G = {f: group(1 if "world1" in f else 2, f.startswith("p_")) for f in forms[1:]}

    ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
    blob, offs = bench.names_for_ids(torch, ids)
    del ids
    # every `last` lies in [T0, T0 + 10 ms): at this reading a bucket holds at
    # most 8 of its 100 tokens, so count 1 is granted and count 50 is denied
    # with an answer about 0.4 s later
    now_q = T0 + 10_000_001
    now = torch.full((n,), now_q, dtype=torch.int64, device=dev)
    freq = torch.full((n,), 100, dtype=torch.int64, device=dev)
    per = torch.full((n,), SEC, dtype=torch.int64, device=dev)
    kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    cut = [0, n // 2, n]

    def cols(z):
        return dict(status=torch.zeros(z, dtype=torch.uint8, device=dev),
                    **{k: torch.zeros(z, dtype=torch.int64, device=dev)
                       for k in ("remaining", "have", "retry_at")})
    one = cols(n)
    res = {1: [cols(n)], 2: [cols(cut[1]), cols(n - cut[1])]}

    def batches(world, cnt, take):
        bs = []
        for i in range(world):
            lo, hi = (0, n) if world == 1 else (cut[i], cut[i + 1])
            b = dict(names=blob, name_offs=offs[lo:hi + 1], now=now[lo:hi], freq=freq[lo:hi],
                     per=per[lo:hi], count=cnt[lo:hi])
            if take:
                b.update(kind=kind[lo:hi], added=None, taken=None, elapsed=None)
            bs.append(b)
        return bs

    def raw_take(g, bs, rs):
        """phip_group_apply_mixed through g's own library (the parent's too)."""
        k = len(bs)
        ops, rr = (phip_ops * k)(), (phip_results * k)()
        for i, b in enumerate(bs):
            ops[i] = phip_ops(b["name_offs"].numel() - 1, 0, b["kind"].data_ptr(), blob.data_ptr(),
                              b["name_offs"].data_ptr(), b["now"].data_ptr(), b["freq"].data_ptr(),
                              b["per"].data_ptr(), b["count"].data_ptr(), None, None, None)
            rr[i] = phip_results(rs[i]["status"].data_ptr(), rs[i]["remaining"].data_ptr(),
                                 rs[i]["have"].data_ptr(), None)
        flags = _lib.DEVICE_PTRS | (_lib.GROUP_RCCL_SELF if k == 1 else 0)
        g._check(g.L.phip_group_apply_mixed(g.g, ops, rr, None, None, flags))

    rows = {}
    for label, c in (("all_ok", 1), ("all_denied", 50)):
        cnt = torch.full((n,), c, dtype=torch.int64, device=dev)
        ms = {f: [] for f in forms}
        stage = {}
        for j in range(W + R):
            for f in forms[j % len(forms):] + forms[:j % len(forms)]:   # none always runs first
                world = 1 if ("world1" in f or f[0] == "a") else 2
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if f[0] == "a":
                    repo.peek_device(n, blob, offs, now, freq, per, cnt, names_len=0, **one)
                elif f[0] in "bc":
                    _, sent, answered = G[f].peek(batches(world, cnt, False), rccl_self=world == 1,
                                                  results=res[world])
                else:
                    raw_take(G[f], batches(world, cnt, True), res[world])
                ms[f].append((time.perf_counter() - t0) * 1e3)
                if f[0] in "bc":
                    assert sum(sent) == n and sum(answered) == n
                    stage[f] = [G[f].stage_ms(i) for i in range(world)]
                    got = torch.cat([r["status"] for r in res[world]])
                    assert torch.equal(got, one["status"]), f
                    assert all(torch.equal(torch.cat([r[k] for r in res[world]]), one[k])
                               for k in ("remaining", "have", "retry_at")), f
            want = _lib.ST_TAKE_OK if c == 1 else _lib.ST_TAKE_DENIED
            assert bool((one["status"] == want).all())
            assert bool((one["retry_at"] == now_q).all() if c == 1 else (one["retry_at"] > now_q).all())
        row = {f: dict(ms=med(v[W:]), min_ms=min(v[W:]), max_ms=max(v[W:]),
                       all_ms=[round(x, 3) for x in v[W:]]) for f, v in ms.items()}
        for f, s in stage.items():
            row[f]["stage_ms"] = s
        ratios = dict(b_over_a=row[forms[1]]["ms"] / row[forms[0]]["ms"],
                      c_over_a=row[forms[2]]["ms"] / row[forms[0]]["ms"],
                      b_over_d=row[forms[1]]["ms"] / row[forms[3]]["ms"],
                      c_over_d=row[forms[2]]["ms"] / row[forms[4]]["ms"])
        if Lp is not None:
            for d, q in ((forms[3], forms[5]), (forms[4], forms[6])):
                spread = max(row[d]["max_ms"] - row[d]["min_ms"], row[q]["max_ms"] - row[q]["min_ms"])
                ratios[d + "_minus_parent_ms"] = row[d]["ms"] - row[q]["ms"]
                ratios[d + "_run_spread_ms"] = spread
                ratios[d + "_inside_spread"] = abs(row[d]["ms"] - row[q]["ms"]) <= spread
        row["ratios"] = ratios
        rows[label] = row
        print(json.dumps({label: row}), flush=True)
    out["runs"] = rows
    # nothing was written by the peeks: the peeked groups still hold C2's table
    assert all(sum(len(r) for r in G[f].repos) == K for f in forms[1:3])
    for g in G.values():
        g.close()

    # the pack alone, 8 owners: the query pack and the ops pack over the same names
    Wr = args.route_world
    repo.set_timing(True)
    cnt = torch.ones(n, dtype=torch.int64, device=dev)
    qry_ms, ops_ms = [], []
    for _ in range(W + R):
        for kd, sink in ((None, qry_ms), (kind, ops_ms)):
            repo.route_pack_ops_device(n, Wr, kd, blob, offs, now, freq, per, cnt, names_len=0)
            tm = dict()
            for nm, x in repo.timings():
                tm[nm] = tm.get(nm, 0.0) + x
            sink.append(tm)

    def kernels(rs):
        return {nm: med([r[nm] for r in rs[W:]]) for nm in rs[-1]}
    kq, kk = kernels(qry_ms), kernels(ops_ms)
    out["route_pack_8_owners"] = dict(
        world=Wr, query_pack=dict(kernels_ms=kq, total_ms=sum(kq.values())),
        phip_route_pack_ops=dict(kernels_ms=kk, total_ms=sum(kk.values())))
    print(json.dumps(out["route_pack_8_owners"]), flush=True)
    repo.close()
    out["note"] = ("one MI355X; the RCCL exchange at world > 1 (one GPU per rank) has not run on "
                   "hardware")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
