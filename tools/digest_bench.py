#!/usr/bin/env python3
"""Partition digest timings (not the bench): phip_table_digest and the
digest-filtered sweep on C2's table, 10M buckets in 2^25 slots with b"b%d"
names -- the table tools/export_sweep_bench.py builds.  One process:

  levels     phip_table_digest (device pointers) at k = 0, 8, 12, 13, 16, 20,
             beside count mode and the one-call full sweep: kernel times from
             phip_last_timings (HIP events around each launch) and a HIP event
             pair around the whole call (the clear of the k >= 13 result and
             the host round trips are in that one only).  Medians of --reps
             after --warmup.
  reconcile  two handles with different placement seeds; B is A with D buckets
             raised (a merge of a higher elapsed), D in 100, 10 000, 1 000 000,
             at k = 12, 16, 20.  A round: both digests, phip_digest_diff, A's
             differing partitions swept into B's phip_receive_datagrams, then
             B's into A's, all with device pointers, --chunk datagrams a call.
             Per row: partitions that differ, datagrams sent, kernel ms of the
             two digests and the two filtered sweeps, the receives' kernel ms,
             and `verified`: both tables' digests at k = 20 are equal
             afterwards.  Medians of --round-reps rounds (each raises D
             buckets again).

Writes profiles/digest_bench.json (--out) with the library's build id.  Keys
the tool does not write (ab_unfiltered_sweep: the unfiltered sweep of this
build against a library built before the partition flag, merged in by
tools/sweep_ab.py) are kept when the file is rewritten.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.evict_bench import make_names  # noqa: E402

T0 = bench.T0
LEVELS = (0, 8, 12, 13, 16, 20)
SWEEP_KERNELS = ("k_sweep_count", "k_sweep_scan", "k_sweep_write")
DIGEST_KERNELS = ("k_digest", "k_digest_reduce")


def med(xs):
    return float(statistics.median(xs)) if xs else None


def kernels(repo):
    out = {}
    for nm, ms in repo.timings():
        out[nm] = out.get(nm, 0.0) + ms
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="the table the buckets end up in")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--round-reps", type=int, default=3)
    p.add_argument("--chunk", type=int, default=1 << 20, help="datagrams per sweep call of a round")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    K, L = args.buckets, args.log2_slots
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    res = dict(tool="tools/digest_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               max_load_pct=pct, reps=args.reps, warmup=args.warmup, round_reps=args.round_reps,
               device=torch.cuda.get_device_name(0))

    kb, ko = make_names(torch, K, 0.0, dev)
    st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
    st[:, 0] = 0x4024000000000000          # added 10.0, taken 3.0, elapsed = id
    st[:, 1] = 0x4008000000000000
    st[:, 2] = torch.arange(K, dtype=torch.int64, device=dev)
    st[:, 3] = T0

    def table(seed):
        repo = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct,
                                  hash_seed=seed)
        repo.use_torch_stream()
        repo.seed_device(kb, ko, st, K)
        assert len(repo) == K and repo.capacity == 1 << L
        repo.set_timing(True, accumulate=True)
        return repo

    A = table(1)
    total = args.warmup + args.reps

    def timed(repo, fn):
        """-> (per-kernel medians, median event ms of the whole call, last result)."""
        ks, calls, r = [], [], None
        for _ in range(total):
            repo.set_timing(True, accumulate=True)   # (drops what came before)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            r = fn()
            b.record(stream)
            b.synchronize()
            calls.append(a.elapsed_time(b))
            ks.append(kernels(repo))
        ks, calls = ks[args.warmup:], calls[args.warmup:]
        names = sorted({k for d in ks for k in d})
        return {k: med([d.get(k, 0.0) for d in ks]) for k in names}, med(calls), r

    # ---- levels ----
    km, call, cnt = timed(A, lambda: A.sweep_count())
    assert cnt["n"] == K, cnt
    count_ms = km["k_sweep_count"]
    lv = dict(count=dict(kernels_ms=km, call_ms=call, n=cnt["n"], bytes=cnt["bytes"]))
    out = torch.empty((cnt["bytes"] + 8 + 7) // 8 * 8, dtype=torch.uint8, device=dev)
    offs = torch.empty(K + 1, dtype=torch.int64, device=dev)
    km, call, r = timed(A, lambda: A.export_sweep_device(out, offs, None, K))
    assert r[0] == K and r[2]["done"] == 1
    sweep_ms = sum(km.get(k, 0.0) for k in SWEEP_KERNELS)
    lv["sweep_one_call"] = dict(kernels_ms=km, sweep_kernels_ms=sweep_ms, call_ms=call)
    dig = torch.empty((1 << 20, 2), dtype=torch.int64, device=dev)
    lv["digest"] = []
    for k in LEVELS:
        km, call, r = timed(A, lambda: A.digest_device(dig, k))
        assert r["records"] == K and r["bytes"] == cnt["bytes"], r
        d_ms = sum(km.get(x, 0.0) for x in DIGEST_KERNELS)
        lv["digest"].append(dict(log2_parts=k, path="lds" if k <= 12 else "global_adds",
                                 kernels_ms=km, digest_kernels_ms=d_ms, call_ms=call,
                                 over_count=d_ms / count_ms, over_full_sweep=d_ms / sweep_ms))
        print(json.dumps(lv["digest"][-1]), flush=True)
    d12 = next(x for x in lv["digest"] if x["log2_parts"] == 12)
    d13 = next(x for x in lv["digest"] if x["log2_parts"] == 13)
    lv["digest_k12_below_full_sweep"] = d12["digest_kernels_ms"] < sweep_ms
    lv["global_adds_over_lds"] = d13["digest_kernels_ms"] / d12["digest_kernels_ms"]
    res["levels"] = lv

    # ---- reconcile ----
    B = table(2)
    dig_b = torch.empty_like(dig)
    gen = torch.Generator(device=dev).manual_seed(11)
    raised = [0]

    def raise_on_b(D):
        """D buckets of B get a higher elapsed (a merge only B has seen)."""
        raised[0] += 1
        ids = torch.randperm(K, device=dev, generator=gen)[:D].sort().values
        nb, no = bench.names_for_ids(torch, ids)
        a = torch.full((D,), 0x4024000000000000, dtype=torch.int64, device=dev)
        t = torch.full((D,), 0x4008000000000000, dtype=torch.int64, device=dev)
        e = ids + (K + raised[0])                   # above every elapsed either side holds
        status = torch.zeros(D, dtype=torch.uint8, device=dev)
        B.receive_soa(nb, a, t, e, T0 + raised[0], name_offs=no, n=D, status=status, device=True)
        assert bool((status == 1).all())

    def digests(k):
        sa, sb = A.digest_device(dig, k), B.digest_device(dig_b, k)
        n = 1 << k
        ha, hb = dig[:n].cpu().numpy().view(np.uint64), dig_b[:n].cpu().numpy().view(np.uint64)
        return (ha[:, 0], ha[:, 1]), (hb[:, 0], hb[:, 1]), sa, sb

    def sweep_into(src, dst, parts, now):
        cursor, sent = None, 0
        while True:
            n, cursor, s = src.export_sweep_device(out, offs, cursor, args.chunk, parts=parts)
            if n:
                assert dst.receive_datagrams_device(out, offs, n, now) == n
            sent += n
            if s["done"]:
                return sent

    def one_round(D, k):
        raise_on_b(D)
        for r in (A, B):
            r.set_timing(True, accumulate=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        da, db, _, _ = digests(k)
        mask, nd = patrol_amd.digest_diff(da, db)
        sent = sweep_into(A, B, (k, mask), T0 + 10**6) + sweep_into(B, A, (k, mask), T0 + 10**6)
        b.record(stream)
        b.synchronize()
        ka, kbb = kernels(A), kernels(B)
        both = {x: ka.get(x, 0.0) + kbb.get(x, 0.0) for x in set(ka) | set(kbb)}
        dg = sum(both.get(x, 0.0) for x in DIGEST_KERNELS)
        sw = sum(both.get(x, 0.0) for x in SWEEP_KERNELS)
        rest = sum(v for x, v in both.items() if x not in DIGEST_KERNELS + SWEEP_KERNELS)
        fa, fb, sa, sb = digests(20)
        ok = bool((fa[0] == fb[0]).all() and (fa[1] == fb[1]).all() and sa == sb)
        return dict(parts_differing=nd, datagrams_sent=sent, digest_kernels_ms=dg,
                    sweep_kernels_ms=sw, receive_kernels_ms=rest, round_ms=a.elapsed_time(b),
                    verified=ok)

    rows = []
    one_round(100, 12)                              # warm both handles' buffers
    for D in (100, 10_000, 1_000_000):
        for k in (12, 16, 20):
            rs = [one_round(D, k) for _ in range(args.round_reps)]
            row = dict(D=D, log2_parts=k, parts=1 << k, verified=all(r["verified"] for r in rs),
                       every_partition_differs=all(r["parts_differing"] == 1 << k for r in rs))
            for key in ("parts_differing", "datagrams_sent", "digest_kernels_ms",
                        "sweep_kernels_ms", "receive_kernels_ms", "round_ms"):
                row[key] = med([r[key] for r in rs])
            row["digest_plus_sweep_kernels_ms"] = row["digest_kernels_ms"] + row["sweep_kernels_ms"]
            # beside it: what pushing everything costs, both ways
            row["full_sweeps_kernels_ms"] = 2 * sweep_ms
            row["full_sweeps_datagrams"] = 2 * K
            rows.append(row)
            print(json.dumps(row), flush=True)
    res["reconcile"] = rows
    A.close()
    B.close()

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
        res.update({k: v for k, v in old.items() if k not in res and k not in ("levels", "reconcile")})
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=res["build_id"],
                          digest_k12_below_full_sweep=lv["digest_k12_below_full_sweep"],
                          verified=all(r["verified"] for r in rows))))


if __name__ == "__main__":
    main()
