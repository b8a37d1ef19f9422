#!/usr/bin/env python3
"""Export sweep timings (not the bench): phip_export_sweep on C2's table, 10M
buckets in 2^25 slots with b"b%d" names, and the variant with 10 % of the
names 32 bytes long (the arena path).  One process; for the same table:

  count            PHIP_SWEEP_COUNT over the whole table
  sweep_one_call   a device-pointer sweep of everything in one call
  sweep_2p20       the same sweep in calls of 2^20 messages
  sweep_half_idle  one call with half the buckets filtered as idle
  evict_dry_run    phip_evict_idle(PHIP_EVICT_DRY_RUN), the count pass the
                   sweep's cost is judged against
  dump             phip_dump (device gather + copy + the host decode loop)

Kernel times are phip_last_timings (HIP events around each launch), summed
over a sweep's calls; call_ms is a HIP event pair on the handle's stream
around the whole loop, host round trips included.  Medians of --reps after
--warmup.  phip_dump is timed on the host clock (most of it is a host loop)
over --dump-reps runs.

The table is opened at 2^20 slots with max_load_pct 45 and grows to 2^25 when
the 10M buckets are seeded (load 0.30, as C2's and tools/evict_bench.py's).

Writes profiles/export_sweep_bench.json (--out) with the library's build id.
"""
import argparse
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
NOW = T0 + 1000 * SEC
IDLE_NS = 500 * SEC
SWEEP_KERNELS = ("k_sweep_count", "k_sweep_scan", "k_sweep_write")


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
    p.add_argument("--dump-reps", type=int, default=3)
    p.add_argument("--chunk", type=int, default=1 << 20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_sweep_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    K, L = args.buckets, args.log2_slots
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    res = dict(tool="tools/export_sweep_bench.py", build_id=_lib.build_id(), buckets=K,
               log2_slots=L, max_load_pct=pct, reps=args.reps, warmup=args.warmup,
               dump_reps=args.dump_reps, chunk=args.chunk, device=torch.cuda.get_device_name(0),
               configs=[])
    total = args.warmup + args.reps
    for long_frac in (0.0, 0.1):
        kb, ko = make_names(torch, K, long_frac, dev)
        # states: added 10.0, taken 3.0, elapsed = id; a random half created long ago (idle at NOW)
        st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
        st[:, 0] = 0x4024000000000000
        st[:, 1] = 0x4008000000000000
        st[:, 2] = torch.arange(K, dtype=torch.int64, device=dev)
        perm = torch.randperm(K, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        st[:, 3] = NOW
        st[perm[:K // 2], 3] = T0
        repo = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct)
        repo.use_torch_stream()
        repo.seed_device(kb, ko, st, K)
        assert len(repo) == K and repo.capacity == 1 << L
        del kb, ko, st, perm
        repo.set_timing(True, accumulate=True)
        cfg = dict(long_name_frac=long_frac)

        def timed(fn):
            """-> (per-kernel medians, median event ms of the whole loop, last result)."""
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

        # count mode
        km, call, cnt = timed(lambda: repo.sweep_count())
        assert cnt["n"] == K, cnt
        cfg["count"] = dict(kernels_ms=km, call_ms=call, n=cnt["n"], bytes=cnt["bytes"])
        cap = (cnt["bytes"] + 8 + 7) // 8 * 8
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        offs = torch.empty(K + 1, dtype=torch.int64, device=dev)

        def sweep(max_msgs, idle_ns=0):
            cursor, n, calls = None, 0, 0
            while True:
                k, cursor, s = repo.export_sweep_device(out, offs, cursor, max_msgs, NOW, idle_ns)
                n += k
                calls += 1
                if s["done"]:
                    return dict(n=n, calls=calls, last_bytes=s["bytes"])

        def sweep_cfg(max_msgs, idle_ns=0):
            km, call, r = timed(lambda: sweep(max_msgs, idle_ns))
            return dict(kernels_ms=km, sweep_kernels_ms=sum(km.get(k, 0.0) for k in SWEEP_KERNELS),
                        call_ms=call, **r)

        cfg["sweep_one_call"] = sweep_cfg(K)
        assert cfg["sweep_one_call"]["n"] == K and cfg["sweep_one_call"]["calls"] == 1
        assert cfg["sweep_one_call"]["last_bytes"] == cnt["bytes"]
        cfg["sweep_2p20"] = sweep_cfg(args.chunk)
        assert cfg["sweep_2p20"]["n"] == K
        cfg["sweep_half_idle"] = sweep_cfg(K, IDLE_NS)
        assert cfg["sweep_half_idle"]["n"] == K - K // 2
        km, call, r = timed(lambda: repo.evict_idle(NOW, IDLE_NS, dry_run=True))
        assert r["idle"] == K // 2 and r["evicted"] == 0
        cfg["evict_dry_run"] = dict(kernels_ms=km, call_ms=call)
        dry = km["k_evict_count"]
        cfg["ratios"] = dict(
            one_call_over_dry_run=cfg["sweep_one_call"]["sweep_kernels_ms"] / dry,
            chunked_over_dry_run=cfg["sweep_2p20"]["sweep_kernels_ms"] / dry,
            count_over_dry_run=cfg["count"]["kernels_ms"]["k_sweep_count"] / dry)
        del out, offs
        repo.set_timing(False)
        ts = []
        for _ in range(1 + args.dump_reps):
            t = time.perf_counter()
            d = repo.dump_arrays()
            ts.append((time.perf_counter() - t) * 1e3)
            assert len(d[1]) == K + 1
            del d
        cfg["dump"] = dict(host_clock_ms=med(ts[1:]), reps=args.dump_reps)
        cfg["ratios"]["dump_over_one_call"] = cfg["dump"]["host_clock_ms"] / cfg["sweep_one_call"]["call_ms"]
        repo.close()
        res["configs"].append(cfg)
        print(json.dumps(cfg), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=res["build_id"],
                          ratios=[c["ratios"] for c in res["configs"]])))


if __name__ == "__main__":
    main()
