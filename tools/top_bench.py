#!/usr/bin/env python3
"""What the top-talkers select costs (not the bench): phip_export_top beside
the whole-table count pass (sweep_count's k_sweep_count), alternating in the
same run, on one build.

The table: 10M buckets b"b%d" in 2^24 slots.  Seeded twice:
  zipf   taken = 1e9 / rank over a random permutation of the buckets, so the
         top keys are distinct and spread over many exponents;
  equal  every bucket holds the same taken: the worst case, every digit pass,
         the tie count and the collect.
Per table: k in {16, 1024, 4096}, with no prefix and with b"b12" (1.1% of the
names), from device pointers and from host pointers.  Per case: passes, the
select's kernels (HIP events around each launch, phip_last_timings) and the
whole call (HIP events on the stream), the ratio of the kernels to one count
pass, and the spread (min / max over --reps after --warmup; the figures
themselves are medians).  Once per table: the host route the call replaces,
phip_dump plus a numpy partial sort of the taken column.

Writes profiles/top_bench.json (--out) with the library's build id.
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

T0 = bench.T0
PREFIX = b"b12"
KS = (16, 1024, 4096)


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
    p.add_argument("--log2-slots", type=int, default=24)
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    K, L, W, R = args.buckets, args.log2_slots, args.warmup, args.reps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    res = dict(tool="tools/top_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               reps=R, warmup=W, prefix=PREFIX.decode(), device=torch.cuda.get_device_name(0),
               tables=[])
    n_prefix = sum(1 for i in range(K) if str(i).startswith(PREFIX[1:].decode()))

    for table in ("zipf", "equal"):
        kb, ko = make_names(torch, K, 0.0, dev)
        st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
        if table == "zipf":
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            rank = torch.randperm(K, device=dev, generator=g).double() + 1.0
            taken = 1e9 / rank
        else:
            taken = torch.full((K,), 7.0, dtype=torch.float64, device=dev)
        want16 = [int(x) for x in torch.sort(taken.view(torch.int64), descending=True)[0][:16].cpu()]
        st[:, 0] = (taken + 10.0).view(torch.int64)
        st[:, 1] = taken.view(torch.int64)
        st[:, 2] = 1
        st[:, 3] = T0
        repo = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20, max_load_pct=90)
        repo.use_torch_stream()
        repo.seed_device(kb, ko, st, K)
        assert len(repo) == K and repo.capacity == 1 << L
        del kb, ko, st, taken
        names = torch.empty(_lib.MAX_NAME_LEN * max(KS), dtype=torch.uint8, device=dev)
        offs = torch.empty(max(KS) + 1, dtype=torch.int64, device=dev)
        tk = torch.empty(max(KS), dtype=torch.int64, device=dev)
        sta = torch.empty((max(KS), 4), dtype=torch.int64, device=dev)

        def timed(fns):
            """The callables in turn, W + R rounds -> per callable (per-kernel
            medians, the kernel sums of every rep, the call ms of every rep,
            the last result)."""
            ks = [[] for _ in fns]
            calls = [[] for _ in fns]
            last = [None] * len(fns)
            for _ in range(W + R):
                for i, fn in enumerate(fns):
                    repo.set_timing(True, accumulate=True)   # (drops what came before)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    last[i] = fn()
                    b.record(stream)
                    b.synchronize()
                    calls[i].append(a.elapsed_time(b))
                    ks[i].append(kernels(repo))
            out = []
            for i in range(len(fns)):
                k = ks[i][W:]
                nms = sorted({n for d in k for n in d})
                out.append(({n: med([d.get(n, 0.0) for d in k]) for n in nms},
                            [sum(d.values()) for d in k], calls[i][W:], last[i]))
            return out

        cfg = dict(table=table, cases=[])
        for prefix in (b"", PREFIX):
            pop = K if not prefix else n_prefix
            for k in KS:
                dv, hs, cn = timed([
                    lambda: repo.top_device(k, names, offs, tk, sta, prefix),
                    lambda: {f: v for f, v in repo.top(k, prefix, state=True).items()
                             if f in ("n", "population", "passes", "truncated")},
                    lambda: repo.sweep_count()])
                assert dv[3]["n"] == hs[3]["n"] == min(k, pop), (dv[3], hs[3])
                assert dv[3]["population"] == pop and cn[3]["n"] == K
                count_ms = med(cn[1])
                case = dict(
                    k=k, prefix=prefix.decode(), population=pop, passes=dv[3]["passes"],
                    kernels_ms=dv[0], kernels_sum_ms=med(dv[1]),
                    kernels_sum_min_max_ms=[min(dv[1]), max(dv[1])],
                    device_call_ms=med(dv[2]), device_call_min_max_ms=[min(dv[2]), max(dv[2])],
                    host_call_ms=med(hs[2]), host_call_min_max_ms=[min(hs[2]), max(hs[2])],
                    count_pass_ms=count_ms, count_pass_min_max_ms=[min(cn[1]), max(cn[1])],
                    kernels_over_count_pass=med(dv[1]) / count_ms,
                    device_call_over_count_pass=med(dv[2]) / count_ms)
                cfg["cases"].append(case)
                print(json.dumps(case), flush=True)
        # the list itself, once
        torch.cuda.synchronize()
        d = repo.top(16)
        assert d["n"] == 16 and [int(x) for x in d["taken"]] == want16, (d["taken"], want16)
        if table == "zipf":
            assert len(set(want16)) == 16 and d["names"] == repo.top(4096)["names"][:16]
        # the host route, once: the whole table to the host, a partial sort there
        t0 = time.perf_counter()
        _, _, _, t_col, _, _ = repo.dump_arrays()
        t1 = time.perf_counter()
        keys = t_col.view(np.int64)
        top = np.argpartition(keys, len(keys) - 4096)[-4096:]
        top = top[np.argsort(-keys[top], kind="stable")]
        t2 = time.perf_counter()
        cfg["host_route"] = dict(dump_ms=(t1 - t0) * 1e3, partial_sort_ms=(t2 - t1) * 1e3,
                                 total_ms=(t2 - t0) * 1e3, k=4096)
        print(json.dumps(cfg["host_route"]), flush=True)
        del t_col, keys, top, names, offs, tk, sta
        repo.close()
        res["tables"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=res["build_id"])))


if __name__ == "__main__":
    main()
