#!/usr/bin/env python3
"""What the throttled sweep costs (not the bench): phip_export_throttled beside
the export sweep over the same table, alternating in the same run, on one build.

The table is C2's: 10M buckets b"b%d" in 2^25 slots (opened at 2^20 with
max_load_pct 45).  Every bucket's `last` is the reading the sweep is asked at
(dt = 0), a throttled one holds no token (added 10, taken 10: denied, with an
answer 10 ms later under 100:1s), the others 7.  Seeded twice: every 100th
bucket throttled (1%), every second (50%).

Per table, under one catch-all rule and again under 8 rules (seven prefixes no
name has in front of the catch-all, so every record walks all eight):
  (a) count mode:        k_throttle_count        beside sweep_count's k_sweep_count
  (b) one device call:   count + scan + write + retry  beside the one-call
      over the table     export_sweep_device's count + scan + write
  (c) calls of 2^16:     the same, a whole sweep in 2^16-entry calls

Kernel times are HIP events around each launch (phip_last_timings), whole
calls HIP events on the stream; the median of --reps after --warmup.  Writes
profiles/throttled_bench.json (--out) with the library's build id and the
throttled / export ratios.
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

SEC = 10**9
T0 = bench.T0
NOW = T0 + 10_000_000
SWEEP_KERNELS = ("k_sweep_count", "k_sweep_scan", "k_sweep_write")
THROTTLE_KERNELS = ("k_throttle_count", "k_sweep_scan", "k_throttle_write", "k_throttle_retry")
CATCH_ALL = (b"", 100, SEC, 1)


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
    p.add_argument("--chunk", type=int, default=1 << 16)
    p.add_argument("--every", type=int, nargs="*", default=[100, 2],
                   help="every n-th bucket is throttled, one table per value")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "throttled_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    K, L, W, R = args.buckets, args.log2_slots, args.warmup, args.reps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    res = dict(tool="tools/throttled_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               max_load_pct=pct, reps=R, warmup=W, chunk=args.chunk,
               device=torch.cuda.get_device_name(0), configs=[])
    rule_sets = {"1_rule": [CATCH_ALL],
                 "8_rules": [(b"no-such-%d:" % i, 3, SEC, 1) for i in range(7)] + [CATCH_ALL]}

    for every in args.every:
        kb, ko = make_names(torch, K, 0.0, dev)
        ids = torch.arange(K, dtype=torch.int64, device=dev)
        st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
        st[:, 0] = 0x4024000000000000                       # added 10.0
        st[:, 1] = 0x4008000000000000                       # taken 3.0
        st[ids % every == 0, 1] = 0x4024000000000000        # taken 10.0: no token left
        st[:, 2] = NOW - T0                                 # last = NOW: dt = 0
        st[:, 3] = T0
        want = (K + every - 1) // every
        repo = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct)
        repo.use_torch_stream()
        repo.seed_device(kb, ko, st, K)
        assert len(repo) == K and repo.capacity == 1 << L
        del kb, ko, st, ids
        cfg = dict(throttled_every=every, throttled=want)

        def timed(fns):
            """The callables in turn, W + R rounds -> per callable (per-kernel
            medians, median event ms of the call or loop, last result)."""
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
                names = sorted({n for d in k for n in d})
                out.append(({n: med([d.get(n, 0.0) for d in k]) for n in names}, med(calls[i][W:]),
                            last[i]))
            return out

        # the export sweep's buffers, and the throttled sweep's
        sc = repo.sweep_count()
        assert sc["n"] == K
        ex_out = torch.empty((sc["bytes"] + 8 + 7) // 8 * 8, dtype=torch.uint8, device=dev)
        ex_offs = torch.empty(K + 1, dtype=torch.int64, device=dev)
        cnt = repo.throttled_count([CATCH_ALL], NOW)
        assert cnt["n"] == want, (cnt, want)
        M = 1 << (L - 2)            # 4 * M slots: one call's window is the table
        assert want <= M
        names = torch.empty(cnt["bytes"] + _lib.MAX_NAME_LEN, dtype=torch.uint8, device=dev)
        offs = torch.empty(M + 1, dtype=torch.int64, device=dev)
        at, rem = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))
        rule = torch.empty(M, dtype=torch.uint8, device=dev)

        def export(max_msgs):
            cursor, n, calls = None, 0, 0
            while True:
                k, cursor, s = repo.export_sweep_device(ex_out, ex_offs, cursor, max_msgs, NOW, 0)
                n += k
                calls += 1
                if s["done"]:
                    return dict(n=n, calls=calls)

        def throttled(rules, max_entries):
            cursor, n, calls = None, 0, 0
            while True:
                k, cursor, s = repo.export_throttled_device(rules, NOW, names, offs, cursor,
                                                            max_entries, 0, at, rem, rule)
                n += k
                calls += 1
                if s["done"]:
                    return dict(n=n, calls=calls)

        def row(t, e):
            """One comparison: (kernels, call ms, result) of the throttled and export sides."""
            tk, ek = (sum(t[0].get(k, 0.0) for k in THROTTLE_KERNELS),
                      sum(e[0].get(k, 0.0) for k in SWEEP_KERNELS))
            return dict(throttled=dict(kernels_ms=t[0], kernels_sum_ms=tk, call_ms=t[1], **t[2]),
                        export=dict(kernels_ms=e[0], kernels_sum_ms=ek, call_ms=e[1], **e[2]),
                        kernels_ratio=tk / ek, call_ratio=t[1] / e[1])

        for label, rules in rule_sets.items():
            c = {}
            t, e = timed([lambda: dict(n=repo.throttled_count(rules, NOW)["n"]),
                          lambda: dict(n=repo.sweep_count()["n"])])
            assert t[2]["n"] == want and e[2]["n"] == K
            c["count"] = row(t, e)
            t, e = timed([lambda: throttled(rules, M), lambda: export(K)])
            assert t[2] == dict(n=want, calls=1) and e[2] == dict(n=K, calls=1)
            c["one_call"] = row(t, e)
            # (count mode against the full one-call export sweep)
            c["count_over_one_call_export"] = (c["count"]["throttled"]["kernels_sum_ms"] /
                                               c["one_call"]["export"]["kernels_sum_ms"])
            t, e = timed([lambda: throttled(rules, args.chunk), lambda: export(args.chunk)])
            assert t[2]["n"] == want and e[2]["n"] == K
            c["chunked"] = row(t, e)
            cfg[label] = c
            print(json.dumps({label: c}), flush=True)
        # the entries themselves, once: names b"b<id>", 10 ms to wait, nothing remaining
        k, _, s = repo.export_throttled_device([CATCH_ALL], NOW, names, offs, None, M, 0, at, rem, rule)
        torch.cuda.synchronize()
        assert k == want and bool((at[:k] == NOW + 10_000_000).all()) and bool((rem[:k] == 0).all())
        assert bool((rule[:k] == 0).all()) and int(offs[k]) == cnt["bytes"]
        del ex_out, ex_offs, names, offs, at, rem, rule
        repo.close()
        res["configs"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=res["build_id"])))


if __name__ == "__main__":
    main()
