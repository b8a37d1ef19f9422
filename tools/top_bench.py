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

In the same run, alternating with the rows above:
  metric 1   PHIP_TOP_SINCE_MARK beside metric 0 on the same table, after a
             usage mark and a batch that raises 1% of the buckets (every 100th
             id: by distinct amounts on zipf, by one amount on equal, so that
             table's window is one tie group of 100k);
  mark       phip_usage_mark (k_usage_mark) beside the count pass, once per
             table;
  parent     metric 0 on the parent commit's library (--parent-lib, by default
             tools/var/libpatrolhip_parent.so; missing: not measured), over a
             table seeded the same way: the bar for "metric 0 did not move" is
             the parent's own min-to-max spread.

Writes profiles/top_bench.json (--out) with the library's build id.
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
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "var", "libpatrolhip_parent.so"),
                   help="the parent commit's libpatrolhip.so ('' or missing: not measured)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_bench.json"))
    args = p.parse_args()
    import numpy as np
    import torch
    import patrol_amd
    from patrol_amd import _lib
    from patrol_amd.engine import GPURepo, phip_config
    dev = torch.device("cuda", 0)
    K, L, W, R = args.buckets, args.log2_slots, args.warmup, args.reps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    res = dict(tool="tools/top_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               reps=R, warmup=W, prefix=PREFIX.decode(), device=torch.cuda.get_device_name(0),
               tables=[])
    n_prefix = sum(1 for i in range(K) if str(i).startswith(PREFIX[1:].decode()))
    # the window's activity: every 100th id
    RAISE0, RAISE_STEP = 37, 100
    n_raised = len(range(RAISE0, K, RAISE_STEP))
    n_raised_prefix = sum(1 for i in range(RAISE0, K, RAISE_STEP)
                          if str(i).startswith(PREFIX[1:].decode()))
    Lp = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        cur, _lib._lib = _lib._lib, None
        try:
            Lp = _lib.load(args.parent_lib)
        finally:
            _lib._lib = cur
        res["parent_build_id"] = Lp.phip_build_id().decode()
        assert res["parent_build_id"] != res["build_id"], "--parent-lib is this build"

    def open_parent():
        r = GPURepo.__new__(GPURepo)
        r.L, r.device, r.owned = Lp, 0, True
        cfg = phip_config(0, L, 1 << 20, 90, 0, 0, 0, 0)
        h = C.c_void_p()
        assert Lp.phip_open(C.byref(cfg), C.byref(h)) == 0
        r.h = h
        r._queued = None
        return r

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
        repo = patrol_amd.GPURepo(device=0, log2_slots=L, arena_bytes=1 << 20, max_load_pct=90,
                                  track_usage=True)
        repos = [repo] + ([open_parent()] if Lp else [])
        for r in repos:
            r.use_torch_stream()
            r.seed_device(kb, ko, st, K)
            assert len(r) == K and r.capacity == 1 << L
        parent = repos[1] if Lp else None
        # the window: a mark, then 1% of the buckets raised (seed overwrites a state)
        mk = repo.usage_mark()
        assert mk == dict(buckets=K, active=K), mk
        ids = torch.arange(RAISE0, K, RAISE_STEP, dtype=torch.int64, device=dev)
        if table == "zipf":
            g2 = torch.Generator(device=dev)
            g2.manual_seed(6)
            up = 1e6 / (torch.randperm(n_raised, device=dev, generator=g2).double() + 1.0)
        else:
            up = torch.full((n_raised,), 5.0, dtype=torch.float64, device=dev)
        raised = taken[ids] + up
        want16_m1 = [int(x) for x in torch.sort((raised - taken[ids]).view(torch.int64),
                                                descending=True)[0][:16].cpu()]
        taken[ids] = raised
        want16 = [int(x) for x in torch.sort(taken.view(torch.int64), descending=True)[0][:16].cpu()]
        rb, ro = bench.names_for_ids(torch, ids)
        rs = st[ids].contiguous()
        rs[:, 0] = (raised + 10.0).view(torch.int64)
        rs[:, 1] = raised.view(torch.int64)
        for r in repos:
            r.seed_device(rb, ro, rs, n_raised)
            assert len(r) == K
        del kb, ko, st, taken, rb, ro, rs, raised, up, ids
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
                    fn, on = fn if isinstance(fn, tuple) else (fn, repo)
                    on.set_timing(True, accumulate=True)   # (drops what came before)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    last[i] = fn()
                    b.record(stream)
                    b.synchronize()
                    calls[i].append(a.elapsed_time(b))
                    ks[i].append(kernels(on))
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
            pop1 = n_raised if not prefix else n_raised_prefix
            for k in KS:
                fns = [
                    lambda: repo.top_device(k, names, offs, tk, sta, prefix),
                    lambda: {f: v for f, v in repo.top(k, prefix, state=True).items()
                             if f in ("n", "population", "passes", "truncated")},
                    lambda: repo.sweep_count(),
                    lambda: repo.top_device(k, names, offs, tk, sta, prefix, metric=1)]
                if parent:
                    fns.append((lambda: parent.top_device(k, names, offs, tk, sta, prefix), parent))
                out = timed(fns)
                dv, hs, cn, m1 = out[:4]
                assert dv[3]["n"] == hs[3]["n"] == min(k, pop), (dv[3], hs[3])
                assert dv[3]["population"] == pop and cn[3]["n"] == K
                assert m1[3]["n"] == min(k, pop1) and m1[3]["population"] == pop1, m1[3]
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
                case["metric1"] = dict(
                    population=pop1, passes=m1[3]["passes"], kernels_ms=m1[0],
                    kernels_sum_ms=med(m1[1]), kernels_sum_min_max_ms=[min(m1[1]), max(m1[1])],
                    device_call_ms=med(m1[2]), device_call_min_max_ms=[min(m1[2]), max(m1[2])],
                    # per table pass: the two metrics stop their refinement at different depths
                    kernels_per_pass_over_metric0=(med(m1[1]) / m1[3]["passes"]) /
                    (med(dv[1]) / dv[3]["passes"]))
                if parent:
                    pr = out[4]
                    assert pr[3]["n"] == dv[3]["n"] and pr[3]["passes"] == dv[3]["passes"]
                    case["parent_metric0"] = dict(
                        kernels_ms=pr[0], kernels_sum_ms=med(pr[1]),
                        kernels_sum_min_max_ms=[min(pr[1]), max(pr[1])],
                        device_call_ms=med(pr[2]), device_call_min_max_ms=[min(pr[2]), max(pr[2])],
                        kernels_over_parent=med(dv[1]) / med(pr[1]),
                        device_call_over_parent=med(dv[2]) / med(pr[2]),
                        kernels_median_inside_parent_spread=min(pr[1]) <= med(dv[1]) <= max(pr[1]))
                cfg["cases"].append(case)
                print(json.dumps(case), flush=True)
        # the list itself, once
        torch.cuda.synchronize()
        d = repo.top(16)
        assert d["n"] == 16 and [int(x) for x in d["taken"]] == want16, (d["taken"], want16)
        if table == "zipf":
            assert len(set(want16)) == 16 and d["names"] == repo.top(4096)["names"][:16]
        d = repo.top(16, metric=1)
        assert d["n"] == 16 and [int(x) for x in d["taken"]] == want16_m1, (d["taken"], want16_m1)
        # the mark beside the count pass (the first of them ends the window)
        um, cn = timed([lambda: repo.usage_mark(), lambda: repo.sweep_count()])
        assert um[3]["buckets"] == K and um[3]["active"] == 0 and cn[3]["n"] == K
        assert repo.top_count(metric=1)["population"] == 0
        cfg["usage_mark"] = dict(
            kernel_ms=med(um[1]), kernel_min_max_ms=[min(um[1]), max(um[1])],
            call_ms=med(um[2]), call_min_max_ms=[min(um[2]), max(um[2])],
            count_pass_ms=med(cn[1]), count_pass_min_max_ms=[min(cn[1]), max(cn[1])],
            kernel_over_count_pass=med(um[1]) / med(cn[1]))
        print(json.dumps(cfg["usage_mark"]), flush=True)
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
        for r in repos:
            r.close()
        res["tables"].append(cfg)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=res["build_id"])))


if __name__ == "__main__":
    main()
