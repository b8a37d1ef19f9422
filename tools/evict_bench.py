#!/usr/bin/env python3
"""Eviction sweep timings (not the bench): phip_evict_idle on C2's table,
10M buckets in 2^25 slots, with 0 %, 50 % and 99 % of the buckets idle, with
and without PHIP_EVICT_SHRINK, and with 10 % of the names 32 bytes long (the
arena path).  Per-kernel times come from phip_last_timings (HIP events).

Beside them, in the same process and on the same table, the two closest
kernels the library already had:
  k_table_stats  one streaming read of all slots      vs k_evict_count
  k_rehash       the 2^24 -> 2^25 growth, 9.8M records vs k_evict_move at 0 % idle

The table is opened at 2^20 slots with max_load_pct 45 and grows to 2^25
when the 10M buckets are seeded (load 0.30, as C2's), so that shrinking has
somewhere to go.  "0 % idle" is one idle bucket of the 10M: with none the
call returns after the count pass and there is no move to time (the count
pass with none idle is timed too).  Every figure is the median of --reps
runs after --warmup; between two runs the evicted buckets are seeded back.

Writes profiles/evict_bench.json (--out) with the library's build id.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SEC = 10**9
T0 = bench.T0
NOW = T0 + 1000 * SEC
IDLE_NS = 500 * SEC


def make_names(torch, K, long_frac, dev):
    """K distinct names: ids below K * long_frac are 32 bytes, the rest b"b%d"."""
    nl = int(K * long_frac)
    ids = torch.arange(K, dtype=torch.int64, device=dev)
    sb, so = bench.names_for_ids(torch, ids[nl:])
    if not nl:
        return sb, so
    lb, lo = bench.padded_names(torch, ids[:nl], 32)
    blob = torch.cat([lb[:nl * 32], sb])
    offs = torch.cat([lo[:-1], so + nl * 32])
    return blob, offs.to(torch.int32)


def med(xs):
    return float(statistics.median(xs)) if xs else None


def kernel_ms(repo, name):
    return sum(ms for nm, ms in repo.timings() if nm == name)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="the table the buckets end up in")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "evict_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    dev = torch.device("cuda", 0)
    K, L = args.buckets, args.log2_slots
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    # the load limit that makes K buckets end up in 2^L slots when the table grows
    pct = 45
    assert (1 << (L - 1)) * pct // 100 < K <= (1 << L) * pct // 100, "pick --log2-slots for --buckets"
    out = dict(tool="tools/evict_bench.py", build_id=_lib.build_id(), buckets=K, log2_slots=L,
               max_load_pct=pct, reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), configs=[])
    total = args.warmup + args.reps
    ref = {}
    for long_frac in (0.0, 0.1):
        kb, ko = make_names(torch, K, long_frac, dev)
        st = torch.zeros((K, 4), dtype=torch.int64, device=dev)
        repo = patrol_amd.GPURepo(device=0, log2_slots=20, arena_bytes=1 << 20, max_load_pct=pct)
        repo.use_torch_stream()
        repo.set_timing(True)
        for idle_frac in (0.0, 0.5, 0.99):
            # a random subset is idle (ids are hashed anyway): created long ago
            n_idle = max(1, int(K * idle_frac))
            perm = torch.randperm(K, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
            st[:, 3] = NOW
            st[perm[:n_idle], 3] = T0
            torch.cuda.synchronize()
            for shrink in (False, True):
                cnt, mov, slots = [], [], None
                for _ in range(total):
                    repo.seed_device(kb, ko, st, K)       # every bucket back, states as given
                    assert len(repo) == K and repo.capacity == 1 << L
                    r = repo.evict_idle(NOW, IDLE_NS, shrink=shrink)
                    assert r["evicted"] == n_idle and r["buckets"] == K - n_idle, r
                    cnt.append(kernel_ms(repo, "k_evict_count"))
                    mov.append(kernel_ms(repo, "k_evict_move"))
                    slots = r["slots"]
                out["configs"].append(dict(
                    long_name_frac=long_frac, idle_frac=idle_frac, idle=n_idle, shrink=shrink,
                    slots_after=slots, arena_used_after=r["arena_used"],
                    arena_freed=r["arena_freed"],
                    k_evict_count_ms=med(cnt[args.warmup:]), k_evict_move_ms=med(mov[args.warmup:])))
                print(json.dumps(out["configs"][-1]), flush=True)
        # the reference kernels and the count-only call, on the same table
        st[:, 3] = NOW
        repo.seed_device(kb, ko, st, K)
        ts, c0 = [], []
        for _ in range(total):
            repo.table_stats()
            ts.append(kernel_ms(repo, "k_table_stats"))
            r = repo.evict_idle(NOW, IDLE_NS)
            assert r["idle"] == 0 and r["evicted"] == 0
            c0.append(kernel_ms(repo, "k_evict_count"))
        ref[long_frac] = dict(k_table_stats_ms=med(ts[args.warmup:]),
                              k_evict_count_none_idle_ms=med(c0[args.warmup:]))
        repo.close()
        # k_rehash: 2^(L-1) -> 2^L with all but 2 % of the buckets in the table
        first = K - K // 50
        pct_g = 59
        assert first <= (1 << (L - 1)) * pct_g // 100 < K <= (1 << L) * pct_g // 100
        offs64 = ko.to(torch.int64)
        cut = int(offs64[first])
        kb2, ko2 = kb[cut:].contiguous(), (offs64[first:] - cut).to(torch.int32)
        rh = []
        for _ in range(total):
            g = patrol_amd.GPURepo(device=0, log2_slots=L - 1, arena_bytes=1 << 26, max_load_pct=pct_g)
            g.use_torch_stream()
            g.seed_device(kb, ko, st, first)
            assert g.capacity == 1 << (L - 1)
            g.set_timing(True)
            g.seed_device(kb2, ko2, st[first:].contiguous(), K - first)
            rh.append(kernel_ms(g, "k_rehash"))
            assert g.capacity == 1 << L and len(g) == K and rh[-1] > 0
            g.close()
        ref[long_frac]["k_rehash_ms"] = med(rh[args.warmup:])
        ref[long_frac]["k_rehash_records"] = first
        print(json.dumps(ref[long_frac]), flush=True)
        del kb, ko, st, kb2, ko2
    out["reference"] = {str(k): v for k, v in ref.items()}
    ratios = {}
    for c in out["configs"]:
        if c["idle_frac"] == 0.0 and not c["shrink"]:
            r = ref[c["long_name_frac"]]
            ratios[str(c["long_name_frac"])] = dict(
                count_over_table_stats=c["k_evict_count_ms"] / r["k_table_stats_ms"],
                move_over_rehash=c["k_evict_move_ms"] / r["k_rehash_ms"])
    out["ratios"] = ratios
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, ratios=ratios, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
