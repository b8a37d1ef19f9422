#!/usr/bin/env python3
"""Group reply egress, timed (not the bench): 2^24 datagrams, Zipf 1.1 over 10M
names (b"b%d"), at world 1 over the RCCL self-exchange and over two shards on
one GPU (each member holding half of the batch), through

  (a)  phip_group_receive_datagrams;
  (a') the same call in the parent commit's library (--parent-lib, loaded
       beside the new one through _lib.load(path)), on a group of its own;
  (b)  phip_group_receive_datagrams_replies of a batch without a request;
  (c)  the same with 64 requests and (d) with 4096, to buckets of the batch;
  (e)  (c)'s batch decoded and sent through phip_group_apply_mixed as RECEIVE
       ops with all four result columns: the workaround the replies form
       replaces.

Every form has a twin group of its own; they alternate step by step in one
process, rotating which runs first, every step with fresh replica states.  A
call's time is a host clock around it ending in a device synchronise, with
phip_group_stage_ms (pack / exchange / merge) and phip_group_reply_stats beside
it; every figure is the median of --reps steps after --warmup, min and max as
the spread.  After the timed steps, --kernel-steps more run (b), (c), (d) with
the members' kernel timing on: the k_zero_count pass and the index-keeping
scatter (k_route_scatter_src) per call, from phip_last_timings.

Reads no oracle.  Writes profiles/group_replies_bench.json (--out) with the
libraries' build ids.
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


def stat(xs):
    return dict(ms=float(statistics.median(xs)), min_ms=float(min(xs)), max_ms=float(max(xs)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--messages", type=int, default=1 << 24)
    p.add_argument("--buckets", type=int, default=10_000_000)
    p.add_argument("--log2-slots", type=int, default=25, help="one table holding every bucket")
    p.add_argument("--reps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--kernel-steps", type=int, default=2)
    p.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "var", "libpatrolhip_parent.so"),
                   help="the parent commit's libpatrolhip.so ('' or missing: (a') is not measured)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_replies_bench.json"))
    args = p.parse_args()
    import torch
    import patrol_amd
    from patrol_amd import _lib
    from patrol_amd.engine import GPUGroup, phip_config, phip_ops, phip_results, phip_wire
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(17)
    n, K, L = args.messages, args.buckets, args.log2_slots
    total = args.warmup + args.reps
    _lib.load()
    out = dict(tool="tools/group_replies_bench.py", build_id=_lib.build_id(), messages=n, buckets=K,
               zipf=1.1, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    Lp = None
    if args.parent_lib and os.path.exists(args.parent_lib):
        cur, _lib._lib = _lib._lib, None
        try:
            Lp = _lib.load(args.parent_lib)
        finally:
            _lib._lib = cur
        out["parent_build_id"] = Lp.phip_build_id().decode()
        assert out["parent_build_id"] != out["build_id"], "--parent-lib is this build"

    ids = bench.zipf_ids(torch, gen, n, K, 1.1, dev)
    blob, offs = bench.names_for_ids(torch, ids)
    del ids
    REQ = dict(b=0, c=64, d=4096)

    def open_parent(devices, log2):
        cfg = phip_config(0, log2, 1 << 20, 90, 0, 0, 0, 0)
        devs = (C.c_int32 * len(devices))(*devices)
        g = C.c_void_p()
        assert Lp.phip_group_open_all(C.byref(cfg), devs, len(devices), C.byref(g)) == 0
        return GPUGroup(g, Lp, [])

    for key, devices, log2 in (("group_world1_rccl_self", [0], L), ("group_shared_world2", [0, 0], L - 1)):
        Wg = len(devices)
        kw = dict(combine=True, rccl_self=Wg == 1, checked=False)
        forms = ["a", "b", "c", "d", "e"] + (["parent_a"] if Lp is not None else [])
        G = {f: (open_parent(devices, log2) if f == "parent_a" else
                 patrol_amd.GPUGroup.open_all(devices, log2_slots=log2, arena_bytes=1 << 20)) for f in forms}
        for g in G.values():
            g.set_timing(True)
        cut = [n * i // Wg for i in range(Wg + 1)]
        per = [cut[i + 1] - cut[i] for i in range(Wg)]
        caps = dict(max_msgs=8192)
        flags = _lib.DEVICE_PTRS | _lib.ROUTE_COMBINE | (_lib.GROUP_RCCL_SELF if Wg == 1 else 0)
        # every form through the C ABI with buffers allocated before the clock starts
        rqs = {f: G[f]._group_rq(caps) for f in REQ}
        # (e)'s columns, allocated once: kind, now and the four result columns
        kind = torch.full((n,), _lib.OP_RECEIVE, dtype=torch.uint8, device=dev)
        res_cols = [(torch.zeros(m, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.int64, device=dev),
                     torch.zeros(m, dtype=torch.int64, device=dev),
                     torch.zeros((m, 4), dtype=torch.int64, device=dev)) for m in per]
        ms = {f: [] for f in forms}
        stg = {f: [] for f in forms}
        rstats, counts = {}, {}

        def run(f, j, wire, dec):
            g = G[f]
            now = bench.T0 + j
            sv, mv, stv = (C.c_uint64 * Wg)(), (C.c_uint64 * Wg)(), (C.c_uint32 * Wg)()
            ws = (phip_wire * Wg)()
            for i, (data, do) in enumerate(wire["b" if f in ("a", "parent_a") else f if f in REQ else "c"]):
                ws[i] = phip_wire(do.numel() - 1, 0, data.data_ptr(), do.data_ptr(), 0)
            t0 = time.perf_counter()
            if f in ("a", "parent_a"):
                g._check(g.L.phip_group_receive_datagrams(g.g, ws, now, sv, mv, stv, flags))
                s, m = list(sv), list(mv)
            elif f == "e":
                a, t, e = dec
                nowc = torch.full((n,), now, dtype=torch.int64, device=dev)
                ops = (phip_ops * Wg)()
                res = (phip_results * Wg)()
                for i in range(Wg):
                    lo, hi = cut[i], cut[i + 1]
                    ops[i] = phip_ops(hi - lo, 0, kind[lo:hi].data_ptr(), blob.data_ptr(),
                                      offs[lo:hi + 1].data_ptr(), nowc[lo:hi].data_ptr(), None, None, None,
                                      a[lo:hi].data_ptr(), t[lo:hi].data_ptr(), e[lo:hi].data_ptr())
                    res[i] = phip_results(*[x.data_ptr() for x in res_cols[i]])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sv, av = (C.c_uint64 * Wg)(), (C.c_uint64 * Wg)()
                g._check(g.L.phip_group_apply_mixed(g.g, ops, res, sv, av, _lib.DEVICE_PTRS |
                                                    (_lib.GROUP_RCCL_SELF if Wg == 1 else 0)))
                s, m = list(sv), list(av)
            else:
                rq = rqs[f][0]
                g._check(g.L.phip_group_receive_datagrams_replies(g.g, ws, now, sv, mv, stv, rq, flags))
                s, m = list(sv), list(mv)
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) * 1e3)
            if f in REQ:
                counts[f] = dict(n=[int(q.n) for q in rq], replies=[int(q.replies) for q in rq])
                rstats[f] = [g.reply_stats(i) for i in range(Wg)]
            stg[f].append([g.stage_ms(i) for i in range(Wg)])
            assert sum(s) == sum(m)

        def step_inputs(j):
            """Fresh states; the clean batch and the ones with 64 / 4096 requests
            (zero states at random places of each member's part) as datagrams,
            and (c)'s batch decoded for (e)."""
            a, t, e = bench.replica_states(torch, gen, n, j, dev)
            wire, dec = {}, None
            for f, r in REQ.items():
                a2, t2, e2 = a.clone(), t.clone(), e.clone()
                if r:
                    at = torch.cat([torch.randperm(per[i], device=dev, generator=gen)[:r // Wg] + cut[i]
                                    for i in range(Wg)])
                    a2[at], t2[at], e2[at] = 0, 0, 0
                data, doffs = bench.datagrams(torch, blob, offs, a2, t2, e2)
                wire[f] = [(data, doffs[cut[i]:cut[i + 1] + 1]) for i in range(Wg)]
                if f == "c":
                    dec = (a2, t2, e2)
            return wire, dec

        for j in range(total):
            wire, dec = step_inputs(j)
            torch.cuda.synchronize()
            for f in forms[j % len(forms):] + forms[:j % len(forms)]:   # none always runs first
                run(f, j, wire, dec)
            del wire, dec
        sizes = {f: sum(len(r) for r in g.repos) for f, g in G.items() if f != "parent_a"}
        assert len(set(sizes.values())) == 1, sizes

        def stages(rows):
            rows = rows[args.warmup:]
            return [{s: float(statistics.median([r[i][s] for r in rows]))
                     for s in ("pack", "exchange", "merge")} for i in range(Wg)]
        row = {}
        for f in forms:
            row[f] = stat(ms[f][args.warmup:])
            row[f]["stage_ms"] = stages(stg[f])
            if f in rstats:
                row[f].update(reply_stats=rstats[f], **counts[f])
        a_ = row["a"]
        ratios = {x + "_over_a": row[x]["ms"] / a_["ms"] for x in ("b", "c", "d")}
        ratios["c_over_e"] = row["c"]["ms"] / row["e"]["ms"]
        if Lp is not None:
            pa_ = row["parent_a"]
            spread = max(a_["max_ms"] - a_["min_ms"], pa_["max_ms"] - pa_["min_ms"])
            ratios.update(a_minus_parent_ms=a_["ms"] - pa_["ms"], run_spread_ms=spread,
                          a_inside_spread=abs(a_["ms"] - pa_["ms"]) <= spread)
        # the new kernels, per call: the members' kernel timing on
        kern = {}
        for j in range(total, total + args.kernel_steps):
            wire, dec = step_inputs(j)
            torch.cuda.synchronize()
            for f in ("b", "c", "d"):
                for r in G[f].repos:   # (every call of the group call on the handle keeps its timings)
                    r.set_timing(True, accumulate=True)
                G[f].receive_datagrams(wire[f], bench.T0 + j, replies=caps, **kw)
                torch.cuda.synchronize()
                tm = {}
                for r in G[f].repos:
                    for nm, x in r.timings():
                        tm[nm] = tm.get(nm, 0.0) + x
                kern.setdefault(f, []).append({k: tm.get(k, 0.0) for k in
                                               ("k_zero_count", "k_route_scatter_src", "k_route_scatter",
                                                "k_route_count")})
            del wire, dec
        row["kernels_ms_per_call_all_members"] = {
            f: {k: float(statistics.median([r[k] for r in rs])) for k in rs[-1]} for f, rs in kern.items()}
        kz = row["kernels_ms_per_call_all_members"].get("b", {}).get("k_zero_count")
        if kz is not None:
            ratios["count_pass_ms"] = kz
            ratios["b_minus_a_ms"] = row["b"]["ms"] - a_["ms"]
        row["ratios"] = ratios
        row["buckets"] = sizes["a"]
        out[key] = row
        print(json.dumps({key: dict({f: row[f]["ms"] for f in forms}, **ratios)}), flush=True)
        for g in G.values():
            g.close()
        del kind, res_cols
    out["note"] = ("one MI355X; the RCCL exchange at world > 1 (one GPU per rank) has not run on "
                   "hardware and remains unmeasured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, build_id=out["build_id"])))


if __name__ == "__main__":
    main()
