#!/usr/bin/env python3
"""The unfiltered export sweep of two builds side by side: merges runs of
tools/export_sweep_bench.py into the `ab_unfiltered_sweep` block of
profiles/digest_bench.json.

Produce the runs on one box, alternating, at least five each, one process per
run; the other build is a library built from the sources before the sweep's
partition flag, loaded through PATROLHIP_LIB:

    for i in 1 2 3 4 5; do
      PATROLHIP_LIB=/path/to/before/libpatrolhip.so \\
        python tools/export_sweep_bench.py --dump-reps 1 --out runs/before_$i.json
      python tools/export_sweep_bench.py --dump-reps 1 --out runs/after_$i.json
    done
    python tools/sweep_ab.py --before runs/before_*.json --after runs/after_*.json

Per run and config ([b"b%d" names, 10 % 32-byte names]) it keeps the one-call
sweep's count + scan + write kernel ms and count mode's kernel ms, and judges
the one-call sweep: the later build's median must lie within the earlier
build's own min-max spread widened by 2 % (the box-to-box spread README
quotes).  Exit status 1 if it does not.  --disassembly records what comparing
the two builds' assembly showed (hipcc -S --cuda-device-only of
phip_engine.hip, the unfiltered sweep kernels' bodies side by side); without
it the note of an existing block is kept.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDEN = 0.02


def series(paths):
    runs = [json.load(open(p)) for p in sorted(paths)]
    ids = {r["build_id"] for r in runs}
    assert len(ids) == 1, "runs of more than one build: %s" % sorted(ids)
    return dict(build_id=ids.pop(),
                one_call_sweep_kernels_ms=[[c["sweep_one_call"]["sweep_kernels_ms"]
                                            for c in r["configs"]] for r in runs],
                count_mode_ms=[[c["count"]["kernels_ms"]["k_sweep_count"] for c in r["configs"]]
                               for r in runs])


def verdict(before, after):
    lo, hi = min(before) * (1 - WIDEN), max(before) * (1 + WIDEN)
    m = statistics.median(after)
    return dict(before_min=min(before), before_max=max(before), bound_lo=lo, bound_hi=hi,
                after_min=min(after), after_max=max(after), after_median=m, within=lo <= m <= hi)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--before", nargs="+", required=True)
    p.add_argument("--after", nargs="+", required=True)
    p.add_argument("--disassembly", help="what comparing the two builds' assembly of the "
                   "unfiltered kernels showed (kept from the existing block when omitted)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest_bench.json"))
    args = p.parse_args()
    assert len(args.before) >= 5 and len(args.after) >= 5, "at least five runs each"
    before, after = series(args.before), series(args.after)

    def col(s, i):
        return [x[i] for x in s["one_call_sweep_kernels_ms"]]
    block = dict(
        tool="tools/sweep_ab.py",
        what="tools/export_sweep_bench.py --dump-reps 1, a library built before the sweep's partition "
             "flag and this build's alternating on one box, one process per run; per run [b%d names, "
             "10 % 32-byte names]: the one-call sweep's count + scan + write kernel ms (medians of 10) "
             "and count mode's kernel ms",
        before=before, after=after,
        one_call_b_names=verdict(col(before, 0), col(after, 0)),
        one_call_long_names=verdict(col(before, 1), col(after, 1)),
        criterion="the later build's median within the earlier build's own min-max spread widened by 2 %")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    note = args.disassembly or doc.get("ab_unfiltered_sweep", {}).get("disassembly")
    if note:
        block["disassembly"] = note
    doc["ab_unfiltered_sweep"] = block
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(b_names=block["one_call_b_names"], long_names=block["one_call_long_names"])))
    return 0 if block["one_call_b_names"]["within"] and block["one_call_long_names"]["within"] else 1


if __name__ == "__main__":
    sys.exit(main())
