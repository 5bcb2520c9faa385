#!/usr/bin/env python3
"""tools/per_bounce_compact.py <kernel_trace.csv> [bounces]: per-bounce mean duration (us) of the compaction's kernels from a
rocprofv3 --kernel-trace CSV of bench.py with MIS on: k_tile_sums runs once per bounce, k_scatter2 after every bounce but the last,
k_scatter_packed after the last (its figure is listed under the last bounce of "scatter")."""
import collections, csv, json, re, sys


def main(path, bounces=8):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    per = {"tile_sums": collections.defaultdict(list), "scatter": collections.defaultdict(list)}
    seen = collections.Counter()
    for r in rows:
        m = re.search(r"(k_\w+)", r["Kernel_Name"])
        if not m:
            continue
        k = m.group(1)
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if k == "k_tile_sums":
            per["tile_sums"][seen[k] % bounces].append(us)
        elif k == "k_scatter2":
            per["scatter"][seen[k] % (bounces - 1)].append(us)
        elif k == "k_scatter_packed":
            per["scatter"][bounces - 1].append(us)
        else:
            continue
        seen[k] += 1
    out = {k: [round(sum(v[b]) / len(v[b]), 1) if v[b] else None for b in range(bounces)] for k, v in per.items()}
    print(json.dumps({"unit": "us per launch, mean over steps", "per_bounce": out}))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8)
