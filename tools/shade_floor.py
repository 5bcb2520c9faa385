#!/usr/bin/env python3
"""tools/shade_floor.py <bench.json> <per_bounce.json> [first last]: the least-squares line through `shade`'s per-launch times of the
bounces first..last (default 4..7, the small queues of config 1) over their segment counts: microseconds per million segments, and the
intercept, the time of a launch with no segments. bench.json is the line bench.py printed in the traced run (segments by bounce),
per_bounce.json the output of tools/per_bounce.py for that trace."""
import json, sys


def main(bench, per_bounce, first=4, last=7):
    d = json.loads(open(bench).read().strip().splitlines()[-1])
    seg = next(v for k, v in d.items() if k.startswith("segments_by_bounce"))
    us = json.load(open(per_bounce))["per_bounce"]["shade"]
    xs = [seg[b] / float(d["steps"]) / 1e6 for b in range(first, last + 1)]        # the counters are those of the timed steps
    ys = [us[b] for b in range(first, last + 1)]
    mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
    slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    print(json.dumps({"bounces": [first, last], "msegments": [round(x, 3) for x in xs], "us": ys,
                      "us_per_msegment": round(slope, 2), "intercept_us": round(my - slope * mx, 1)}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], *(int(a) for a in sys.argv[3:5]))
