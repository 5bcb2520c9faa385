"""What moving an object by matrix on the device (ptmi_transform_groups) costs beside sending its records (ptmi_update_triangles), on
grid_1m (the 1 M-triangle scene of bench.py's config 3) and cornell_spheres, for groups that cover 1 % and 100 % of the triangles.

The yardstick is the path there was before: ptmi_update_triangles with the same transformed records, prepared beforehand (the host-side
transform that path needs as well is NOT counted). Members of a glTF node are scattered over the uploaded array by the builder's
reorder, so the 1 % group here is a seeded random 1 % of the triangles, and the update path has two readings: `span`, one call over
[lowest member, highest member] (what a host without a scatter list per object sends), and `contiguous`, one call over a 1 % range
(the best case, which a scattered object cannot have).

Per scene and share, in ONE process and in turn: 2 warm-up runs, then the median of 10 runs of
  transform_ms   ptmi_transform_status.transform_ms of transform_groups (its refit included)
  update_ms      ptmi_scene_update_status.refit_ms of update_triangles (its copy and refit included)
with the wall time around each call beside it. Every run moves the group to another matrix, so no run finds its work done.

The driver runs one worker process per library - the one as built and, where lib/ab/libptmi_old.so exists (the parent commit's
library, for a same-box comparison of a change to this path with its parent), that one - each under its own `timeout`, one after the
other, and stops at the first that fails. It writes --json (default profiles/transform_cost.json) and prints the first section of
profiles/README.md for pasting. (The lane-per-triangle layout the kernel was once measured against is in profiles/README.md.)

    python tools/transform_cost.py [--rounds 10] [--warmup 2] [--scenes grid_1m,cornell_spheres] [--json out.json] [--limit 480]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wgpu-path-tracing_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAYOUTS = {"eight_lanes": os.path.join(PKG, "lib", "libptmi.so"), "parent": os.path.join(PKG, "lib", "ab", "libptmi_old.so")}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return dict(median=med(xs), min=min(xs), max=max(xs), runs=list(xs))


def worker(a):
    from ptmi import native, scenes
    import transform_ref as ref
    results = {}
    for name in a.scenes.split(","):
        sc = scenes.make(name)
        n = len(sc.tris)
        rng = np.random.default_rng(3)
        one = np.zeros(n, np.uint32)
        one[rng.choice(n, max(1, n // 100), replace=False)] = 1
        shares = {"1": (one, 1), "100": (np.zeros(n, np.uint32), 0)}
        runs = a.warmup + a.rounds
        mats = [ref.affine(ref.rot_y(0.01 * (k + 1)), shift=(0.001 * k, 0.0, 0.0)) for k in range(runs)]
        out = {"triangles": n}
        with native.Context(0) as ctx:
            ctx.set_options(leaves=2, tree_builder=2)
            for share, (groups, g) in shares.items():
                member = np.flatnonzero(groups == g)
                lo, hi = int(member.min()), int(member.max())
                rest = ref.rest_of(sc.tris)
                records = [ref.transformed(sc.tris, rest, groups, [ref.op(g, m)]) for m in mats]      # prepared beforehand
                ops = [native.group_ops([ref.op(g, m)]) for m in mats]
                ctx.upload_scene(sc)
                ctx.set_triangle_groups(groups)
                t_ms, t_wall = [], []
                for k in range(runs):
                    t0 = time.perf_counter()
                    ctx.transform_groups(ops[k])
                    t_wall.append((time.perf_counter() - t0) * 1e3)
                    t_ms.append(ctx.transform_status().transform_ms)
                assert ctx.read_triangles(lo, 1).tobytes() == records[-1][lo:lo + 1].tobytes()
                r = dict(members=len(member), span=hi - lo + 1, plan_ms=ctx.scene_update_status().plan_ms,
                         transform_ms=spread(t_ms[a.warmup:]), transform_wall_ms=spread(t_wall[a.warmup:]))
                ranges = {"span": (lo, hi + 1)}
                if share == "1":
                    ranges["contiguous"] = (n // 2, n // 2 + len(member))
                for what, (first, end) in ranges.items():
                    ctx.upload_scene(sc)
                    u_ms, u_wall = [], []
                    for k in range(runs):
                        part = np.ascontiguousarray(records[k][first:end])
                        t0 = time.perf_counter()
                        ctx.update_triangles(first, part)
                        u_wall.append((time.perf_counter() - t0) * 1e3)
                        u_ms.append(ctx.scene_update_status().refit_ms)
                    r[f"update_{what}_ms"] = spread(u_ms[a.warmup:])
                    r[f"update_{what}_wall_ms"] = spread(u_wall[a.warmup:])
                    r[f"update_{what}_bytes"] = (end - first) * 128
                out[share] = r
                del records
        results[name] = out
        print(name, json.dumps({s: {k: (v["median"] if isinstance(v, dict) else v) for k, v in out[s].items()} for s in shares}),
              file=sys.stderr, flush=True)
    print(json.dumps(results))


def readme(res, a):
    f = lambda s: f"{s['median']:.2f} ({s['min']:.2f} - {s['max']:.2f})"
    lines = ["# Moving objects on the device (`ptmi_transform_groups`; `csrc/scene_transform.hip`, `tools/transform_cost.py`)", "",
             f"One process per layout, MI355X; medians of {a.rounds} calls after {a.warmup} warm-up calls (smallest - largest), from the "
             "`*_ms` status fields (wall time of the call inside the library; every call ends in a device synchronise). The update path is "
             "`ptmi_update_triangles` with the same records prepared beforehand: `span` sends [lowest member, highest member], `contiguous` "
             "a range as long as the group (a scattered object cannot have it).", "",
             "| layout | scene | share | members | transform ms | update ms, span | update ms, contiguous | bytes sent, transform / span |",
             "|---|---|---|---|---|---|---|---|"]
    for layout, scenes_ in res.items():
        for name, r in scenes_.items():
            for share in ("1", "100"):
                s = r[share]
                contiguous = f(s["update_contiguous_ms"]) if "update_contiguous_ms" in s else "-"
                lines.append(f"| {layout} | {name} | {share} % | {s['members']} | {f(s['transform_ms'])} | {f(s['update_span_ms'])} | "
                             f"{contiguous} | 96 / {s['update_span_bytes']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="grid_1m,cornell_spheres")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "transform_cost.json"))
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    ap.add_argument("--limit", type=int, default=480, help="seconds a worker may take")
    ap.add_argument("--worker", action="store_true", help="measure with the library PTMI_LIB names and print JSON (what the driver starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = {}
    for layout, lib in LAYOUTS.items():
        if not os.path.exists(lib):
            print(f"{layout}: {lib} is not built, skipped", file=sys.stderr)
            continue
        # a fresh process per layout under its own time limit; a failure ends the run: nothing more is started on the device
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(a.rounds),
               "--warmup", str(a.warmup), "--scenes", a.scenes]
        p = subprocess.run(cmd, env=dict(os.environ, PTMI_LIB=lib), stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"{layout}: the worker ended with status {p.returncode}; nothing further was run")
        res[layout] = json.loads(p.stdout.strip().splitlines()[-1])
    with open(a.json, "w") as f:
        json.dump(dict(rounds=a.rounds, warmup=a.warmup, layouts=res), f, indent=1)
    text = readme(res, a)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
