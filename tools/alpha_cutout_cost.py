"""What alpha cutouts cost (include/ptmi.h ptmi_set_alpha_cutoff).

Renders scenes.cornell_fence (the enclosed Cornell box behind an 8 x 8 checker fence) at --width x --height, --spp frames per run, and
reports device nanoseconds per path segment (gpu_ms over ptmi_stats.segments, with timing = 1) for
  none        no table: the launches of a build without the feature (the fence is opaque)
  opaque      a table whose only cutout material has no albedo map (alpha 1): both resolve loops run on every bounce, nothing passes
  checker_L   the fence's material cut at 0.5, max_layers = L for L in --layers: every other cell is a hole
Every configuration is warmed up once; then --rounds rounds run them all in turn, so that drift of the machine reaches all alike; the
figure of a configuration is the median over its rounds, reported beside the smallest and the largest. The scene is uploaded once.
After the rounds each configuration runs once more with timing = 3 for a breakdown by stage (ms of device time: the path loop counts
under extend, the shadow loop under shadow); those runs carry an event pair per launch and are not part of the figures.

    python tools/alpha_cutout_cost.py [--width 1920 --height 1080 --spp 64 --rounds 7 --layers 1 4 8] [--json out.json] [--none-only]
--none-only runs `none` alone and never calls the feature: with PTMI_LIB naming a build that predates it, the baseline.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402


def run(ctx, cam, spp):
    ctx.reset_stats()
    ctx.dispatch(cam, spp)
    st = ctx.stats()
    return st.gpu_ms * 1e6 / st.segments, int(st.segments)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--none-only", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    has_alpha = not a.none_only
    alpha = np.add.outer(np.arange(scenes.FENCE_CELLS), np.arange(scenes.FENCE_CELLS)) % 2 == 0
    sc = scenes.cornell_fence(alpha[None].astype(np.float32))
    fence = sc.info["fence_materials"][0]
    n = len(sc.mats)
    tables = {"none": (None, 0)}
    if has_alpha:
        opaque = np.zeros(n, np.float32)
        opaque[0] = 0.5                                         # the walls' material: no albedo map
        cut = np.zeros(n, np.float32)
        cut[fence] = 0.5
        tables["opaque"] = (opaque, 0)
        for L in a.layers:
            tables["checker_%d" % L] = (cut, L)
    cam = layout.make_camera(a.width, a.height)
    runs = {k: [] for k in tables}
    segments, status = {}, {}
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(a.width, a.height)
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)

        def one(key):
            table, layers = tables[key]
            if has_alpha:
                ctx.set_alpha_cutoff(table, max_layers=layers)
            ns, seg = run(ctx, cam, a.spp)
            if has_alpha:
                status[key] = ctx.alpha_status().as_dict()
            return ns, seg
        for key in tables:                                      # warm-up of every configuration (and its batch arrays)
            one(key)
        for _ in range(a.rounds):
            for key in tables:
                ns, seg = one(key)
                runs[key].append(ns)
                segments[key] = seg
            print({k: round(v[-1], 4) for k, v in runs.items()}, file=sys.stderr, flush=True)
        used = int(ctx.stats().frames_per_batch_used)
        ctx.set_options(timing=3)
        stages = {}
        for key in tables:
            one(key)
            st = ctx.stats()
            stages[key] = {k: round(float(getattr(st, k)), 3) for k in ("gpu_ms", "extend_ms", "shade_ms", "shadow_ms", "compact_ms",
                                                                          "raygen_ms", "accumulate_ms")}
    out = dict(scene=sc.name, width=a.width, height=a.height, spp=a.spp, rounds=a.rounds, library=os.path.relpath(native.LIB_PATH, ROOT),
               frames_per_batch_used=used, unit="device ns per path segment",
               configs={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), runs=v, segments=segments[k],
                                status=status.get(k), stages_ms=stages[k]) for k, v in runs.items()})
    base = out["configs"]["none"]["median"]
    for k, c in out["configs"].items():
        c["ratio_to_none"] = c["median"] / base
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
