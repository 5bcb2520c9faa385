"""What editing a loaded scene in place (ptmi_update_triangles) costs beside uploading it again, and what a refitted tree costs to walk:
on grid_1m (the 1 M-triangle scene of bench.py's config 3) and cornell_spheres, in one process.

Per scene:
  plan_ms      the one-time preparation at the first update after an upload (ptmi_scene_update_status)
  refit_ms     wall time of ptmi_update_triangles for the whole triangle array and for a 1 % range, after a warm-up update: the median
               of --rounds calls with the smallest and largest beside it (every call ends in a device synchronise)
  upload_ms    ptmi_stats.upload_ms of ptmi_upload_scene for the same scene under tree_builder = 1 and 2, the comparison: median of
               --uploads calls
  walk         the scene wobbled (tests/scene_update_ref.py wobble) by 0, 1, 5 and 20 % of its extent through ONE update each from a
               fresh upload; then config 3's view (1920x1080, 8 bounces, MIS) traced for --frames frames after a warm-up dispatch:
               device time per path segment (ptmi_stats.gpu_ms / segments) beside cost_now / cost_built, and, for the same wobbled
               triangles, the same figure after a fresh upload of (wobbled triangles, refitted nodes): what a rebuild would buy

Writes --json (default profiles/scene_update_cost.json) and prints the first section of profiles/README.md for pasting.

    python tools/scene_update_cost.py [--rounds 7] [--uploads 3] [--frames 16] [--scenes grid_1m,cornell_spheres] [--json out.json]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ptmi import layout, native, scenes  # noqa: E402
import scene_update_ref as ref  # noqa: E402

W, H = 1920, 1080
WOBBLES = (0.0, 0.01, 0.05, 0.20)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return dict(median=med(xs), min=min(xs), max=max(xs), runs=list(xs))


def extent(tris):
    v = np.concatenate([tris[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


def timed_update(ctx, first, tris):
    t0 = time.perf_counter()
    ctx.update_triangles(first, tris)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, ctx.scene_update_status().refit_ms


def ns_per_segment(ctx, frames):
    cam = lambda f: layout.make_camera(W, H, frame_index=f, aperture=0.001, focus_distance=5.0)
    ctx.dispatch(cam(0), frames)                             # warm-up (allocates the batch, loads the code objects)
    ctx.reset_stats()
    ctx.dispatch(cam(frames), frames)
    st = ctx.stats()
    return st.gpu_ms * 1e6 / st.segments, int(st.segments), int(st.extend_variant)


def measure(name, a):
    sc = scenes.make(name)
    out = {"triangles": len(sc.tris), "nodes": len(sc.nodes)}
    n1 = max(1, len(sc.tris) // 100)
    with native.Context(0) as ctx:
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)
        out["upload_ms"] = {}
        for builder in (1, 2):
            ctx.set_options(tree_builder=builder)
            runs = []
            for _ in range(a.uploads):
                ctx.upload_scene(sc)
                runs.append(ctx.stats().upload_ms)
            out["upload_ms"][f"tree_builder_{builder}"] = dict(spread(runs), tree_builder_used=int(ctx.stats().tree_builder_used))
        # the plan, then whole-array and 1 % updates of the unmoved triangles (the work does not depend on the values)
        ctx.update_triangles(0, sc.tris)
        st = ctx.scene_update_status()
        out["plan_ms"] = st.plan_ms
        out["quantised_kept"] = int(st.quantised_kept)
        whole = [timed_update(ctx, 0, sc.tris) for _ in range(a.rounds)]
        part = [timed_update(ctx, len(sc.tris) // 2, sc.tris[len(sc.tris) // 2:len(sc.tris) // 2 + n1]) for _ in range(a.rounds)]
        out["refit_ms"] = {"whole": spread([w for w, _ in whole]), "whole_reported": spread([r for _, r in whole]),
                           "one_percent": spread([w for w, _ in part]), "one_percent_reported": spread([r for _, r in part]),
                           "one_percent_triangles": n1}
        out["walk"] = []
        ext = extent(sc.tris)
        for amp in WOBBLES:
            moved = ref.wobble(sc.tris, amp * ext) if amp else sc.tris
            ctx.upload_scene(sc)
            ctx.update_triangles(0, moved)
            st = ctx.scene_update_status()
            ns_refit, seg, variant = ns_per_segment(ctx, a.frames)
            ctx.upload_scene(dataclasses.replace(sc, tris=moved, nodes=ref.refit_nodes(sc.nodes, moved)))
            ns_fresh, seg_fresh, _ = ns_per_segment(ctx, a.frames)
            assert seg == seg_fresh                          # the same bits either way: the same paths
            out["walk"].append(dict(wobble=amp, cost_built=st.cost_built, cost_now=st.cost_now, ratio=st.cost_now / st.cost_built,
                                    ns_per_segment_refitted=ns_refit, ns_per_segment_rebuilt=ns_fresh, segments=seg,
                                    extend_variant=variant))
    return out


def readme(results, a):
    lines = ["# Editing a loaded scene in place (`ptmi_update_triangles`; `csrc/scene_update.hip`, `tools/scene_update_cost.py`)", "",
             f"One process per table, MI355X; medians of {a.rounds} updates / {a.uploads} uploads (smallest - largest); wall time around calls "
             "that end in a device synchronise.", "",
             "| scene | triangles | plan ms | refit ms, whole array | refit ms, 1 % range | upload ms, host builder | upload ms, device builder |",
             "|---|---|---|---|---|---|---|"]
    f = lambda s: f"{s['median']:.2f} ({s['min']:.2f} - {s['max']:.2f})"
    for name, r in results.items():
        lines.append(f"| {name} | {r['triangles']} | {r['plan_ms']:.2f} | {f(r['refit_ms']['whole'])} | {f(r['refit_ms']['one_percent'])} | "
                     f"{f(r['upload_ms']['tree_builder_1'])} | {f(r['upload_ms']['tree_builder_2'])} |")
    lines += ["", f"Walking the refitted tree: config 3's view, {a.frames} frames after a warm-up dispatch, device ns per path segment; "
              "\"rebuilt\" is a fresh upload of the same wobbled triangles.", "",
              "| scene | wobble, % of extent | cost_now / cost_built | ns per segment, refitted | ns per segment, rebuilt | refitted / rebuilt |",
              "|---|---|---|---|---|---|"]
    for name, r in results.items():
        for w in r["walk"]:
            lines.append(f"| {name} | {100 * w['wobble']:.0f} | {w['ratio']:.3f} | {w['ns_per_segment_refitted']:.3f} | "
                         f"{w['ns_per_segment_rebuilt']:.3f} | {w['ns_per_segment_refitted'] / w['ns_per_segment_rebuilt']:.3f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--scenes", default="grid_1m,cornell_spheres")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "scene_update_cost.json"))
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    a = ap.parse_args()
    results = {}
    for name in a.scenes.split(","):
        results[name] = measure(name, a)
        print(name, json.dumps({k: v for k, v in results[name].items() if k != "walk"}), flush=True)
    with open(a.json, "w") as f:
        json.dump(dict(width=W, height=H, frames=a.frames, rounds=a.rounds, uploads=a.uploads, scenes=results), f, indent=1)
    text = readme(results, a)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
