"""What rebuilding the walked tree in place (ptmi_rebuild_tree) costs beside uploading the edited scene again, and what it buys per path
segment: on grid_1m (the 1 M-triangle scene of bench.py's config 3) and cornell_spheres, in one process.

Per scene the triangles are wobbled (tests/scene_update_ref.py wobble) in growing steps, one ptmi_update_triangles each, until the
refitted tree's cost_now / cost_built passes --ratio (about 1.8). Then, for that edited scene:
  build_ms        ptmi_rebuild_status.build_ms of ptmi_rebuild_tree (builder 2), --rounds calls: the first on the refitted tree, the others
                  on the rebuilt one (the same build: its input is the triangles, not the tree); and the plan_ms of each re-plan
  upload_ms       ptmi_stats.upload_ms / upload_tree_ms of a fresh tree_builder = 2 upload of (edited triangles, refitted nodes), the
                  yardstick, --uploads calls
  ns per segment  config 3's view (1920x1080, 8 bounces, MIS), --frames frames after a warm-up dispatch, device time per path segment
                  (ptmi_stats.gpu_ms / segments), --rounds times each: refitted, rebuilt, freshly uploaded
The rebuilt and the fresh image are compared byte for byte on the way (the contract; tests/test_gpu_rebuild_tree.py checks it properly).

The yardsticks are the fresh upload and nothing of the new code: a rebuild does the upload's build without validation and copies, so
build_ms should not exceed upload_tree_ms + the re-plan by more than the run-to-run spread of upload_tree_ms; the rebuilt and the
fresh per-segment times should agree within their spread. The verdicts are reported, not asserted.

Writes --json (default profiles/rebuild_cost.json) and prints the first section of profiles/README.md for pasting.

    python tools/rebuild_cost.py [--rounds 3] [--uploads 3] [--frames 8] [--ratio 1.8] [--scenes grid_1m,cornell_spheres] [--json out.json]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ptmi import layout, native, scenes  # noqa: E402
import scene_update_ref as ref  # noqa: E402

W, H = 1920, 1080
STEPS = (0.02, 0.05, 0.10, 0.15, 0.20, 0.25, 0.30, 0.40, 0.50)      # wobble amplitudes, fractions of the scene's extent


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return dict(median=med(xs), min=min(xs), max=max(xs), runs=list(xs))


def extent(tris):
    v = np.concatenate([tris[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


def ns_per_segment(ctx, frames, rounds):
    cam = lambda f: layout.make_camera(W, H, frame_index=f, aperture=0.001, focus_distance=5.0)
    ctx.dispatch(cam(0), frames)                             # warm-up (allocates the batch, loads the code objects)
    runs, seg, variant = [], 0, 0
    for _ in range(rounds):
        ctx.reset_stats()
        ctx.dispatch(cam(frames), frames)
        st = ctx.stats()
        runs.append(st.gpu_ms * 1e6 / st.segments)
        seg, variant = int(st.segments), int(st.extend_variant)
    return spread(runs), seg, variant


def image_bytes(ctx):
    return b"".join(a.tobytes() for a in ctx.read_image()[1:] if a is not None)


def measure(name, a):
    sc = scenes.make(name)
    out = {"triangles": len(sc.tris), "nodes": len(sc.nodes), "steps": []}
    ext = extent(sc.tris)
    with native.Context(0) as ctx:
        ctx.resize(W, H)
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1, leaves=2, tree_builder=2)
        ctx.upload_scene(sc)
        out["tree_builder_used"] = int(ctx.stats().tree_builder_used)
        moved = sc.tris
        for amp in STEPS:
            moved = ref.wobble(sc.tris, amp * ext)
            ctx.update_triangles(0, moved)
            st = ctx.scene_update_status()
            out["steps"].append(dict(wobble=amp, ratio=st.cost_now / st.cost_built, refit_ms=st.refit_ms))
            if st.cost_now / st.cost_built >= a.ratio:
                break
        st = ctx.scene_update_status()
        out.update(cost_built=st.cost_built, cost_refitted=st.cost_now, ratio=st.cost_now / st.cost_built, first_plan_ms=st.plan_ms)
        out["ns_refitted"], seg, out["variant_refitted"] = ns_per_segment(ctx, a.frames, a.rounds)
        builds, plans = [], []
        for _ in range(a.rounds):
            rb = ctx.rebuild_tree(2)
            builds.append(rb.build_ms)
            plans.append(ctx.scene_update_status().plan_ms)
            if len(builds) == 1:
                out.update(cost_rebuilt=rb.cost_after, builder_used=int(rb.builder_used))
        out["build_ms"], out["replan_ms"] = spread(builds), spread(plans)
        rebuilt = image_bytes(ctx)
        out["ns_rebuilt"], seg_rebuilt, out["variant_rebuilt"] = ns_per_segment(ctx, a.frames, a.rounds)
        fresh = dataclasses.replace(sc, tris=moved, nodes=ref.refit_nodes(sc.nodes, moved))
        ups, trees = [], []
        for _ in range(a.uploads):
            ctx.upload_scene(fresh)
            ups.append(ctx.stats().upload_ms)
            trees.append(ctx.stats().upload_tree_ms)
        out["upload_ms"], out["upload_tree_ms"] = spread(ups), spread(trees)
        out["image_equals_fresh_upload"] = rebuilt == image_bytes(ctx)
        out["ns_fresh"], seg_fresh, out["variant_fresh"] = ns_per_segment(ctx, a.frames, a.rounds)
        assert seg == seg_rebuilt == seg_fresh               # the same bits either way: the same paths
        out["segments"] = seg
    t, b, p = out["upload_tree_ms"], out["build_ms"], out["replan_ms"]
    out["build_yardstick_ms"] = t["median"] + p["median"] + (t["max"] - t["min"])
    out["build_within_yardstick"] = b["median"] <= out["build_yardstick_ms"]
    margin = max(out["ns_rebuilt"]["max"] - out["ns_rebuilt"]["min"], out["ns_fresh"]["max"] - out["ns_fresh"]["min"])
    out["ns_rebuilt_equals_fresh_within_spread"] = abs(out["ns_rebuilt"]["median"] - out["ns_fresh"]["median"]) <= margin
    return out


def readme(results, a):
    f = lambda s: f"{s['median']:.2f} ({s['min']:.2f} - {s['max']:.2f})"
    g = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"
    lines = ["# Rebuilding the walked tree in place (`ptmi_rebuild_tree`; `csrc/scene_rebuild.hip`, `tools/rebuild_cost.py`)", "",
             f"One process, MI355X; the scene wobbled in steps until cost_now / cost_built passed {a.ratio}; medians of {a.rounds} rebuilds / "
             f"{a.uploads} fresh `tree_builder = 2` uploads of the same edited scene (smallest - largest).", "",
             "| scene | triangles | ratio | builder | rebuild ms | of which re-plan ms | fresh upload ms | its upload_tree_ms | yardstick ms | within |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in results.items():
        lines.append(f"| {name} | {r['triangles']} | {r['ratio']:.3f} | {r['builder_used']} | {f(r['build_ms'])} | {f(r['replan_ms'])} | "
                     f"{f(r['upload_ms'])} | {f(r['upload_tree_ms'])} | {r['build_yardstick_ms']:.2f} | {'yes' if r['build_within_yardstick'] else 'NO'} |")
    lines += ["", f"Config 3's view, {a.frames} frames after a warm-up dispatch, device ns per path segment, {a.rounds} runs each; the rebuilt image "
              "equals the fresh upload's byte for byte.", "",
              "| scene | cost refitted -> rebuilt (built) | ns refitted | ns rebuilt | ns fresh upload | refitted / rebuilt | rebuilt = fresh within spread |",
              "|---|---|---|---|---|---|---|"]
    for name, r in results.items():
        lines.append(f"| {name} | {r['cost_refitted']:.3f} -> {r['cost_rebuilt']:.3f} ({r['cost_built']:.3f}) | {g(r['ns_refitted'])} | {g(r['ns_rebuilt'])} | "
                     f"{g(r['ns_fresh'])} | {r['ns_refitted']['median'] / r['ns_rebuilt']['median']:.3f} | "
                     f"{'yes' if r['ns_rebuilt_equals_fresh_within_spread'] else 'NO'} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--ratio", type=float, default=1.8)
    ap.add_argument("--scenes", default="grid_1m,cornell_spheres")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rebuild_cost.json"))
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    a = ap.parse_args()
    results = {}
    for name in a.scenes.split(","):
        results[name] = measure(name, a)
        print(name, json.dumps(results[name]), flush=True)
    with open(a.json, "w") as f:
        json.dump(dict(width=W, height=H, frames=a.frames, rounds=a.rounds, uploads=a.uploads, ratio=a.ratio, scenes=results), f, indent=1)
    text = readme(results, a)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
