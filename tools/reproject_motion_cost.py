"""What ptmi_reproject costs with motion on (include/ptmi.h ptmi_set_motion), beside what it costs with motion off and what it cost
before motion existed.

At 1920x1080 on cornell_spheres and grid_1m (the 1 M-triangle scene), with HIP events on the context's stream (a caller-owned torch
stream, so that the events and the library's work share it): the device time of one ptmi_reproject after a sideways camera move
  (a) with motion off,
  (b) with motion on and nothing dirty,
  (c) with motion on after an update that moves 1 % of the triangles,
  (d) with motion on after an update that wobbles all of them,
and of ptmi_motion_commit alone after the updates of (c) and (d). Every figure is the median of --reps calls after a warm-up call, with
the smallest and the largest beside it; every reprojection starts from freshly rendered planes. The edits alternate between the moved
and the uploaded triangles, so every call of (c) and (d) sees its whole range moved against the committed positions.

--parent-tree DIR: a checkout of the parent commit with its library built (the binding insists on every symbol it lists, so the
parent's library goes with the parent's binding). Its (a) is measured in child processes of this one, before and after this build's
cases: the yardstick for (a) and (b), and two runs of the same code to read the run-to-run spread from.

    python tools/reproject_motion_cost.py [--size 1920x1080] [--reps 20] [--scenes cornell_spheres,grid_1m] [--parent-tree DIR]
                                          [--json profiles/reproject_motion_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    s = sorted(xs)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, a, baseline_only):
    import torch
    sys.path[:0] = [os.path.join(a.tree, "wgpu-path-tracing_amd"), os.path.join(a.tree, "tests")]
    from ptmi import layout, native, scenes
    import scene_update_ref as ref
    W, H = (int(v) for v in a.size.split("x"))
    cam_from = layout.make_camera(W, H)
    cam_to = layout.make_camera(W, H, position=(0.3, 1.0, 2.8))
    sc = scenes.make(name)
    n = len(sc.tris)
    out = dict(triangles=n)
    stream = torch.cuda.Stream()
    with native.Context(0) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(sc)
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=0)
        ctx.resize(W, H)
        ctx.set_aovs("albedo", "normal", "id")
        ctx.set_moments(True)

        def reprojections(edit=None):
            """edit: (first, [triangles A, triangles B]) applied in turn before each call"""
            runs = []
            for rep in range(a.reps + 1):                     # the first is the warm-up (it allocates)
                ctx.dispatch(cam_from, a.frames)
                if edit:
                    ctx.update_triangles(edit[0], edit[1][rep % 2])
                ms = timed(torch, stream, lambda: ctx.reproject(cam_from, cam_to))
                if rep:
                    runs.append(ms)
            return dict(spread(runs), status=ctx.reproject_status().as_dict())

        def commits(edit):
            runs = []
            for rep in range(a.reps + 1):
                ctx.update_triangles(edit[0], edit[1][rep % 2])
                ms = timed(torch, stream, ctx.motion_commit)
                if rep:
                    runs.append(ms)
            return spread(runs)

        out["a_motion_off"] = reprojections()
        if not baseline_only:
            v = np.concatenate([sc.tris[k] for k in ("v0", "v1", "v2")]).astype(np.float64)
            ext = float((v.max(axis=0) - v.min(axis=0)).max())
            n1 = max(1, n // 100)
            first = n // 2
            part = ref.move_part(sc.tris, np.arange(first, first + n1), np.eye(3), (0.02 * ext, 0.01 * ext, 0.0))
            one = (first, [part[first:first + n1], sc.tris[first:first + n1]])
            every = (0, [ref.wobble(sc.tris, 0.01 * ext), sc.tris])
            ctx.set_motion(True)
            out["b_motion_on_clean"] = reprojections()
            out["c_one_percent_moved"] = dict(reprojections(one), triangles=n1, motion=ctx.motion_status().as_dict())
            ctx.update_triangles(0, sc.tris)
            ctx.motion_commit()
            out["d_all_wobbled"] = dict(reprojections(every), motion=ctx.motion_status().as_dict())
            ctx.update_triangles(0, sc.tris)
            ctx.motion_commit()
            out["commit_one_percent"] = commits(one)
            out["commit_all"] = commits(every)
            ctx.update_triangles(0, sc.tris)                  # the scene as uploaded again
            ctx.set_motion(False)
            out["a_motion_off_again"] = reprojections()
        ctx.synchronize()
        ctx.set_stream(0)
    return out


def parent_run(a):
    """case (a) with the parent's library and binding, in a child process (a process loads one libptmi)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--baseline-only", "--tree", os.path.abspath(a.parent_tree), "--size", a.size,
           "--reps", str(a.reps), "--frames", str(a.frames), "--scenes", a.scenes]
    return json.loads(subprocess.check_output(cmd, text=True, timeout=900).strip().splitlines()[-1])


def readme(res, a):
    f = lambda s: f"{s['median']:.3f} ({s['min']:.3f} - {s['max']:.3f})"
    lines = ["# Reprojection across a geometry edit (`ptmi_set_motion`; `csrc/motion.hip`, `csrc/reproject.hip`, "
             "`tools/reproject_motion_cost.py`)", "",
             f"{a.size}, MI355X, HIP events around one `ptmi_reproject` after a sideways camera move; medians of {a.reps} calls after a "
             "warm-up call (smallest - largest), ms. \"parent\" is the parent commit's library measured in the same call, in child "
             "processes before and after this build's cases.", "",
             "| scene | triangles | parent, before | parent, after | (a) motion off | (a) again, last | (b) on, nothing dirty | (c) on, 1 % moved | "
             "(d) on, all wobbled | commit alone, 1 % | commit alone, all |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in res["this"].items():
        p = [f(run[name]["a_motion_off"]) if run else "not measured" for run in res["parent"]]
        lines.append(f"| {name} | {r['triangles']} | {p[0]} | {p[1]} | {f(r['a_motion_off'])} | {f(r['a_motion_off_again'])} | "
                     f"{f(r['b_motion_on_clean'])} | {f(r['c_one_percent_moved'])} | {f(r['d_all_wobbled'])} | {f(r['commit_one_percent'])} | "
                     f"{f(r['commit_all'])} |")
    lines += ["", "Pixels of the last call of each case that took the moved rule (of them, carried): " +
              "; ".join(f"{name}: (c) {r['c_one_percent_moved']['motion']['moved']} ({r['c_one_percent_moved']['motion']['moved_carried']}), "
                        f"(d) {r['d_all_wobbled']['motion']['moved']} ({r['d_all_wobbled']['motion']['moved_carried']})"
                        for name, r in res["this"].items()) + "."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=2, help="frames accumulated before each reprojection")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default="cornell_spheres,grid_1m")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its case (a), before and after this build's cases")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose ptmi package and library are measured (default: this one)")
    ap.add_argument("--baseline-only", action="store_true", help="case (a) alone, one JSON line (what --parent-tree runs with --tree)")
    ap.add_argument("--json")
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    a = ap.parse_args()
    names = a.scenes.split(",")
    if a.baseline_only:
        print(json.dumps({name: measure(name, a, True) for name in names}), flush=True)
        return
    res = dict(size=a.size, reps=a.reps, frames=a.frames, parent=[None, None])
    if a.parent_tree:
        res["parent"][0] = parent_run(a)
    res["this"] = {name: measure(name, a, False) for name in names}
    if a.parent_tree:
        res["parent"][1] = parent_run(a)
    text = readme(res, a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
