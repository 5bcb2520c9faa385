"""What alpha blending costs (include/ptmi.h ptmi_set_alpha_blend), and that it costs nothing where it is not used.

Renders scenes.cornell_fence (the enclosed Cornell box behind an 8 x 8 fence) at --width x --height, --spp frames per run, and reports
device nanoseconds per path segment (gpu_ms over ptmi_stats.segments, with timing = 1) for
  none      (a) no table: the launches of a build without either feature
  cutoff    (b) a cutoff table that cuts nothing (the walls' material, which has no albedo map): both resolve loops run on every
                bounce with the BLEND = false kernels, nothing passes
  blend_1   (c) a blend table over alpha 1 (the fence's material, factor 1): the BLEND = true kernels, every fence hit is a test,
                nothing passes, no hash is computed
  blend_05  (d) the same table over a fence of alpha 0.5: every fence hit computes the hash and half of them pass
One measurement is a fresh process that uploads the scene, warms every configuration up once and runs them in turn for --rounds
rounds; its figure for a configuration is the median over the rounds. --repeats measurements are made.

With --parent-lib naming a libptmi.so built from the parent commit, each repeat measures (a) and (b) with that library first and
then all four with this one, so that drift of the machine reaches both alike. This build passes when its median over the repeats
lies inside the parent's own min-max range over its repeats, widened on either side by that range's width: those launches are meant
to be the same code, and the parent's spread is the only margin. (c) and (d) are reported, not judged.

    python tools/alpha_blend_cost.py [--width 1920 --height 1080 --spp 64 --rounds 5 --repeats 5] [--parent-lib PATH] [--json out.json]
Prints one JSON line; exits 1 when a judged configuration lies outside its range.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

BLEND_NAMES = ("set_alpha_blend", "alpha_blend_status")


def worker(a):
    """one measurement in this process: {configuration: {ns, segments, status}} on stdout"""
    from ptmi import layout, native, scenes
    configs = a.worker.split(",")
    if not a.has_blend:                                         # a library that predates the feature: do not ask it for the new calls
        native.EXPORTS[:] = [n for n in native.EXPORTS if not n.endswith(BLEND_NAMES)]
        for n in BLEND_NAMES:
            native._SHARED.pop(n, None)
    cam = layout.make_camera(a.width, a.height)
    out = {}
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)
        # (d) needs a fence of its own; the others share the opaque one
        for alpha, keys in ((1.0, [k for k in configs if k != "blend_05"]), (0.5, [k for k in configs if k == "blend_05"])):
            if not keys:
                continue
            sc = scenes.cornell_fence(np.full((1, scenes.FENCE_CELLS, scenes.FENCE_CELLS), alpha, np.float32))
            n, fence = len(sc.mats), sc.info["fence_materials"][0]
            ctx.upload_scene(sc)
            ctx.resize(a.width, a.height)

            def one(key):
                ctx.set_alpha_cutoff(None)
                if a.has_blend:
                    ctx.set_alpha_blend(None)
                if key == "cutoff":
                    t = np.zeros(n, np.float32)
                    t[0] = 0.5                                  # the walls' material: no albedo map
                    ctx.set_alpha_cutoff(t)
                elif key != "none":
                    t = np.full(n, -1.0, np.float32)
                    t[fence] = 1.0
                    ctx.set_alpha_blend(t)
                ctx.reset_stats()
                ctx.dispatch(cam, a.spp)
                st = ctx.stats()
                status = ctx.alpha_blend_status().as_dict() if a.has_blend else None
                return st.gpu_ms * 1e6 / st.segments, int(st.segments), status
            runs = {k: [] for k in keys}
            for k in keys:
                one(k)
            for _ in range(a.rounds):
                for k in keys:
                    ns, seg, status = one(k)
                    runs[k].append(ns)
                    out[k] = dict(segments=seg, status=status)
            for k in keys:
                out[k].update(ns=float(np.median(runs[k])), runs=runs[k])
    print(json.dumps(out))


def measure(a, lib, configs, has_blend):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = os.path.abspath(lib)
    else:
        env.pop("PTMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", ",".join(configs), "--width", str(a.width), "--height", str(a.height),
           "--spp", str(a.spp), "--rounds", str(a.rounds)] + ([] if has_blend else ["--no-blend"])
    txt = subprocess.check_output(cmd, env=env, text=True, timeout=a.timeout)
    return json.loads(txt.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one measurement may take")
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--no-blend", dest="has_blend", action="store_false", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    judged, every = ["none", "cutoff"], ["none", "cutoff", "blend_1", "blend_05"]
    parent, this = {k: [] for k in judged}, {k: [] for k in every}
    last = {}
    for r in range(a.repeats):
        if a.parent_lib:
            m = measure(a, a.parent_lib, judged, False)
            for k in judged:
                parent[k].append(m[k]["ns"])
        m = measure(a, None, every, True)
        for k in every:
            this[k].append(m[k]["ns"])
        last = m
        print("repeat %d: parent %s, this %s" % (r, {k: round(v[-1], 4) for k, v in parent.items() if v},
                                                  {k: round(v[-1], 4) for k, v in this.items()}), file=sys.stderr, flush=True)
    out = dict(scene="cornell_fence", width=a.width, height=a.height, spp=a.spp, rounds=a.rounds, repeats=a.repeats,
               unit="device ns per path segment", configs={})
    ok = True
    for k in every:
        c = dict(median=float(np.median(this[k])), min=float(np.min(this[k])), max=float(np.max(this[k])), repeats=this[k],
                 segments=last[k]["segments"], status=last[k]["status"])
        if a.parent_lib and k in judged:
            lo, hi = float(np.min(parent[k])), float(np.max(parent[k]))
            c["parent"] = dict(median=float(np.median(parent[k])), min=lo, max=hi, repeats=parent[k])
            c["allowed"] = [lo - (hi - lo), hi + (hi - lo)]
            c["within_parent_range"] = bool(c["allowed"][0] <= c["median"] <= c["allowed"][1])
            ok = ok and c["within_parent_range"]
        out["configs"][k] = c
    base = out["configs"]["none"]["median"]
    for c in out["configs"].values():
        c["ratio_to_none"] = c["median"] / base
    out["pass"] = ok
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
