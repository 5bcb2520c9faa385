"""What camera projections cost (include/ptmi.h ptmi_set_projections), and that they cost nothing where they are not used.

Renders cornell_spheres at --width x --height, --spp frames per run, and reports device nanoseconds per path segment (gpu_ms over
ptmi_stats.segments, with timing = 1) for
  off        the switch off: the launches of a build without the feature
  on_kind0   the switch on and a perspective camera: the same kernels behind one more host-side check
  ortho      an orthographic camera whose frame covers the box's open side (other rays than the pinhole's: another picture, so the
             figure is per segment)
  equirect   the full sphere from inside the box
One measurement is a fresh process that uploads the scene, warms every configuration up once and runs them in turn for --rounds
rounds; its figure for a configuration is the median over the rounds. --repeats measurements are made.

With --parent-lib naming a libptmi.so built from the parent commit, each repeat measures `off` with that library first and then all
four with this one, so that drift of the machine reaches both alike. The claim checked: the medians of `off` and `on_kind0` over the
repeats lie inside the parent's own min-max range over its repeats - those launches are the same code (the kernels' instruction
streams are the parent's). `ortho` and `equirect` are reported, not judged.

    python tools/projection_cost.py [--width 1920 --height 1080 --spp 64 --rounds 5 --repeats 5] [--parent-lib PATH] [--json out.json]
Prints one JSON line; exits 1 when a judged configuration lies outside the parent's range.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

NEW_NAMES = ("set_projections", "get_projections")
EVERY, JUDGED = ["off", "on_kind0", "ortho", "equirect"], ["off", "on_kind0"]


def worker(a):
    """one measurement in this process: {configuration: {ns, segments, runs}} on stdout"""
    from ptmi import layout, native, scenes
    configs = a.worker.split(",")
    if not a.has_projections:                                   # a library that predates the feature: do not ask it for the new calls
        native.EXPORTS[:] = [n for n in native.EXPORTS if not n.endswith(NEW_NAMES)]
        for n in NEW_NAMES:
            native._SHARED.pop(n, None)
    W, H = a.width, a.height
    cams = {"off": layout.make_camera(W, H), "on_kind0": layout.make_camera(W, H)}
    if a.has_projections:
        cams["ortho"] = layout.make_camera(W, H, projection="orthographic", ymag=1.0)
        cams["equirect"] = layout.make_camera(W, H, position=(0.0, 1.0, 0.0), projection="equirect")
    out = {}
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)
        ctx.upload_scene(scenes.make("cornell_spheres"))
        ctx.resize(W, H)

        def one(key):
            if a.has_projections:
                ctx.set_projections(key != "off")
            ctx.reset_stats()
            ctx.dispatch(cams[key], a.spp)
            st = ctx.stats()
            return st.gpu_ms * 1e6 / st.segments, int(st.segments)
        runs = {k: [] for k in configs}
        for k in configs:
            one(k)
        for _ in range(a.rounds):
            for k in configs:
                ns, seg = one(k)
                runs[k].append(ns)
                out[k] = dict(segments=seg)
        for k in configs:
            out[k].update(ns=float(np.median(runs[k])), runs=runs[k])
    print(json.dumps(out))


def measure(a, lib, configs, has_projections):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = os.path.abspath(lib)
    else:
        env.pop("PTMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", ",".join(configs), "--width", str(a.width), "--height", str(a.height),
           "--spp", str(a.spp), "--rounds", str(a.rounds)] + ([] if has_projections else ["--no-projections"])
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
    ap.add_argument("--no-projections", dest="has_projections", action="store_false", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    parent, this, last = [], {k: [] for k in EVERY}, {}
    for r in range(a.repeats):
        if a.parent_lib:
            parent.append(measure(a, a.parent_lib, ["off"], False)["off"]["ns"])
        last = measure(a, None, EVERY, True)
        for k in EVERY:
            this[k].append(last[k]["ns"])
        print("repeat %d: parent %s, this %s" % (r, round(parent[-1], 4) if parent else None, {k: round(v[-1], 4) for k, v in this.items()}),
              file=sys.stderr, flush=True)
    out = dict(scene="cornell_spheres", width=a.width, height=a.height, spp=a.spp, rounds=a.rounds, repeats=a.repeats,
               unit="device ns per path segment", configs={})
    if parent:
        out["parent"] = dict(median=float(np.median(parent)), min=float(np.min(parent)), max=float(np.max(parent)), repeats=parent)
    ok = True
    for k in EVERY:
        c = dict(median=float(np.median(this[k])), min=float(np.min(this[k])), max=float(np.max(this[k])), repeats=this[k],
                 segments=last[k]["segments"])
        if parent and k in JUDGED:
            c["within_parent_range"] = bool(out["parent"]["min"] <= c["median"] <= out["parent"]["max"])
            c["ratio_to_parent"] = c["median"] / out["parent"]["median"]
            ok = ok and c["within_parent_range"]
        out["configs"][k] = c
    base = out["configs"]["off"]["median"]
    for c in out["configs"].values():
        c["ratio_to_off"] = c["median"] / base
    out["pass"] = ok
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
