"""What the lightmap filter costs (include/ptmi.h ptmi_bake_denoise), and that it costs nothing where it is not used.

  (a) denoise  ptmi_bake_denoise on tools/bake_cost.py's --size x --size surface over cornell_spheres after a --spp frame bake with the
               moments plane on, 5 iterations, with and without 4 gutter passes:
                 call_ms    wall milliseconds of the synchronous call, which ends with the copy of the result (16 bytes per texel)
                 filter_ms  wall milliseconds from the asynchronous call (dst NULL) to the end of ptmi_synchronize: the kernels alone,
                            with their launches and without the copy
  (b) bake, plain  ptmi_dispatch_bake on that surface (moments off, as tools/bake_cost.py measures it) and ptmi_dispatch of
               cornell_spheres at --width x --height, --spp frames each: device nanoseconds per path segment (gpu_ms over
               ptmi_stats.segments, with timing = 1). With --parent-lib naming a libptmi.so built from the parent commit, each repeat
               measures the parent's library first and this one after it, so that drift of the machine reaches both alike. The claim
               checked: this commit's median over the repeats lies inside the parent's own min-max range over its repeats - both
               dispatches launch the parent's kernels.

One measurement is a fresh process under a time limit of its own that uploads the scene, warms up once and takes the median of
--rounds runs. --repeats measurements of (b) are made, one of (a).

    python tools/bake_denoise_cost.py [--size 1024 --width 1920 --height 1080 --spp 64 --rounds 5 --repeats 5] [--parent-lib PATH] [--json out.json]
Prints one JSON line; exits 1 when a median of (b) lies outside the parent's range.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bake_cost import cell_atlas  # noqa: E402

NEW_NAMES = ("ptmi_bake_denoise", "ptmi_bake_denoised_device_ptr", "ptmi_write_moments")


def worker(a):
    """one measurement in this process: a JSON object on stdout"""
    from ptmi import bake, layout, native, scenes
    if a.worker == "parent":                                    # a library that predates the feature: do not ask it for the new calls
        native.EXPORTS[:] = [n for n in native.EXPORTS if n not in NEW_NAMES]
    sc = scenes.make("cornell_spheres")
    S = a.size
    pos, nrm, _ = bake.scene_arrays(sc)
    tex = bake.rasterise(pos, nrm, cell_atlas(len(sc.tris)), S, S)
    covered = int((tex["covered"] != 0).sum())
    out = {}
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)
        ctx.upload_scene(sc)

        def timed(run):
            ctx.reset_stats()
            run()
            st = ctx.stats()
            return st.gpu_ms * 1e6 / st.segments, int(st.segments)

        def median_of(run):
            timed(run)
            runs = [timed(run) for _ in range(a.rounds)]
            return dict(ns=float(np.median([r[0] for r in runs])), runs=[r[0] for r in runs], segments=runs[-1][1])

        def wall(run):
            ms = []
            for _ in range(a.rounds + 1):
                t0 = time.perf_counter()
                run()
                ms.append((time.perf_counter() - t0) * 1e3)
            return dict(ms=float(np.median(ms[1:])), runs=ms[1:])

        def queued(**kw):
            ctx.bake_denoise(dst=False, **kw)
            ctx.synchronize()

        ctx.resize(S, S)
        ctx.upload_bake_surface(tex)
        if a.worker == "denoise":
            ctx.set_moments(True)
            ctx.dispatch_bake(a.spp)
            ctx.synchronize()
            out["denoise"] = dict(covered=covered, texels=S * S, iterations=5,
                                  call_ms=wall(lambda: ctx.bake_denoise(iterations=5)),
                                  call_dilate4_ms=wall(lambda: ctx.bake_denoise(iterations=5, dilate=4)),
                                  filter_ms=wall(lambda: queued(iterations=5)),
                                  filter_dilate4_ms=wall(lambda: queued(iterations=5, dilate=4)))
        else:
            out["bake"] = dict(median_of(lambda: ctx.dispatch_bake(a.spp)), covered=covered)
            ctx.upload_bake_surface(None)
            ctx.resize(a.width, a.height)
            cam = layout.make_camera(a.width, a.height)
            out["plain"] = median_of(lambda: ctx.dispatch(cam, a.spp))
    print(json.dumps(out))


def measure(a, what, lib=None):
    env = dict(os.environ)
    if lib:
        env["PTMI_LIB"] = os.path.abspath(lib)
    else:
        env.pop("PTMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--size", str(a.size), "--width", str(a.width), "--height",
           str(a.height), "--spp", str(a.spp), "--rounds", str(a.rounds)]
    txt = subprocess.check_output(cmd, env=env, text=True, timeout=a.timeout)
    return json.loads(txt.strip().splitlines()[-1])


def summary(runs):
    return dict(median=float(np.median(runs)), min=float(np.min(runs)), max=float(np.max(runs)), repeats=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one measurement may take")
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    out = dict(scene="cornell_spheres", size=a.size, width=a.width, height=a.height, spp=a.spp, rounds=a.rounds, repeats=a.repeats,
               unit="denoise: wall ms; bake, plain: device ns per path segment")
    out.update(measure(a, "denoise"))
    print("denoise %s" % {k: round(v["ms"], 4) for k, v in out["denoise"].items() if isinstance(v, dict)}, file=sys.stderr, flush=True)
    parent, this = dict(bake=[], plain=[]), dict(bake=[], plain=[])
    for r in range(a.repeats):
        for lib, into in ((a.parent_lib, parent), (None, this)):
            if into is parent and not lib:
                continue
            m = measure(a, "parent" if lib else "this", lib)
            for k in into:
                into[k].append(m[k]["ns"])
        print("repeat %d: parent %s, this %s" % (r, {k: round(v[-1], 4) for k, v in parent.items() if v},
                                                 {k: round(v[-1], 4) for k, v in this.items()}), file=sys.stderr, flush=True)
    ok = True
    for k in this:
        out[k] = summary(this[k])
        if parent[k]:
            p = out["parent_" + k] = summary(parent[k])
            out[k]["within_parent_range"] = inside = bool(p["min"] <= out[k]["median"] <= p["max"])
            out[k]["ratio_to_parent"] = out[k]["median"] / p["median"]
            ok = ok and inside
    out["pass"] = ok
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
