"""What a lightmap bake costs (include/ptmi.h ptmi_dispatch_bake, ptmi_bake_dilate), and that it costs nothing where it
is not used.

  (a) bake     a --size x --size surface over cornell_spheres, --spp frames: device nanoseconds per path segment (gpu_ms over
               ptmi_stats.segments, with timing = 1). The surface gives every triangle a cell of its own in a square grid of cells and
               rasterises it with ptmi.bake.rasterise, so neighbouring texels are neighbours in the scene, as in a real lightmap.
      camera   beside it, a camera render of the same scene with as many paths: a square frame of about the covered texels, --spp frames
  (b) plain    ptmi_dispatch of cornell_spheres at --width x --height, --spp frames. With --parent-lib naming a libptmi.so built from the
               parent commit, each repeat measures the parent's library first and this one after it, so that drift of the machine reaches
               both alike. The claim checked: this commit's median over the repeats lies inside the parent's own min-max range over its
               repeats - the plain dispatch launches the parent's kernels.
  (c) dilate   ptmi_bake_dilate at --size x --size, 4 passes: wall milliseconds of the call, which ends with the copy of the result
               (16 bytes per texel) to the host

One measurement is a fresh process under a time limit of its own that uploads the scene, warms up once and takes the median of
--rounds runs. --repeats measurements of (b) are made, one of (a) and (c).

    python tools/bake_cost.py [--size 1024 --width 1920 --height 1080 --spp 64 --rounds 5 --repeats 5] [--parent-lib PATH] [--json out.json]
Prints one JSON line; exits 1 when (b) lies outside the parent's range.
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

NEW_NAMES = ("ptmi_upload_bake_surface", "ptmi_dispatch_bake", "ptmi_bake_status", "ptmi_bake_dilate", "ptmi_debug_bake_rays")


def cell_atlas(n_tris):
    """lightmap coordinates that give triangle t the lower-left half of cell (t mod G, t div G) of a G x G grid, inset by a
    twentieth of a cell: (n_tris, 3, 2) float32"""
    G = int(np.ceil(np.sqrt(n_tris)))
    t = np.arange(n_tris)
    corner = np.stack([t % G, t // G], axis=1)[:, None, :] / G
    return (corner + np.array([(0.05, 0.05), (0.9, 0.05), (0.05, 0.9)])[None, :, :] / G).astype(np.float32)


def worker(a):
    """one measurement in this process: a JSON object on stdout"""
    from ptmi import layout, native, scenes
    if a.worker == "parent":                                    # a library that predates the feature: do not ask it for the new calls
        native.EXPORTS[:] = [n for n in native.EXPORTS if n not in NEW_NAMES]
    sc = scenes.make("cornell_spheres")
    out = {}
    with native.Context(0) as ctx:
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=1)
        ctx.upload_scene(sc)

        def timed(run):
            ctx.reset_stats()
            run()
            st = ctx.stats()
            return st.gpu_ms * 1e6 / st.segments, int(st.segments), int(st.paths)

        def median_of(run):
            timed(run)
            runs = [timed(run) for _ in range(a.rounds)]
            return dict(ns=float(np.median([r[0] for r in runs])), runs=[r[0] for r in runs], segments=runs[-1][1], paths=runs[-1][2])

        if a.worker in ("plain", "parent"):
            ctx.resize(a.width, a.height)
            cam = layout.make_camera(a.width, a.height)
            out["plain"] = median_of(lambda: ctx.dispatch(cam, a.spp))
        else:
            from ptmi import bake
            S = a.size
            pos, nrm, _ = bake.scene_arrays(sc)
            tex = bake.rasterise(pos, nrm, cell_atlas(len(sc.tris)), S, S)
            covered = int((tex["covered"] != 0).sum())
            ctx.resize(S, S)
            ctx.upload_bake_surface(tex)
            out["bake"] = dict(median_of(lambda: ctx.dispatch_bake(a.spp)), covered=covered, triangles=len(sc.tris))
            ms = []
            for _ in range(a.rounds + 1):
                t0 = time.perf_counter()
                ctx.bake_dilate(4)
                ms.append((time.perf_counter() - t0) * 1e3)
            out["dilate"] = dict(ms=float(np.median(ms[1:])), runs=ms[1:], passes=4)
            side = int(round(np.sqrt(covered)))
            ctx.resize(side, side)
            cam = layout.make_camera(side, side)
            out["camera"] = dict(median_of(lambda: ctx.dispatch(cam, a.spp)), width=side, height=side)
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
               unit="device ns per path segment; dilate: wall ms")
    out.update(measure(a, "bake"))
    print("bake %s" % {k: round(v.get("ns", v.get("ms")), 4) for k, v in out.items() if isinstance(v, dict)}, file=sys.stderr, flush=True)
    parent, this, last = [], [], {}
    for r in range(a.repeats):
        if a.parent_lib:
            parent.append(measure(a, "parent", a.parent_lib)["plain"]["ns"])
        last = measure(a, "plain")["plain"]
        this.append(last["ns"])
        print("repeat %d: parent %s, this %.4f" % (r, round(parent[-1], 4) if parent else None, this[-1]), file=sys.stderr, flush=True)
    plain = dict(median=float(np.median(this)), min=float(np.min(this)), max=float(np.max(this)), repeats=this, segments=last["segments"])
    ok = True
    if parent:
        out["parent"] = dict(median=float(np.median(parent)), min=float(np.min(parent)), max=float(np.max(parent)), repeats=parent)
        plain["within_parent_range"] = ok = bool(out["parent"]["min"] <= plain["median"] <= out["parent"]["max"])
        plain["ratio_to_parent"] = plain["median"] / out["parent"]["median"]
    out["plain"] = plain
    out["pass"] = ok
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
