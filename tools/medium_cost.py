"""What the participating medium (ptmi_set_medium) costs: bench.py's config 1 (Cornell, 1920x1080, 64 frames, 8 bounces, MIS) at full
size in two set-ups on one context, in alternating runs (none, fog, none, ...): no medium (the kernels of before) and a medium over
the scene's box of optical thickness about 1 across the room (sigma_t = 1 / the box's largest extent, albedo 0.8, g = 0.3). Each run
is one timed 64-frame dispatch after a warm-up; reported are the dispatch's milliseconds of device time, Msegments/s (path segments
per second of device time, bench.py's metric) and the shade kernel's milliseconds per dispatch (timing = 3), each as the median of
the rounds with the smallest and the largest run beside it: the run-to-run spread.

The no-medium render launches the kernels of a build without the medium. To hold its time against such a build (the commit before
ptmi_set_medium), run this file with `--only none` from a checkout of each (copied into the older one, where it finds no medium to
remove), in alternation on one machine, and compare the medians with the spread printed here.

    python tools/medium_cost.py [--rounds 5] [--only none] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402

CFG = dict(scene="cornell", width=1920, height=1080, fps=64, bounces=8, mis=1)      # bench.py CONFIGS[1]
SETUPS = ("none", "fog")


def scene_box(sc):
    v = np.concatenate([sc.tris[k][:, :3] for k in ("v0", "v1", "v2")]).astype(np.float64)
    return tuple(np.float32(v.min(axis=0))), tuple(np.float32(v.max(axis=0)))


def measure(ctx, fog, setup, frame_index):
    if setup == "fog":
        ctx.set_medium(**fog)
    elif hasattr(native.load(), "ptmi_set_medium"):         # (a build from before the medium has nothing to remove)
        ctx.set_medium(None)
    W, H, fps = CFG["width"], CFG["height"], CFG["fps"]
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index), fps)          # warm-up (allocates the batch)
    ctx.reset_stats()
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index + fps), fps)
    st = ctx.stats()
    return st.gpu_ms, st.segments / (st.gpu_ms * 1e3), st.shade_ms, st.segments


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=SETUPS, help="time this set-up alone (none: also runs on a build without ptmi_set_medium)")
    ap.add_argument("--json")
    a = ap.parse_args()
    setups = (a.only,) if a.only else SETUPS
    sc = scenes.make(CFG["scene"])
    lo, hi = scene_box(sc)
    fog = dict(sigma_t=float(1.0 / (np.asarray(hi, np.float64) - lo).max()), albedo=0.8, g=0.3, box=(lo, hi))
    runs = {k: [] for k in setups}
    with native.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.resize(CFG["width"], CFG["height"])
        ctx.set_options(max_bounces=CFG["bounces"], do_mis=CFG["mis"], frames_per_batch=0, timing=3)
        for r in range(a.rounds):
            for k in setups:
                runs[k].append(measure(ctx, fog, k, 128 * r))
    out = {"sigma_t": fog["sigma_t"]}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for k in setups:
        out[k] = dict(gpu_ms=[x[0] for x in runs[k]], msegments=[x[1] for x in runs[k]], shade_ms=[x[2] for x in runs[k]],
                      segments=runs[k][-1][3])
        out[k].update(median_gpu_ms=med(out[k]["gpu_ms"]), median_msegments=med(out[k]["msegments"]), median_shade_ms=med(out[k]["shade_ms"]))
        print(f"{k:5s} {out[k]['median_gpu_ms']:8.2f} ms per {CFG['fps']}-frame dispatch (min {min(out[k]['gpu_ms']):.2f}, max {max(out[k]['gpu_ms']):.2f}; "
              f"runs {', '.join(f'{x:.2f}' for x in out[k]['gpu_ms'])}); "
              f"{out[k]['median_msegments']:7.0f} Msegments/s; shade {out[k]['median_shade_ms']:.2f} ms; {out[k]['segments']} segments", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
