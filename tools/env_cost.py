"""What environment lighting (ptmi_upload_environment) costs: bench.py's config 1 (Cornell, 1920x1080, 64 spp, 8 bounces, MIS) at
full size in three set-ups on one context, in alternating runs (none, lookup, sampled, none, ...): no sky (the kernels of before), a sky
that misses only look up (sample = 1: the ENV kernels, no extra light), and a sampled sky (one more light for next-event estimation,
the MIS weight carried per path). Each run is one timed 64-frame dispatch after a warm-up; reported are Msegments/s (path segments
per second of device time, bench.py's metric) and the shade kernel's milliseconds per dispatch (timing = 3).

    python tools/env_cost.py [--rounds 5] [--map 2048 1024] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402

CFG = dict(scene="cornell", width=1920, height=1080, fps=64, bounces=8, mis=1)      # bench.py CONFIGS[1]
SETUPS = ("none", "lookup", "sampled")


def measure(ctx, sky, setup, frame_index):
    if setup == "none":
        ctx.upload_environment(None)
    else:
        ctx.upload_environment(sky, intensity=0.2, sample=1 if setup == "lookup" else 0)
    W, H, fps = CFG["width"], CFG["height"], CFG["fps"]
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index), fps)          # warm-up (allocates the batch)
    ctx.reset_stats()
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index + fps), fps)
    st = ctx.stats()
    return st.segments / (st.gpu_ms * 1e3), st.shade_ms, st.segments


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--map", type=int, nargs=2, default=[2048, 1024])
    ap.add_argument("--json")
    a = ap.parse_args()
    sky = scenes.sky(a.map[0], a.map[1], "disc")
    runs = {k: [] for k in SETUPS}
    with native.Context(0) as ctx:
        ctx.upload_scene(scenes.make(CFG["scene"]))
        ctx.resize(CFG["width"], CFG["height"])
        ctx.set_options(max_bounces=CFG["bounces"], do_mis=CFG["mis"], frames_per_batch=0, timing=3)
        for r in range(a.rounds):
            for k in SETUPS:
                runs[k].append(measure(ctx, sky, k, 128 * r))
        ctx.upload_environment(None)
    out = {}
    for k in SETUPS:
        rate, shade = sorted(x[0] for x in runs[k]), sorted(x[1] for x in runs[k])
        out[k] = dict(msegments=[x[0] for x in runs[k]], shade_ms=[x[1] for x in runs[k]], segments=runs[k][-1][2],
                      median_msegments=rate[len(rate) // 2], median_shade_ms=shade[len(shade) // 2])
        print(f"{k:8s} {out[k]['median_msegments']:8.0f} Msegments/s (runs {', '.join(f'{x:.0f}' for x in out[k]['msegments'])}); "
              f"shade {out[k]['median_shade_ms']:.2f} ms per {CFG['fps']}-frame dispatch; {out[k]['segments']} segments", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
