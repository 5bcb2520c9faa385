"""What the first-hit planes (ptmi_set_aovs) cost: Msamples/s (path segments per second of device time, bench.py's metric) of
bench.py's configs 1 and 2 at full size with the planes off and with all three on, in alternating runs on one context (off, on, off,
on, ...), each run one timed 64-frame dispatch after a warm-up.

    python tools/aov_cost.py [--configs 1 2] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402

CONFIGS = {  # bench.py CONFIGS, the single-device views
    1: dict(scene="cornell", width=1920, height=1080, fps=64, bounces=8, mis=1),
    2: dict(scene="cornell_spheres", width=1920, height=1080, fps=64, bounces=8, mis=1),
}


def measure(ctx, cfg, aovs, frame_index):
    ctx.set_aovs(*aovs)
    W, H, fps = cfg["width"], cfg["height"], cfg["fps"]
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index), fps)          # warm-up (allocates the batch)
    ctx.reset_stats()
    ctx.dispatch(layout.make_camera(W, H, frame_index=frame_index + fps), fps)
    st = ctx.stats()
    return st.segments / (st.gpu_ms * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {}
    with native.Context(0) as ctx:
        for k in a.configs:
            cfg = CONFIGS[k]
            ctx.set_aovs()
            ctx.upload_scene(scenes.make(cfg["scene"]))
            ctx.resize(cfg["width"], cfg["height"])
            ctx.set_options(max_bounces=cfg["bounces"], do_mis=cfg["mis"], frames_per_batch=0, timing=1)
            runs = {"off": [], "on": []}
            for r in range(a.rounds):
                for key, aovs in (("off", ()), ("on", ("albedo", "normal", "id"))):
                    runs[key].append(measure(ctx, cfg, aovs, 128 * r))
            med = {key: sorted(v)[len(v) // 2] for key, v in runs.items()}
            out[k] = dict(scene=cfg["scene"], msamples_off=runs["off"], msamples_on=runs["on"],
                          median_off=med["off"], median_on=med["on"], cost_pct=100.0 * (med["off"] / med["on"] - 1.0))
            print(f"config {k} ({cfg['scene']}, {cfg['width']}x{cfg['height']}, {cfg['fps']} spp): off "
                  f"{', '.join(f'{x:.0f}' for x in runs['off'])}  on {', '.join(f'{x:.0f}' for x in runs['on'])} Msamples/s; "
                  f"median cost {out[k]['cost_pct']:+.1f} %", flush=True)
        ctx.set_aovs()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
