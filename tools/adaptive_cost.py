"""What adaptive sampling costs and buys (include/ptmi.h ptmi_dispatch_adaptive).

overhead: Msamples/s (path segments per second of device time, bench.py's metric, from gpu_ms) of bench.py's configs 1 and 2 at
full size, alternating on one context a plain 64-frame ptmi_dispatch and ONE adaptive round of step = 64 that lists every pixel
(min_frames above every count: nothing converges). Both trace the same number of paths; --rounds alternations after a warm-up.
buys: the same scenes rendered adaptively to --threshold (rounds of --step frames until a round lists nothing or --max-rounds)
against the uniform render with the same total samples (rounded up to whole frames): wall time of both, total samples, min / max /
median count and its histogram, and with --truth N the MSE of both against an N-frame render of the same build.

    python tools/adaptive_cost.py [--configs 1 2] [--rounds 5] [--threshold 0.05] [--step 16] [--max-frames 1024] [--truth 4096]
                                  [--skip-overhead] [--skip-buys] [--json out.json]
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402

CONFIGS = {  # bench.py CONFIGS, the single-device views
    1: dict(scene="cornell", width=1920, height=1080, fps=64, bounces=8, mis=1),
    2: dict(scene="cornell_spheres", width=1920, height=1080, fps=64, bounces=8, mis=1),
}


def msamples(ctx, cam, fps, adaptive):
    ctx.reset_stats()
    if adaptive:
        ctx.dispatch_adaptive(cam, 1, threshold=1.0, min_frames=1 << 20, max_frames=1 << 20, step=fps)
    else:
        ctx.dispatch(cam, fps)
    st = ctx.stats()
    return st.segments / (st.gpu_ms * 1e3), int(st.segments)


def overhead(ctx, cfg, rounds):
    W, H, fps = cfg["width"], cfg["height"], cfg["fps"]
    cam = layout.make_camera(W, H)                              # frame_index 0: both render frames 0 .. fps - 1
    ctx.set_options(max_bounces=cfg["bounces"], do_mis=cfg["mis"], frames_per_batch=0, timing=1)
    msamples(ctx, cam, fps, False), msamples(ctx, cam, fps, True)                 # warm-up of both paths
    runs = {"plain": [], "adaptive": []}
    for _ in range(rounds):
        for key in ("plain", "adaptive"):
            v, seg = msamples(ctx, cam, fps, key == "adaptive")
            runs[key].append(v)
            runs.setdefault("segments_" + key, seg)
    med = {k: float(np.median(runs[k])) for k in ("plain", "adaptive")}
    return dict(scene=cfg["scene"], msamples_plain=runs["plain"], msamples_adaptive=runs["adaptive"], median_plain=med["plain"],
                median_adaptive=med["adaptive"], ratio=med["adaptive"] / med["plain"],
                same_segments=runs["segments_plain"] == runs["segments_adaptive"])


def buys(ctx, cfg, a):
    W, H = cfg["width"], cfg["height"]
    cam = layout.make_camera(W, H)
    ctx.set_options(max_bounces=cfg["bounces"], do_mis=cfg["mis"], frames_per_batch=0, timing=0)
    prm = dict(threshold=a.threshold, step=a.step, min_frames=a.min_frames, max_frames=a.max_frames, neighbourhood=a.neighbourhood,
               floor=a.floor)
    ctx.dispatch_adaptive(cam, 1, **prm)                         # warm-up
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.dispatch_adaptive(cam, 1, **prm)
    rounds = 1
    while rounds < a.max_rounds:
        if ctx.adaptive_status().active == 0:
            break
        c = cam.copy()
        c["frame_index"] = 1
        ctx.dispatch_adaptive(c, 1, **prm)
        rounds += 1
    ctx.synchronize()
    t_ad = time.perf_counter() - t0
    img_ad = ctx.read_output()
    counts = ctx.read_moments()[..., 2].astype(np.int64)
    total = int(counts.sum())
    n_uni = -(-total // (W * H))
    ctx.dispatch(cam, n_uni)                                     # warm-up
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.dispatch(cam, n_uni)
    ctx.synchronize()
    t_uni = time.perf_counter() - t0
    img_uni = ctx.read_output()
    hist, edges = np.histogram(counts, bins=[0, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 1 << 24])
    out = dict(scene=cfg["scene"], params=prm, rounds=rounds, wall_s_adaptive=t_ad, wall_s_uniform=t_uni, samples=total,
               uniform_frames=n_uni, min_count=int(counts.min()), max_count=int(counts.max()), median_count=float(np.median(counts)),
               histogram={f"{int(lo)}-{int(hi) - 1}": int(n) for lo, hi, n in zip(edges[:-1], edges[1:], hist)})
    if a.truth:
        ctx.dispatch(cam, a.truth)
        gt = ctx.read_output()[..., :3].astype(np.float64)
        out["truth_frames"] = a.truth
        out["mse_adaptive"] = float(np.mean((img_ad[..., :3] - gt) ** 2))
        out["mse_uniform"] = float(np.mean((img_uni[..., :3] - gt) ** 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.0)
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--min-frames", type=int, default=0)
    ap.add_argument("--max-frames", type=int, default=1024)
    ap.add_argument("--neighbourhood", type=int, default=1)
    ap.add_argument("--max-rounds", type=int, default=256)
    ap.add_argument("--truth", type=int, default=0)
    ap.add_argument("--skip-overhead", action="store_true")
    ap.add_argument("--skip-buys", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"overhead": {}, "buys": {}}
    with native.Context(0) as ctx:
        for k in a.configs:
            cfg = CONFIGS[k]
            ctx.set_moments(False)
            ctx.upload_scene(scenes.make(cfg["scene"]))
            ctx.resize(cfg["width"], cfg["height"])
            ctx.set_moments(True)
            if not a.skip_overhead:
                out["overhead"][k] = overhead(ctx, cfg, a.rounds)
                print("overhead", k, out["overhead"][k], file=sys.stderr, flush=True)
            if not a.skip_buys:
                out["buys"][k] = buys(ctx, cfg, a)
                print("buys", k, out["buys"][k], file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
