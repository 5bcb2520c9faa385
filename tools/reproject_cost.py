"""What a reprojection costs beside the work it saves (include/ptmi.h ptmi_reproject).

At 1920x1080 on the Cornell box, with HIP events on the context's stream (a caller-owned torch stream, so that the events and the
library's work share it): the time of one ptmi_reproject after a sideways camera move (snapshot copies, centre rays, closest hits,
the reprojection kernel), and the time of one 1-frame ptmi_dispatch at the same size - the work one carried sample per pixel saves.
Each is the median of --reps runs after a warm-up; every reprojection starts from the same freshly rendered planes.

    python tools/reproject_cost.py [--size 1920x1080] [--frames 8] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))

from ptmi import layout, native, scenes  # noqa: E402


def timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=8, help="frames accumulated before the move")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    cam_from = layout.make_camera(W, H)
    cam_to = layout.make_camera(W, H, position=(0.3, 1.0, 2.8))
    stream = torch.cuda.Stream()
    with native.Context(0) as ctx:
        ctx.set_stream(stream.cuda_stream)
        ctx.upload_scene(scenes.make("cornell"))
        ctx.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, timing=0)
        ctx.resize(W, H)
        ctx.set_aovs("albedo", "normal", "id")
        ctx.set_moments(True)
        rp, one = [], []
        for rep in range(a.reps + 1):                         # the first of each is the warm-up (it allocates)
            ctx.dispatch(cam_from, a.frames)
            ms = timed(torch, stream, lambda: ctx.reproject(cam_from, cam_to))
            st = ctx.reproject_status().as_dict()
            cam = cam_to.copy()
            cam["frame_index"] = a.frames
            ms1 = timed(torch, stream, lambda: ctx.dispatch(cam, 1))
            if rep:
                rp.append(ms)
                one.append(ms1)
        ctx.synchronize()
        ctx.set_stream(0)
    rp.sort()
    one.sort()
    out = dict(width=W, height=H, frames=a.frames, reps=a.reps, status=st, reproject_ms=rp[len(rp) // 2], reproject_min_ms=rp[0],
               reproject_max_ms=rp[-1], one_frame_dispatch_ms=one[len(one) // 2], one_frame_min_ms=one[0], one_frame_max_ms=one[-1])
    print(f"{W}x{H} cornell, {a.frames} frames accumulated, {a.reps} runs: ptmi_reproject median {out['reproject_ms']:.3f} ms "
          f"(min {rp[0]:.3f}, max {rp[-1]:.3f}); one 1-frame ptmi_dispatch median {out['one_frame_dispatch_ms']:.3f} ms "
          f"(min {one[0]:.3f}, max {one[-1]:.3f}); carried {st['carried']}, disoccluded {st['disoccluded']}, missed {st['missed']} "
          f"of {W * H} pixels", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
