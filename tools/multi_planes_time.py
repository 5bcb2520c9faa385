#!/usr/bin/env python3
"""tools/multi_planes_time.py: what the fused planes gather (ptmi_multi_gather_planes, include/ptmi.h) costs beside the radiance
gather, on a one-GPU box: N = 4 contexts on the one device (PTMI_MULTI_LOOPBACK), 1920x1080, every plane on. After a warm-up, REPEATS
interleaved repeats of
  (a) ptmi_multi_gather: the output buffer alone, 16 bytes per pixel - the yardstick;
  (b) ptmi_multi_gather_planes of everything: output, ALBEDO, NORMAL, ID and moments, 72 bytes per pixel,
both through the one gather: one pack kernel per device but device 0, one copy per device, ONE unpack kernel (a library from before the
two were merged, named by PTMI_LIB, runs (a) with a pack on device 0 too and one unpack kernel per share). Each is timed by the
library's own events (ptmi_multi_gather_ms: pack + device copy + unpack). Both are pure copies, so (b)'s time per byte should not
exceed (a)'s; the margin (b) gets is (a)'s own max / min spread over the repeats.
Loopback times pack + device-to-device copy + unpack on ONE GPU: it says nothing about xGMI or RCCL."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wgpu-path-tracing_amd"))
from ptmi import layout, native, scenes  # noqa: E402

N, W, H, REPEATS = 4, 1920, 1080, 7
EVERYTHING = ("albedo", "normal", "id", "moments", "output")

with native.MultiContext([0] * N, loopback=True) as m:
    m.upload_scene(scenes.make("cornell"))
    m.resize(W, H)
    m.set_options(max_bounces=8, do_mis=1, frames_per_batch=2)
    m.set_aovs("albedo", "normal", "id")
    m.set_moments(True)
    m.dispatch(layout.make_camera(W, H), 2)
    m.synchronize()
    strip = int(m.options().tile_strip)
    # bytes that arrive on device 0: the rows of the other devices (its own are in place)
    rows_elsewhere = H - sum(1 for y in range(H) if (y // strip) % N == 0)
    bytes_a, bytes_b = rows_elsewhere * W * 16, rows_elsewhere * W * 72

    def time_a():
        m.gather()
        return m.gather_ms()

    def time_b():
        m.gather_planes(*EVERYTHING)
        return m.gather_ms()

    for _ in range(2):                                      # warm-up: first launches, first copies
        time_a(), time_b()
    a, b = [], []
    for _ in range(REPEATS):
        a.append(time_a())
        b.append(time_b())

med = lambda v: sorted(v)[len(v) // 2]
spread = max(a) / min(a)
ns_per_kb_a, ns_per_kb_b = med(a) * 1e6 / (bytes_a / 1024), med(b) * 1e6 / (bytes_b / 1024)
out = {
    "devices": N, "frame": [W, H], "tile_strip": strip, "repeats": REPEATS,
    "a_output_only": {"ms": [round(v, 4) for v in a], "median_ms": round(med(a), 4), "bytes": bytes_a, "ns_per_KiB": round(ns_per_kb_a, 2),
                      "max_over_min": round(spread, 3)},
    "b_all_planes": {"ms": [round(v, 4) for v in b], "median_ms": round(med(b), 4), "bytes": bytes_b, "ns_per_KiB": round(ns_per_kb_b, 2),
                     "max_over_min": round(max(b) / min(b), 3)},
    "b_per_byte_over_a_per_byte": round(ns_per_kb_b / ns_per_kb_a, 3),
    "b_within_a_spread": bool(ns_per_kb_b <= ns_per_kb_a * spread),
    "note": "loopback: pack + device copy + unpack on one GPU; nothing about xGMI",
}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out, indent=1))
