"""What posing a skinned mesh on the device (ptmi_pose_skin) costs beside sending its records (ptmi_update_triangles), on grid_1m (the
1 M-triangle scene of bench.py's config 3) and cornell_spheres at 1920 x 1080, for skins that list all of the triangles and a
scattered 5 % of them, with 64 joints (the joint records in LDS) and 2 048 joints (read from global memory).

The yardstick is the path there was before, in the same process and in turn: ptmi_update_triangles over the span [lowest listed,
highest listed] with the skinned records, prepared beforehand (the host-side skinning that path needs as well is NOT counted). The
records are read back from the posed context (tests/test_gpu_skin.py holds them to the numpy model byte for byte; the first run is
held to it here as well, on the first and the last listed triangle).

Per scene, share and joint count: --warmup runs, then the median of --rounds runs of
  pose_ms     ptmi_skin_status.pose_ms of pose_skin (its refit included)
  update_ms   ptmi_scene_update_status.refit_ms of update_triangles over the span (its copy and refit included)
  refit_ms    ... of update_triangles with no records: the refit both paths end in, alone
Every run poses to other matrices, so no run finds its work done. The driver runs one worker process under `timeout`, writes --json
(default profiles/skin_cost.json) and prints the first section of profiles/README.md for pasting.

    python tools/skin_cost.py [--rounds 8] [--warmup 2] [--scenes grid_1m,cornell_spheres] [--json out.json] [--limit 480]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wgpu-path-tracing_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
JOINTS = (64, 2048)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return dict(median=med(xs), min=min(xs), max=max(xs), runs=list(xs))


def worker(a):
    from ptmi import native, scenes
    import skin_ref as ref
    import transform_ref as tref
    results = {}
    runs = a.warmup + a.rounds
    for name in a.scenes.split(","):
        sc = scenes.make(name)
        n = len(sc.tris)
        rng = np.random.default_rng(3)
        lists = {"5": np.sort(rng.choice(n, max(1, n // 20), replace=False)).astype(np.uint32), "100": np.arange(n, dtype=np.uint32)}
        out = {"triangles": n}
        with native.Context(0) as posed, native.Context(0) as updated:
            for c in (posed, updated):
                c.set_options(leaves=2, tree_builder=2)
                c.resize(W, H)
            for share, listed in lists.items():
                lo, hi = int(listed[0]), int(listed[-1])
                for nj in JOINTS:
                    corners = ref.random_corners(np.random.default_rng(4), len(listed), nj, 4, cover=True)
                    poses = [native.joint_ops([ref.joint(tref.affine(tref.rot_y(0.01 * (k + 1) + 1e-5 * j), shift=(0.001 * k, 0.0, 1e-6 * j)))
                                               for j in range(nj)]) for k in range(runs)]
                    posed.upload_scene(sc)
                    updated.upload_scene(sc)
                    posed.set_skin(listed, corners, nj)
                    p_ms, p_wall, u_ms, u_wall, r_ms = [], [], [], [], []
                    for k in range(runs):
                        t0 = time.perf_counter()
                        posed.pose_skin(poses[k])
                        p_wall.append((time.perf_counter() - t0) * 1e3)
                        p_ms.append(posed.skin_status().pose_ms)
                        records = posed.read_triangles(lo, hi - lo + 1)                    # prepared beforehand: not timed
                        if k == 0:
                            ends = np.array([0, len(listed) - 1])
                            some = ref.skinned(sc.tris, tref.rest_of(sc.tris), listed[ends], corners.reshape(-1, 3)[ends].reshape(-1), poses[0])
                            assert records[listed[ends] - lo].tobytes() == some[listed[ends]].tobytes()
                        t0 = time.perf_counter()
                        updated.update_triangles(lo, records)
                        u_wall.append((time.perf_counter() - t0) * 1e3)
                        u_ms.append(updated.scene_update_status().refit_ms)
                        updated.update_triangles(0, records[:0])                          # the refit alone
                        r_ms.append(updated.scene_update_status().refit_ms)
                        del records
                    w = a.warmup
                    out[f"{share}/{nj}"] = dict(listed=len(listed), span=hi - lo + 1, joints=nj, pose_ms=spread(p_ms[w:]),
                                                pose_wall_ms=spread(p_wall[w:]), update_ms=spread(u_ms[w:]), update_wall_ms=spread(u_wall[w:]),
                                                refit_ms=spread(r_ms[w:]), pose_bytes=96 * nj, update_bytes=(hi - lo + 1) * 128)
        results[name] = out
        print(name, json.dumps({k: {f: (v["median"] if isinstance(v, dict) else v) for f, v in r.items()} for k, r in out.items()
                                if isinstance(r, dict)}), file=sys.stderr, flush=True)
    print(json.dumps(results))


def readme(res, a):
    f = lambda s: f"{s['median']:.2f} ({s['min']:.2f} - {s['max']:.2f})"
    lines = ["# Posing a skinned mesh on the device (`ptmi_pose_skin`; `csrc/scene_skin.hip`, `tools/skin_cost.py`)", "",
             f"One process, MI355X, {W} x {H}; medians of {a.rounds} calls after {a.warmup} warm-up calls (smallest - largest), from the "
             "`*_ms` status fields (wall time of the call inside the library; every call ends in a device synchronise). The update path is "
             "`ptmi_update_triangles` over [lowest listed, highest listed] with the same records prepared beforehand; `refit` is that call "
             "with no records, the part both paths end in. 64 joints sit in LDS, 2 048 are read from global memory.", "",
             "| scene | listed | joints | pose ms | update ms, span | refit ms | refit share of pose | bytes sent, pose / update |",
             "|---|---|---|---|---|---|---|---|"]
    for name, r in res.items():
        for key, s in r.items():
            if not isinstance(s, dict):
                continue
            lines.append(f"| {name} | {s['listed']} ({key.split('/')[0]} %) | {s['joints']} | {f(s['pose_ms'])} | {f(s['update_ms'])} | "
                         f"{f(s['refit_ms'])} | {100 * s['refit_ms']['median'] / s['pose_ms']['median']:.0f} % | "
                         f"{s['pose_bytes']} / {s['update_bytes']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="grid_1m,cornell_spheres")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "skin_cost.json"))
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    ap.add_argument("--limit", type=int, default=480, help="seconds the worker may take")
    ap.add_argument("--worker", action="store_true", help="measure and print JSON (what the driver starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # a fresh process under its own time limit; a failure ends the run
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(a.rounds),
           "--warmup", str(a.warmup), "--scenes", a.scenes]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"the worker ended with status {p.returncode}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(a.json, "w") as f:
        json.dump(dict(rounds=a.rounds, warmup=a.warmup, width=W, height=H, scenes=res), f, indent=1)
    text = readme(res, a)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
