"""What posing a morphed mesh on the device (ptmi_pose_morph) costs beside sending its records (ptmi_update_triangles), on grid_1m (the
1 M-triangle scene of bench.py's config 3) and cornell_spheres at 1920 x 1080.

The yardstick is the path there was before, in the same process and in turn: ptmi_update_triangles over the span [lowest listed,
highest listed] with the morphed records, prepared beforehand (the host-side morphing that path needs as well is NOT counted). The
records are read back from the posed context (tests/test_gpu_morph.py holds them to the numpy model byte for byte; the first run is held
to it here as well, on the first and the last listed triangle).

Rows, per scene:
  a       every triangle listed, 8 records per row (8 targets), 8 non-zero weights
  b       the same table, 1 non-zero weight of 8: seven records of every row are skipped before their 96 bytes are loaded
  c       a scattered 5 % listed, 8 records per row, 8 non-zero weights
  d       the triangles of a (grid_1m: of c) listed by the morph AND by a skin of 64 joints: pose_morph + pose_skin against pose_skin
          alone. The morph leg writes the skin's rest rows and runs no refit.
Row b run again with --lib pointing at a build with -DPT_MORPH_LOAD_FIRST (make variant NAME=loadfirst EXTRA=-DPT_MORPH_LOAD_FIRST)
gives the kernel that loads a record before it knows its weight; --variant names the result in the JSON.

Per row: --warmup runs, then the median of --rounds runs of
  pose_ms     ptmi_morph_status.pose_ms of pose_morph (its refit included), and the wall time of the call seen from Python
  update_ms   ptmi_scene_update_status.refit_ms of update_triangles over the span (its copy and refit included), and its wall time
  refit_ms    ... of update_triangles with no records: the refit both paths end in, alone
Every run poses to other weights, so no run finds its work done. The driver runs one worker process under `timeout`, writes --json
(default profiles/morph_cost.json) and prints the first section of profiles/README.md for pasting.

    python tools/morph_cost.py [--rounds 8] [--warmup 2] [--scenes grid_1m,cornell_spheres] [--json out.json] [--limit 480]
                               [--lib other/libptmi.so --variant load_first --rows b]
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
TARGETS, JOINTS = 8, 64


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return dict(median=med(xs), min=min(xs), max=max(xs), runs=list(xs))


def weights_of(k, active):
    w = np.zeros(TARGETS, np.float32)
    w[:active] = 0.2 + 0.01 * (k + 1) + 0.001 * np.arange(active)
    return np.roll(w, k % TARGETS)


def worker(a):
    from ptmi import native, scenes
    import morph_ref as ref
    import skin_ref as sref
    import transform_ref as tref
    results = {}
    runs = a.warmup + a.rounds
    wanted = a.rows.split(",")
    for name in a.scenes.split(","):
        sc = scenes.make(name)
        n = len(sc.tris)
        rng = np.random.default_rng(3)
        some = np.sort(rng.choice(n, max(1, n // 20), replace=False)).astype(np.uint32)
        every = np.arange(n, dtype=np.uint32)
        rest = tref.rest_of(sc.tris)
        out = {"triangles": n}
        with native.Context(0) as posed, native.Context(0) as updated:
            for c in (posed, updated):
                c.set_options(leaves=2, tree_builder=2)
                c.resize(W, H)
            tables = {}
            for row, listed, active in (("a", every, 8), ("b", every, 1), ("c", some, 8)):
                if row not in wanted:
                    continue
                lo, hi = int(listed[0]), int(listed[-1])
                if len(listed) not in tables:
                    tables = {len(listed): ref.table(np.random.default_rng(4), len(listed), TARGETS, (TARGETS,), dv=0.002, dn=0.1)}
                row_start, deltas = tables[len(listed)]
                posed.upload_scene(sc)
                updated.upload_scene(sc)
                posed.set_morph(listed, row_start, deltas, TARGETS)
                p_ms, p_wall, u_ms, u_wall, r_ms = [], [], [], [], []
                for k in range(runs):
                    w = weights_of(k, active)
                    t0 = time.perf_counter()
                    posed.pose_morph(w)
                    p_wall.append((time.perf_counter() - t0) * 1e3)
                    p_ms.append(posed.morph_status().pose_ms)
                    records = posed.read_triangles(lo, hi - lo + 1)                    # prepared beforehand: not timed
                    if k == 0:
                        ends = np.array([0, len(listed) - 1])
                        rs = np.array([0, TARGETS, 2 * TARGETS], np.uint32)
                        d2 = np.concatenate([deltas[:TARGETS], deltas[-TARGETS:]])
                        model = ref.morphed(sc.tris, rest, listed[ends], rs, d2, w)
                        assert records[listed[ends] - lo].tobytes() == model[listed[ends]].tobytes()
                    t0 = time.perf_counter()
                    updated.update_triangles(lo, records)
                    u_wall.append((time.perf_counter() - t0) * 1e3)
                    u_ms.append(updated.scene_update_status().refit_ms)
                    updated.update_triangles(0, records[:0])                          # the refit alone
                    r_ms.append(updated.scene_update_status().refit_ms)
                    del records
                s = a.warmup
                out[row] = dict(listed=len(listed), span=hi - lo + 1, records=len(deltas), active=active, pose_ms=spread(p_ms[s:]),
                                pose_wall_ms=spread(p_wall[s:]), update_ms=spread(u_ms[s:]), update_wall_ms=spread(u_wall[s:]),
                                refit_ms=spread(r_ms[s:]), pose_bytes=4 * TARGETS, update_bytes=(hi - lo + 1) * 128)
            if "d" in wanted:
                listed = every if n <= 100000 else some
                if len(listed) not in tables:
                    tables = {len(listed): ref.table(np.random.default_rng(4), len(listed), TARGETS, (TARGETS,), dv=0.002, dn=0.1)}
                row_start, deltas = tables[len(listed)]
                corners = sref.random_corners(np.random.default_rng(5), len(listed), JOINTS, 4, cover=True)
                poses = [native.joint_ops([sref.joint(tref.affine(tref.rot_y(0.01 * (k + 1) + 1e-5 * j), shift=(0.001 * k, 0.0, 1e-6 * j)))
                                           for j in range(JOINTS)]) for k in range(runs)]
                posed.upload_scene(sc)
                posed.set_skin(listed, corners, JOINTS)
                posed.set_morph(listed, row_start, deltas, TARGETS)
                assert posed.morph_status().n_in_skin == len(listed)
                m_ms, m_wall, s_ms, both_wall, alone_ms, alone_wall = [], [], [], [], [], []
                for k in range(runs):
                    before = posed.scene_update_status().updates
                    t0 = time.perf_counter()
                    posed.pose_morph(weights_of(k, 8))
                    t1 = time.perf_counter()
                    posed.pose_skin(poses[k])
                    t2 = time.perf_counter()
                    assert posed.scene_update_status().updates == before + 1          # one refit for the two calls
                    m_ms.append(posed.morph_status().pose_ms)
                    m_wall.append((t1 - t0) * 1e3)
                    s_ms.append(posed.skin_status().pose_ms)
                    both_wall.append((t2 - t0) * 1e3)
                    t0 = time.perf_counter()
                    posed.pose_skin(poses[(k + 1) % runs])                             # the skin alone, to other matrices
                    alone_wall.append((time.perf_counter() - t0) * 1e3)
                    alone_ms.append(posed.skin_status().pose_ms)
                s = a.warmup
                out["d"] = dict(listed=len(listed), records=len(deltas), joints=JOINTS, morph_ms=spread(m_ms[s:]), morph_wall_ms=spread(m_wall[s:]),
                                skin_after_morph_ms=spread(s_ms[s:]), both_wall_ms=spread(both_wall[s:]), skin_alone_ms=spread(alone_ms[s:]),
                                skin_alone_wall_ms=spread(alone_wall[s:]))
        results[name] = out
        print(name, json.dumps({k: {f: (v["median"] if isinstance(v, dict) else v) for f, v in r.items()} for k, r in out.items()
                                if isinstance(r, dict)}), file=sys.stderr, flush=True)
    print(json.dumps(results))


def readme(res, a):
    f = lambda s: f"{s['median']:.2f} ({s['min']:.2f} - {s['max']:.2f})"
    lines = ["# Posing a morphed mesh on the device (`ptmi_pose_morph`; `csrc/scene_morph.hip`, `tools/morph_cost.py`)", "",
             f"One process, MI355X, {W} x {H}; medians of {a.rounds} calls after {a.warmup} warm-up calls (smallest - largest). `ms`: the "
             "`*_ms` status fields (wall time of the call inside the library; every call ends in a device synchronise); `wall`: the call "
             "seen from Python. The update path is `ptmi_update_triangles` over [lowest listed, highest listed] with the same records "
             "prepared beforehand; `refit` is that call with no records, the part both paths end in. 8 targets, 8 records per row.", "",
             "| scene | row | listed | non-zero weights | pose ms | pose wall | update ms, span | update wall | refit ms | refit share of pose |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in res.items():
        for key in ("a", "b", "c"):
            s = r.get(key)
            if s:
                lines.append(f"| {name} | {key} | {s['listed']} | {s['active']} of 8 | {f(s['pose_ms'])} | {f(s['pose_wall_ms'])} | "
                             f"{f(s['update_ms'])} | {f(s['update_wall_ms'])} | {f(s['refit_ms'])} | "
                             f"{100 * s['refit_ms']['median'] / s['pose_ms']['median']:.0f} % |")
    lines += ["", "| scene | row | listed by both | pose_morph ms | pose_skin after it ms | both, wall | pose_skin alone ms | alone, wall |",
              "|---|---|---|---|---|---|---|---|"]
    for name, r in res.items():
        s = r.get("d")
        if s:
            lines.append(f"| {name} | d | {s['listed']} | {f(s['morph_ms'])} | {f(s['skin_after_morph_ms'])} | {f(s['both_wall_ms'])} | "
                         f"{f(s['skin_alone_ms'])} | {f(s['skin_alone_wall_ms'])} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="grid_1m,cornell_spheres")
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "morph_cost.json"))
    ap.add_argument("--readme", help="write the README section here instead of printing it")
    ap.add_argument("--limit", type=int, default=480, help="seconds the worker may take")
    ap.add_argument("--lib", help="another build of the library (PTMI_LIB) for the worker")
    ap.add_argument("--variant", default="skip_before_load", help="what the JSON calls this build")
    ap.add_argument("--worker", action="store_true", help="measure and print JSON (what the driver starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    # a fresh process under its own time limit; a failure ends the run
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(a.rounds),
           "--warmup", str(a.warmup), "--scenes", a.scenes, "--rows", a.rows]
    env = dict(os.environ, PTMI_LIB=os.path.abspath(a.lib)) if a.lib else None
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    if p.returncode != 0:
        sys.exit(f"the worker ended with status {p.returncode}")
    res = json.loads(p.stdout.strip().splitlines()[-1])
    with open(a.json, "w") as f:
        json.dump(dict(rounds=a.rounds, warmup=a.warmup, width=W, height=H, variant=a.variant, scenes=res), f, indent=1)
    text = readme(res, a)
    if a.readme:
        with open(a.readme, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
