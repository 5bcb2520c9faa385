"""Camera projections (include/ptmi.h ptmi_set_projections) restated in numpy float32, sharing no code with the kernels
(csrc/pipeline.hip camera_dir / camera_ray, csrc/reproject.hip): the orthographic and the equirectangular camera ray, operation by
operation, and step 4 of ptmi_reproject for an orthographic `from`.

The rays use the oracle's RNG (pto_seed, pto_rand) and sincos (pto_sincos), the contract normalize3 (a fused dot, one correctly
rounded sqrt and 1/x, three multiplies) and the fused madd3 of the lens, as the kernels and the oracle's contract build do:

  uvx = (px / W) * 2 - 1, uvy = (py / H) * 2 - 1 at (px, py) = (x + jitter x, y + jitter y), or (x + 0.5, y + 0.5) for a centre ray
  orthographic   a = ((right * uvx) * ymag) * aspect, b = (up * uvy) * ymag, org0 = (position + a) + b, raw = forward
  equirect       lon = uvx * pi, lat = uvy * (pi * 0.5f), raw = (forward * (cl * co) + right * (cl * so)) + up * sl, org0 = position
  dir = normalize3(raw); the lens (aperture > 0, not for centre rays) is the pinhole's with org0 where position stands

fov0_cameras() turns (org0, raw) into the pinhole cameras the oracle renders the same rays with: position = org0, forward = raw,
fov = 0, everything else equal (the header states why; no component of raw may be a zero, which it asserts).

reproject_ortho() is tests/reproject_motion_ref.py's statement of step 4 with the three orthographic differences: dist = zf,
sx = (v . right) / (ymag * aspect), sy = (v . up) / ymag. With prev = None it is the pass with motion off.
"""
import numpy as np

from reproject_ref import DEFAULTS, MISS
from reproject_motion_ref import CARRIED, DISOCCLUDED, MISSED, moved_mask
from scene_update_ref import fmaf

f32 = np.float32
PERSPECTIVE, ORTHOGRAPHIC, EQUIRECT = 0, 1, 2
PI = f32(3.14159265359)


def projection_of(cam):
    """(kind, ymag) of a camera record's two projection words"""
    w = np.asarray(cam["_p3"], np.uint32)
    return int(w[0]), w[1:2].view(f32)[0]


def _fma(a, b, c):
    return np.asarray(fmaf(a, b, c), f32)


def normalize3(a):
    """a / sqrt(a . a): the dot fused as (x x + y y) + z z, then one reciprocal of the root and three multiplies"""
    a = np.asarray(a, f32)
    l2 = _fma(a[:, 2], a[:, 2], _fma(a[:, 1], a[:, 1], a[:, 0] * a[:, 0]))
    inv = (f32(1) / np.sqrt(l2)).astype(f32)
    return a * inv[:, None]


def _sincos(oracle, x):
    sc = np.array([oracle.sincos(v) for v in np.asarray(x, f32)], f32).reshape(-1, 2)
    return sc[:, 0], sc[:, 1]


def rays(oracle, cam, xs, ys, frames=None):
    """The camera rays of pixels (xs, ys) at `frames` (None: the centre rays, no jitter, no lens, no RNG) for an orthographic or
    equirectangular camera record. Returns dict(org0, raw: the ray before the lens and before normalize3; o, d: the ray; rng: the
    RNG state it leaves, uint32, zeros for centre rays), arrays of (n, 3) / (n,)."""
    kind, ymag = projection_of(cam)
    assert kind in (ORTHOGRAPHIC, EQUIRECT)
    xs, ys = np.asarray(xs, np.uint32).ravel(), np.asarray(ys, np.uint32).ravel()
    n = len(xs)
    W, H = f32(int(cam["width"])), f32(int(cam["height"]))
    fw, rt, up, pos = (np.asarray(cam[k], f32) for k in ("forward", "right", "up", "position"))
    aspect, aperture, focus = f32(cam["aspect"]), f32(cam["aperture"]), f32(cam["focus_distance"])
    draws, states = np.zeros((n, 4), f32), np.zeros((n, 4), np.uint32)
    if frames is None:
        jx = jy = f32(0.5)
    else:
        for i, (x, y, f) in enumerate(zip(xs, ys, np.asarray(frames, np.uint32).ravel())):
            states[i], _, draws[i] = oracle.rand(oracle.seed(int(x), int(y), int(f)), 4)
        jx, jy = draws[:, 0], draws[:, 1]
    px, py = xs.astype(f32) + jx, ys.astype(f32) + jy
    uvx, uvy = (px / W) * f32(2) - f32(1), (py / H) * f32(2) - f32(1)
    assert uvx.dtype == f32 and uvy.dtype == f32
    if kind == ORTHOGRAPHIC:
        a = ((rt[None, :] * uvx[:, None]) * ymag) * aspect
        b = (up[None, :] * uvy[:, None]) * ymag
        org0 = (pos[None, :] + a) + b
        raw = np.broadcast_to(fw, (n, 3)).copy()
    else:
        so, co = _sincos(oracle, uvx * PI)
        sl, cl = _sincos(oracle, uvy * (PI * f32(0.5)))
        raw = (fw[None, :] * (cl * co)[:, None] + rt[None, :] * (cl * so)[:, None]) + up[None, :] * sl[:, None]
        org0 = np.broadcast_to(pos, (n, 3)).copy()
    assert org0.dtype == f32 and raw.dtype == f32
    o, d, rng = org0.copy(), normalize3(raw), states[:, 1].copy()
    if frames is None:
        rng[:] = 0
    elif aperture > 0:
        focal = _fma(d, focus, org0)
        r = np.sqrt(draws[:, 2]) * aperture
        st, ct = _sincos(oracle, draws[:, 3] * f32(2) * PI)
        off = _fma(up[None, :], (r * st)[:, None], rt[None, :] * (r * ct)[:, None])
        o = org0 + off
        d = normalize3(focal - o)
        rng = states[:, 3].copy()
    assert o.dtype == f32 and d.dtype == f32
    return dict(org0=org0, raw=raw, o=o, d=d, rng=rng)


def fov0_cameras(cam, org0, raw):
    """per ray, the pinhole camera that sends every pixel along normalize3(raw) from org0: `cam` with position = org0, forward = raw,
    fov = 0 and zeroed projection words. No component of raw may be +-0: the pinhole's expression adds +0 to each."""
    assert (np.asarray(raw, f32) != 0).all(), "a zero component of a direction: rotate the camera basis"
    cams = np.repeat(np.asarray(cam).reshape(1), len(org0))
    cams["position"], cams["forward"], cams["fov"], cams["_p3"] = org0, raw, 0.0, 0
    return cams


def _dot3(v, b):
    b = np.asarray(b, f32)
    return v[:, 0] * b[0] + v[:, 1] * b[1] + v[:, 2] * b[2]


def reproject_ortho(snap, cam_from, o, d, t, tri, tri_material, max_history=0, depth_tolerance=0.0, match_ids=0, rows=None,
                    u=None, v=None, prev=None, cur=None, dirty=(0, 0)):
    """ptmi_reproject, step 4, for an orthographic cam_from (its ymag in the record). snap, o, d, t, tri, tri_material, rows and the
    three parameters as tests/reproject_ref.reproject takes them. prev (with u, v, cur, dirty as tests/reproject_motion_ref.reproject
    takes them): motion is on, the moved rule applies and the planes returned include 'motion'. Returns (planes, status)."""
    kind, ymag = projection_of(cam_from)
    assert kind == ORTHOGRAPHIC
    motion = prev is not None
    out_s, mom_s, nrm_s = (np.ascontiguousarray(snap[k], f32) for k in ("output", "moments", "normal"))
    alb_s = None if snap.get("albedo") is None else np.ascontiguousarray(snap["albedo"], f32)
    ids_s = None if snap.get("id") is None else np.ascontiguousarray(snap["id"], np.uint32)
    H, W = out_s.shape[:2]
    N = H * W
    mot_s = None if not motion else np.zeros((H, W, 4), f32) if snap.get("motion") is None else np.ascontiguousarray(snap["motion"], f32)
    rows = np.ones(H, bool) if rows is None else np.asarray(rows, bool)
    assert match_ids in (0, 1, 2) and not (match_ids == 2 and ids_s is None)
    compare = match_ids == 2 or (match_ids == 0 and ids_s is not None)
    cap = f32(max_history or DEFAULTS["max_history"])
    tol_rel = f32(depth_tolerance or DEFAULTS["depth_tolerance"])
    o, d, t = np.asarray(o, f32).reshape(N, 3), np.asarray(d, f32).reshape(N, 3), np.asarray(t, f32).reshape(N)
    tri = np.asarray(tri, np.uint32).reshape(N)
    tri_material = np.asarray(tri_material, np.uint32)
    aspect = f32(cam_from["aspect"])
    own = np.repeat(rows, W)
    hit = tri != MISS
    safe_tri = np.where(hit, tri, 0).astype(np.int64)
    mat = np.where(hit, tri_material[safe_tri], MISS).astype(np.uint32)

    with np.errstate(all="ignore"):
        P = o + t[:, None] * d
        moved = np.zeros(N, bool)
        if motion:
            u, v = (np.asarray(a, f32).reshape(N) for a in (u, v))
            moved = moved_mask(tri, prev, cur, dirty)
            pv = np.ascontiguousarray(prev, f32).reshape(-1, 3, 3)[safe_tri]
            e1, e2 = pv[:, 1] - pv[:, 0], pv[:, 2] - pv[:, 0]
            P = np.where(moved[:, None], (pv[:, 0] + u[:, None] * e1) + v[:, None] * e2, P)
        vec = P - np.asarray(cam_from["position"], f32)[None, :]
        zf = _dot3(vec, cam_from["forward"])
        dist = zf
        sx = _dot3(vec, cam_from["right"]) / (ymag * aspect)
        sy = _dot3(vec, cam_from["up"]) / ymag
        fx = (sx + f32(1)) * f32(0.5) * f32(W) - f32(0.5)
        fy = (sy + f32(1)) * f32(0.5) * f32(H) - f32(0.5)
        projects = hit & (zf > 0) & np.isfinite(fx) & np.isfinite(fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        tol = tol_rel * dist
        assert all(a.dtype == f32 for a in (P, vec, zf, sx, sy, fx, fy, x0, ax, ay, tol))

        sw, nmin = np.zeros(N, f32), np.full(N, np.inf, f32)
        acc = {k: np.zeros((N, c), f32) for k, c in (("output", 3), ("moments", 2), ("albedo", 4), ("normal", 3))}
        some = np.zeros(N, bool)
        for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
            qxf, qyf = x0 + f32(i), y0 + f32(j)
            ok = projects & (qxf >= 0) & (qxf < f32(W)) & (qyf >= 0) & (qyf < f32(H))
            qx, qy = np.where(ok, qxf, 0).astype(np.int64), np.where(ok, qyf, 0).astype(np.int64)
            ok &= rows[qy]
            qo, qm, qn = out_s[qy, qx], mom_s[qy, qx], nrm_s[qy, qx]
            qa = np.zeros((N, 4), f32) if alb_s is None else alb_s[qy, qx]
            ok &= (qm[:, 2] >= 1) & (qn[:, 3] > 0) & (np.abs(qn[:, 3] - dist) <= tol)
            ok &= np.isfinite(qo[:, :3]).all(axis=1) & np.isfinite(qm[:, :3]).all(axis=1) & np.isfinite(qn).all(axis=1)
            ok &= np.isfinite(qa).all(axis=1)
            if compare:
                ok &= ids_s[qy, qx, 1] == mat
            w = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
            assert w.dtype == f32
            sw = np.where(ok, sw + w, sw)
            for k, q in (("output", qo[:, :3]), ("moments", qm[:, :2]), ("albedo", qa), ("normal", qn[:, :3])):
                acc[k] = np.where(ok[:, None], acc[k] + w[:, None] * q, acc[k])
            nmin = np.where(ok & (qm[:, 2] < nmin), qm[:, 2], nmin)
            some |= ok
        carried = projects & some & (sw > 0)
        count = np.where(carried, np.where(nmin < cap, nmin, cap), f32(0)).astype(f32)
        mean = {k: (a / sw[:, None]).astype(f32) for k, a in acc.items()}
        py_, px_ = np.divmod(np.arange(N), W)
        mx, my = fx - px_.astype(f32), fy - py_.astype(f32)

    new = dict(output=np.zeros((N, 4), f32), moments=np.zeros((N, 4), f32), normal=np.zeros((N, 4), f32),
               albedo=np.zeros((N, 4), f32), id=np.full((N, 2), MISS, np.uint32), motion=np.zeros((N, 4), f32))
    c = carried
    new["output"][c, :3] = mean["output"][c]
    new["moments"][c, :2], new["moments"][c, 2] = mean["moments"][c], count[c]
    new["albedo"][c] = mean["albedo"][c]
    new["normal"][c, :3], new["normal"][c, 3] = mean["normal"][c], t[c]
    new["id"][hit, 0], new["id"][hit, 1] = tri[hit], mat[hit]
    new["motion"][projects, 0], new["motion"][projects, 1], new["motion"][projects, 2] = mx[projects], my[projects], dist[projects]
    new["motion"][:, 3] = np.where(carried, CARRIED, np.where(hit, DISOCCLUDED, MISSED)).astype(f32)

    planes = {}
    for k, s in (("output", out_s), ("moments", mom_s), ("normal", nrm_s), ("albedo", alb_s), ("id", ids_s), ("motion", mot_s)):
        if k == "motion" and not motion:
            continue
        if s is None:
            planes[k] = None
            continue
        p = s.copy().reshape(N, -1)
        p[own] = new[k][own]                          # rows of other contexts keep their contents
        planes[k] = p.reshape(s.shape)
    status = dict(carried=int((carried & own).sum()), disoccluded=int((hit & ~carried & own).sum()), missed=int((~hit & own).sum()),
                  samples=int(count[own].astype(np.uint64).sum()))
    if motion:
        status.update(moved=int((moved & own).sum()), moved_carried=int((moved & carried & own).sum()))
    return planes, status
