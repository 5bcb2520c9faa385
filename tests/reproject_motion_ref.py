"""ptmi_reproject with motion on (include/ptmi.h, ptmi_set_motion): step 4 with the moved rule and the motion plane, restated in numpy
float32, sharing no code with the kernel (csrc/reproject.hip k_reproject<true>) and none of step 4 with tests/reproject_ref.py (the host
test holds the two models against each other where they must agree: nothing moved).

  MOVED (a hit on triangle tri)   first <= tri < first + count of the dirty range, and one of the nine previous-position floats of
                                  tri differs in its bits from the current v0, v1, v2
  a MOVED hit                     e1 = v1p - v0p, e2 = v2p - v0p, Pprev = (v0p + u * e1) + v * e2 per component, float32, no FMA;
                                  v = Pprev - from.position. Every other hit: P = o + t d, v = P - from.position.
  then, as without motion         zf, dist, sx, sy, fx, fy, the four taps and their tests, the blends, the count, normal.w = t (new hit)
  motion plane                    x = fx - px, y = fy - py, z = dist, w = 0 / 1 / 2 carried / disoccluded / missed; x = y = z = 0 on
                                  a miss, where not zf > 0, and where fx or fy is not finite

Every expression is float32, evaluated left to right, for all pixels at once."""
import numpy as np

from reproject_ref import DEFAULTS, MISS

f32 = np.float32
CARRIED, DISOCCLUDED, MISSED = 0, 1, 2


def _dot3(v, b):
    b = np.asarray(b, f32)
    return v[:, 0] * b[0] + v[:, 1] * b[1] + v[:, 2] * b[2]


def moved_mask(tri, prev, cur, dirty):
    """per hit: the triangle lies in the dirty range (first, count) and a previous position differs in its bits from the current one"""
    tri = np.asarray(tri, np.uint32)
    first, count = int(dirty[0]), int(dirty[1])
    prev = np.ascontiguousarray(prev, f32).reshape(-1, 9)
    cur = np.ascontiguousarray(cur, f32).reshape(-1, 9)
    assert prev.shape == cur.shape
    differs = (prev.view(np.uint32) != cur.view(np.uint32)).any(axis=1)
    t64 = tri.astype(np.int64)
    inside = (tri != MISS) & (t64 >= first) & (t64 < first + count) & (t64 < len(cur))
    return inside & differs[np.where(inside, t64, 0)]


def reproject(snap, cam_from, o, d, t, tri, u, v, tri_material, th, prev, cur, dirty, max_history=0, depth_tolerance=0.0, match_ids=0,
              rows=None):
    """snap: the planes under cam_from as tests/reproject_ref.reproject takes them, and optionally 'motion' (H, W, 4), what the motion
    plane held (rows of other contexts keep it; absent: zeros). o, d (H * W, 3), t, u, v (H * W,) float32, tri (H * W,) uint32: the
    centre rays of the camera moved to and their hits as ptmi_debug_intersect reports them. prev, cur: (n_tris, 3, 3) float32, the
    previous and the current v0, v1, v2. dirty: (first, count). Returns (planes with 'motion', status with moved and moved_carried)."""
    out_s, mom_s, nrm_s = (np.ascontiguousarray(snap[k], f32) for k in ("output", "moments", "normal"))
    alb_s = None if snap.get("albedo") is None else np.ascontiguousarray(snap["albedo"], f32)
    ids_s = None if snap.get("id") is None else np.ascontiguousarray(snap["id"], np.uint32)
    H, W = out_s.shape[:2]
    N = H * W
    mot_s = np.zeros((H, W, 4), f32) if snap.get("motion") is None else np.ascontiguousarray(snap["motion"], f32)
    rows = np.ones(H, bool) if rows is None else np.asarray(rows, bool)
    assert match_ids in (0, 1, 2) and not (match_ids == 2 and ids_s is None)
    compare = match_ids == 2 or (match_ids == 0 and ids_s is not None)
    cap = f32(max_history or DEFAULTS["max_history"])
    tol_rel = f32(depth_tolerance or DEFAULTS["depth_tolerance"])
    o, d = np.asarray(o, f32).reshape(N, 3), np.asarray(d, f32).reshape(N, 3)
    t, u, v = (np.asarray(a, f32).reshape(N) for a in (t, u, v))
    tri = np.asarray(tri, np.uint32).reshape(N)
    tri_material = np.asarray(tri_material, np.uint32)
    th, aspect = f32(th), f32(cam_from["aspect"])
    own = np.repeat(rows, W)
    hit = tri != MISS
    safe_tri = np.where(hit, tri, 0).astype(np.int64)
    mat = np.where(hit, tri_material[safe_tri], MISS).astype(np.uint32)
    moved = moved_mask(tri, prev, cur, dirty)
    pv = np.ascontiguousarray(prev, f32).reshape(-1, 3, 3)[safe_tri]              # (N, vertex, axis)

    with np.errstate(all="ignore"):
        P_static = o + t[:, None] * d
        e1, e2 = pv[:, 1] - pv[:, 0], pv[:, 2] - pv[:, 0]
        P_prev = (pv[:, 0] + u[:, None] * e1) + v[:, None] * e2
        assert P_static.dtype == f32 and P_prev.dtype == f32
        P = np.where(moved[:, None], P_prev, P_static)
        vec = P - np.asarray(cam_from["position"], f32)[None, :]
        zf = _dot3(vec, cam_from["forward"])
        dist = np.sqrt(vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1] + vec[:, 2] * vec[:, 2])
        sx = _dot3(vec, cam_from["right"]) / (zf * th * aspect)
        sy = _dot3(vec, cam_from["up"]) / (zf * th)
        fx = (sx + f32(1)) * f32(0.5) * f32(W) - f32(0.5)
        fy = (sy + f32(1)) * f32(0.5) * f32(H) - f32(0.5)
        projects = hit & (zf > 0) & np.isfinite(fx) & np.isfinite(fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        tol = tol_rel * dist
        assert all(a.dtype == f32 for a in (vec, zf, dist, sx, sy, fx, fy, x0, ax, ay, tol))

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
        ys, xs = np.divmod(np.arange(N), W)
        mx, my = fx - xs.astype(f32), fy - ys.astype(f32)
        assert mx.dtype == f32 and my.dtype == f32

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
        if s is None:
            planes[k] = None
            continue
        p = s.copy().reshape(N, -1)
        p[own] = new[k][own]                          # rows of other contexts keep their contents
        planes[k] = p.reshape(s.shape)
    status = dict(carried=int((carried & own).sum()), disoccluded=int((hit & ~carried & own).sum()), missed=int((~hit & own).sum()),
                  samples=int(count[own].astype(np.uint64).sum()), moved=int((moved & own).sum()),
                  moved_carried=int((moved & carried & own).sum()))
    return planes, status
