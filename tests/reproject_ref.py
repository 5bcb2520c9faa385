"""ptmi_reproject (include/ptmi.h), step 4, restated in numpy float32, sharing no code with the kernel (csrc/reproject.hip).

Given the snapshot of the planes under the camera `from`, the centre rays of the camera `to`, their closest hits (t, tri), the
triangles' material indices and th = tan(from.fov * 0.5f), reproject() returns the planes the call leaves and its four counters.
Every expression is float32, evaluated left to right without FMA, in the order the header states it, for all pixels at once:

  miss (tri == 0xFFFFFFFF)   planes zero, ids 0xFFFFFFFF twice, count 0
  P = o + t d, v = P - from.position, zf = v . forward, dist = sqrt(v . v)
  not zf > 0                 disoccluded
  sx = (v . right) / (zf * th * aspect), sy = (v . up) / (zf * th)
  fx = (sx + 1) * 0.5 * W - 0.5, fy likewise with H; not finite: disoccluded
  x0 = floor(fx), ax = fx - x0, likewise y; taps (0,0), (1,0), (0,1), (1,1), w = (i ? ax : 1 - ax) * (j ? ay : 1 - ay)
  a tap is valid iff inside the image and in a row of the context, n_q = moments.z >= 1, t_q = normal.w > 0,
    |t_q - dist| <= depth_tolerance * dist, every snapshot float read for it finite, and (ids compared) its material == the hit's
  sw = sum of the valid weights; no valid tap or not sw > 0: disoccluded (planes zero, ids (tri, material), count 0)
  carried: output rgb, moments xy, albedo xyzw, normal xyz = (sum of w * value in tap order) / sw; normal.w = t; ids = (tri, material);
    output.w = moments.w = 0; count = min(min of the valid n_q, max_history), min(a, b) = a < b ? a : b

center_rays64() evaluates the centre rays' formula in float64, for the host tests and the 2e-6 bound of the GPU test.
"""
import numpy as np

f32 = np.float32
MISS = 0xFFFFFFFF
DEFAULTS = dict(max_history=32, depth_tolerance=0.02)


def center_rays64(cam):
    """origins (n, 3) and unit directions (n, 3) in float64, index y * W + x: the camera ray through the pixel centre, no lens"""
    W, H = int(cam["width"]), int(cam["height"])
    ys, xs = np.divmod(np.arange(W * H), W)
    uvx = (xs + 0.5) / W * 2.0 - 1.0
    uvy = (ys + 0.5) / H * 2.0 - 1.0
    th = np.tan(float(f32(cam["fov"]) * f32(0.5)))
    fw, rt, up = (np.asarray(cam[k], np.float64) for k in ("forward", "right", "up"))
    d = fw[None, :] + rt[None, :] * (uvx * th * float(cam["aspect"]))[:, None] + up[None, :] * (uvy * th)[:, None]
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    o = np.broadcast_to(np.asarray(cam["position"], np.float64), (W * H, 3)).copy()
    return o, d


def _dot(v, b):
    return v[:, 0] * f32(b[0]) + v[:, 1] * f32(b[1]) + v[:, 2] * f32(b[2])


def reproject(snap, cam_from, o, d, t, tri, tri_material, th, max_history=0, depth_tolerance=0.0, match_ids=0, rows=None):
    """snap: dict of (H, W, C) planes: 'output', 'moments', 'normal' float32 x 4; 'albedo' float32 x 4 or None; 'id' uint32 x 2 or None.
    o, d: (H * W, 3) float32 centre rays of the camera moved to; t (H * W,) float32, tri (H * W,) uint32 their closest hits.
    tri_material: the triangles' material_index. rows: boolean (H,), the context's rows (None: all). match_ids as in the header.
    Returns (planes: the same dict after the call, status: dict(carried, disoccluded, missed, samples))."""
    out_s, mom_s, nrm_s = (np.ascontiguousarray(snap[k], f32) for k in ("output", "moments", "normal"))
    alb_s = None if snap.get("albedo") is None else np.ascontiguousarray(snap["albedo"], f32)
    ids_s = None if snap.get("id") is None else np.ascontiguousarray(snap["id"], np.uint32)
    H, W = out_s.shape[:2]
    N = H * W
    rows = np.ones(H, bool) if rows is None else np.asarray(rows, bool)
    assert match_ids in (0, 1, 2) and not (match_ids == 2 and ids_s is None)
    compare = match_ids == 2 or (match_ids == 0 and ids_s is not None)
    cap = f32(max_history or DEFAULTS["max_history"])
    tol_rel = f32(depth_tolerance or DEFAULTS["depth_tolerance"])
    o, d, t = np.asarray(o, f32).reshape(N, 3), np.asarray(d, f32).reshape(N, 3), np.asarray(t, f32).reshape(N)
    tri = np.asarray(tri, np.uint32).reshape(N)
    tri_material = np.asarray(tri_material, np.uint32)
    th, aspect = f32(th), f32(cam_from["aspect"])
    own_row = np.repeat(rows, W)
    hit = tri != MISS
    mat = np.where(hit, tri_material[np.where(hit, tri, 0)], MISS).astype(np.uint32)

    with np.errstate(all="ignore"):
        P = o + t[:, None] * d
        v = P - np.asarray(cam_from["position"], f32)[None, :]
        zf = _dot(v, cam_from["forward"])
        dist = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        sx = _dot(v, cam_from["right"]) / (zf * th * aspect)
        sy = _dot(v, cam_from["up"]) / (zf * th)
        fx = (sx + f32(1)) * f32(0.5) * f32(W) - f32(0.5)
        fy = (sy + f32(1)) * f32(0.5) * f32(H) - f32(0.5)
        projects = hit & (zf > 0) & np.isfinite(fx) & np.isfinite(fy)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        tol = tol_rel * dist
        assert all(a.dtype == f32 for a in (P, v, zf, dist, sx, sy, fx, fy, x0, ax, tol))

        sw, nmin = np.zeros(N, f32), np.full(N, np.inf, f32)
        acc = {k: np.zeros((N, c), f32) for k, c in (("output", 3), ("moments", 2), ("albedo", 4), ("normal", 3))}
        any_valid = np.zeros(N, bool)
        for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
            qxf, qyf = x0 + f32(i), y0 + f32(j)
            valid = projects & (qxf >= 0) & (qxf < f32(W)) & (qyf >= 0) & (qyf < f32(H))
            qx, qy = np.where(valid, qxf, 0).astype(np.int64), np.where(valid, qyf, 0).astype(np.int64)
            valid &= rows[qy]
            qo, qm, qn = out_s[qy, qx], mom_s[qy, qx], nrm_s[qy, qx]
            qa = np.zeros((N, 4), f32) if alb_s is None else alb_s[qy, qx]
            valid &= (qm[:, 2] >= 1) & (qn[:, 3] > 0) & (np.abs(qn[:, 3] - dist) <= tol)
            valid &= np.isfinite(qo[:, :3]).all(axis=1) & np.isfinite(qm[:, :3]).all(axis=1) & np.isfinite(qn).all(axis=1)
            valid &= np.isfinite(qa).all(axis=1)
            if compare:
                valid &= ids_s[qy, qx, 1] == mat
            w = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
            assert w.dtype == f32
            sw = np.where(valid, sw + w, sw)
            for k, q in (("output", qo[:, :3]), ("moments", qm[:, :2]), ("albedo", qa), ("normal", qn[:, :3])):
                acc[k] = np.where(valid[:, None], acc[k] + w[:, None] * q, acc[k])
            nmin = np.where(valid & (qm[:, 2] < nmin), qm[:, 2], nmin)
            any_valid |= valid
        carried = projects & any_valid & (sw > 0)
        count = np.where(carried, np.where(nmin < cap, nmin, cap), f32(0)).astype(f32)
        mean = {k: (a / sw[:, None]).astype(f32) for k, a in acc.items()}

    zero = f32(0)
    new = dict(output=np.zeros((N, 4), f32), moments=np.zeros((N, 4), f32), normal=np.zeros((N, 4), f32),
               albedo=np.zeros((N, 4), f32), id=np.full((N, 2), MISS, np.uint32))
    c = carried
    new["output"][c, :3] = mean["output"][c]
    new["moments"][c, :2], new["moments"][c, 2] = mean["moments"][c], count[c]
    new["albedo"][c] = mean["albedo"][c]
    new["normal"][c, :3], new["normal"][c, 3] = mean["normal"][c], t[c]
    new["id"][hit, 0], new["id"][hit, 1] = tri[hit], mat[hit]
    assert new["output"][:, 3].max(initial=zero) == 0

    planes = {}
    for k, s in (("output", out_s), ("moments", mom_s), ("normal", nrm_s), ("albedo", alb_s), ("id", ids_s)):
        if s is None:
            planes[k] = None
            continue
        p = s.copy().reshape(N, -1)
        p[own_row] = new[k][own_row]                 # rows of other contexts keep their contents
        planes[k] = p.reshape(s.shape)
    status = dict(carried=int((carried & own_row).sum()), disoccluded=int((hit & ~carried & own_row).sum()),
                  missed=int((~hit & own_row).sum()), samples=int(count[own_row].astype(np.uint64).sum()))
    return planes, status
