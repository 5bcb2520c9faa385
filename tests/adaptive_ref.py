"""Adaptive sampling (include/ptmi.h ptmi_dispatch_adaptive) restated in numpy, sharing no code with the kernels.

Every pixel is at its own frame index n = moments.z. A round selects, then every active pixel receives its frames n .. n + step - 1,
folded in ascending order with the output buffer's rule (frame 0 overwrites, frame f mixes with weight 1 / (f + 1) through
mix(a, b, t) = fma(b, t, a * (1 - t)), the FMA emulated in float64 as tests/denoise_ref.py does).

  select  with (m1, m2, n) = moments.xyz in float32, left to right, max(a, b) = (a < b ? b : a):
            var = max(m2 - m1 * m1, 0), e = threshold * max(m1, floor), bound = e * e * n
          noisy  = n < min_frames, or n < max_frames and not var <= bound
          active = noisy (neighbourhood 0), or own n < max_frames and (noisy or one of the 8 neighbours inside the context's rows
          and the image is noisy) (neighbourhood 1).
  run     keeps an image, a moments plane (hence the counts) and what the device counters would say; the per-path radiance of a
          (pixel, frame) comes from Oracle.trace_path, which agrees with the kernels bit for bit.
  run_planes  the same rule over whole planes, for frames too large for run's loop over pixels: select, then one Oracle.trace_paths
          call per round and frame offset for all listed pixels, then fold_listed. tests/test_adaptive_host.py holds the two equal
          bit for bit; run stays as the statement of the rule.
"""
import numpy as np

f32 = np.float32
DEFAULTS = dict(floor=1.0, min_frames=16, max_frames=4096, step=16, neighbourhood=0)


def resolve(params):
    """the parameters with the library's defaults in place of zeros / missing keys"""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k == "threshold" or v:
            p[k] = v
    assert p["threshold"] > 0
    return p


def _max(a, b):
    return np.where(a < b, b, a).astype(np.float32)


def noisy(moments, params):
    p = resolve(params)
    m = np.asarray(moments, np.float32)
    m1, m2, n = m[..., 0], m[..., 1], m[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        var = _max(m2 - m1 * m1, f32(0))
        e = f32(p["threshold"]) * _max(m1, f32(p["floor"]))
        bound = e * e * n
        return (n < f32(p["min_frames"])) | ((n < f32(p["max_frames"])) & ~(var <= bound))


def rows_mask(H, rows):
    """rows: None (all), a boolean array of H, or an iterable of row numbers -> boolean array of H"""
    if rows is None:
        return np.ones(H, bool)
    rows = np.asarray(rows)
    if rows.dtype == bool:
        return rows.copy()
    m = np.zeros(H, bool)
    m[rows] = True
    return m


def band_rows(H, y0=0, y1=0, parts=1, part=0, strip=1):
    """the rows of a context as ptmi_options' tile_y0 / tile_y1 / tile_parts / tile_part / tile_strip deal them"""
    y1 = min(y1, H) if y1 else H
    m = np.zeros(H, bool)
    for y in range(y0, y1):
        m[y] = parts <= 1 or ((y - y0) // max(strip, 1)) % parts == part
    return m


def select(moments, params, rows=None):
    """(H, W, 4) moments -> (H, W) bool: the pixels that receive frames this round"""
    p = resolve(params)
    m = np.asarray(moments, np.float32)
    H, W = m.shape[:2]
    inside = rows_mask(H, rows)[:, None] & np.ones((H, W), bool)
    nz = noisy(m, p) & inside
    if not p["neighbourhood"]:
        return nz
    near = nz.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.zeros_like(nz)
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            sh[yd, xd] = nz[ys, xs]
            near |= sh
    return near & inside & (m[..., 2] < f32(p["max_frames"]))


def _mix(a, b, t):
    t = np.asarray(t, np.float32)
    p = np.asarray(a, np.float32) * (f32(1) - t)
    return (np.asarray(b, np.float32).astype(np.float64) * np.float64(t) + p.astype(np.float64)).astype(np.float32)


def fold_pixel(rgb, mom, L, frame):
    """one frame's per-path radiance L (3,) into a pixel's radiance (3,) and moments (4,)"""
    c = np.fmin(np.asarray(L, np.float32), f32(2.5))
    l = f32(0.2126) * c[0] + f32(0.7152) * c[1] + f32(0.0722) * c[2]
    m = np.array([l, l * l], np.float32)
    if frame > 0:
        t = f32(1) / f32(frame + 1)
        c = _mix(rgb, c, t)
        m = _mix(mom[:2], m, t)
    return c, np.array([m[0], m[1], f32(frame + 1), f32(0)], np.float32)


class State:
    """image (H, W, 4), moments (H, W, 4); active: list of the rounds' list lengths; paths / segments: what ptmi_stats would add"""

    def __init__(self, H, W, image=None, moments=None):
        self.image = np.zeros((H, W, 4), np.float32) if image is None else np.array(image, np.float32)
        self.moments = np.zeros((H, W, 4), np.float32) if moments is None else np.array(moments, np.float32)
        self.active, self.paths, self.segments, self.rounds = [], 0, 0, 0

    @property
    def counts(self):
        return self.moments[..., 2].astype(np.uint32)


def run(oracle, scene, cam, params, rounds, rows=None, state=None, restart=True, max_bounces=8, do_mis=1):
    """`rounds` rounds from `state` (None: fresh). restart: the first round takes every count of the context's rows as 0
    (camera.frame_index == 0). Returns the State."""
    p = resolve(params)
    W, H = int(cam["width"]), int(cam["height"])
    st = State(H, W) if state is None else state
    inside = rows_mask(H, rows)
    if restart:
        st.moments[inside, :, 2] = 0
        st.rounds = 0
    for _ in range(rounds):
        act = select(st.moments, p, inside)
        st.active.append(int(act.sum()))
        for y, x in zip(*np.nonzero(act)):
            n = int(st.moments[y, x, 2])
            rgb, mom = st.image[y, x, :3], st.moments[y, x]
            for f in range(n, n + p["step"]):
                L, log = oracle.trace_path(scene, cam, int(x), int(y), f, max_bounces=max_bounces, do_mis=do_mis)
                rgb, mom = fold_pixel(rgb, mom, L, f)
                st.segments += int((log[:, 15] == 1).sum())          # the last record (alive = 0) is no segment
            st.image[y, x] = (rgb[0], rgb[1], rgb[2], 0)
            st.moments[y, x] = mom
        st.paths += st.active[-1] * p["step"]
        st.rounds += 1
    return st


def fold_listed(rgb, mom, L, frame):
    """fold_pixel for n pixels at once: rgb (n, 3), mom (n, 4), per-path radiance L (n, 3), each pixel at its own frame (n,)"""
    frame = np.asarray(frame, np.uint32)
    c = np.fmin(np.asarray(L, np.float32), f32(2.5))
    l = f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1] + f32(0.0722) * c[:, 2]
    m = np.stack([l, l * l], axis=1).astype(np.float32)
    t = (f32(1) / (frame + np.uint32(1)).astype(np.float32))[:, None]
    later = (frame > 0)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(later, _mix(rgb, c, t), c).astype(np.float32)
        m = np.where(later, _mix(mom[:, :2], m, t), m).astype(np.float32)
    out = np.zeros((len(frame), 4), np.float32)
    out[:, :2], out[:, 2] = m, (frame + np.uint32(1)).astype(np.float32)
    return c, out


def run_planes(oracle, scene, cam, params, rounds, rows=None, state=None, restart=True, max_bounces=8, do_mis=1):
    """run(), with the listed pixels of a round traced and folded together (same arguments, same State, bit for bit)"""
    p = resolve(params)
    W, H = int(cam["width"]), int(cam["height"])
    st = State(H, W) if state is None else state
    inside = rows_mask(H, rows)
    if restart:
        st.moments[inside, :, 2] = 0
        st.rounds = 0
    for _ in range(rounds):
        act = select(st.moments, p, inside)
        st.active.append(int(act.sum()))
        ys, xs = np.nonzero(act)
        rgb, mom = st.image[ys, xs, :3], st.moments[ys, xs]
        n0 = mom[:, 2].astype(np.uint32)
        for k in range(p["step"] if len(ys) else 0):
            L, seg = oracle.trace_paths(scene, cam, xs, ys, n0 + np.uint32(k), max_bounces=max_bounces, do_mis=do_mis)
            rgb, mom = fold_listed(rgb, mom, L, n0 + np.uint32(k))
            st.segments += int(seg.sum(dtype=np.uint64))
        st.image[ys, xs, :3], st.image[ys, xs, 3] = rgb, 0
        st.moments[ys, xs] = mom
        st.paths += st.active[-1] * p["step"]
        st.rounds += 1
    return st


def status(st, rows=None):
    """what ptmi_adaptive_status reports for the model's state"""
    c = st.counts[rows_mask(st.image.shape[0], rows)]
    return dict(active=st.active[-1] if st.active else 0, samples=int(c.astype(np.uint64).sum()), min_count=int(c.min()),
                max_count=int(c.max()), rounds=st.rounds)


def planes_at_counts(counts, planes_by_n):
    """per pixel the value of planes_by_n[counts[pixel]]: what a plane folded per pixel in frame order holds when every pixel has its
    own count (planes_by_n: {n: (H, W, C) plane after n uniform frames})"""
    any_plane = next(iter(planes_by_n.values()))
    out = np.zeros_like(any_plane)
    for n in np.unique(counts):
        if n == 0:
            continue
        out[counts == n] = planes_by_n[int(n)][counts == n]
    return out
