"""A numpy model of the participating medium (include/ptmi.h ptmi_set_medium): the interval a ray spends inside the
box, free flight, transmittance, the Henyey-Greenstein phase value and its sampling with the frame of Duff et al. 2017. Every function
takes a dtype: float64 is the reference; float32 runs the same formulas in the kernels' precision (with numpy's own rounding of each
step, no fused multiply-adds), which is what the tests measure a tolerance from."""
import functools

import numpy as np


class Medium:
    def __init__(self, sigma_t, albedo, g, box_min, box_max):
        self.sigma_t, self.g = float(np.float32(sigma_t)), float(np.float32(g))
        self.albedo = np.broadcast_to(np.asarray(albedo, np.float32), (3,)).astype(np.float64)
        self.box_min, self.box_max = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)

    def kwargs(self):
        """what native.Context.set_medium takes"""
        return dict(sigma_t=self.sigma_t, albedo=tuple(self.albedo), g=self.g, box=(tuple(self.box_min), tuple(self.box_max)))


def interval(m, o, d, t_hit, dtype=np.float64):
    """(near, far, a, b) per ray; fmin / fmax drop the NaN of 0 * inf. No interval: NOT b > a; a ray that is NaN on every axis has none."""
    o, d, t_hit = np.asarray(o, np.float32).astype(dtype), np.asarray(d, np.float32).astype(dtype), np.asarray(t_hit, np.float32).astype(dtype)
    lo, hi = m.box_min.astype(dtype), m.box_max.astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = dtype(1.0) / d
        t1, t2 = (lo - o) * inv, (hi - o) * inv
    near = np.fmax(np.fmax(np.fmin(t1, t2)[:, 0], np.fmin(t1, t2)[:, 1]), np.fmin(t1, t2)[:, 2])
    far = np.fmin(np.fmin(np.fmax(t1, t2)[:, 0], np.fmax(t1, t2)[:, 1]), np.fmax(t1, t2)[:, 2])
    a = np.fmax(near, dtype(0.0))
    return near, far, a, np.where(np.isnan(far), a, np.fmin(far, t_hit))


def free_flight(m, r, dtype=np.float64):
    r = np.asarray(r, np.float32).astype(dtype)
    with np.errstate(divide="ignore"):
        return -np.log(dtype(1.0) - r) / dtype(m.sigma_t)


def transmittance(m, o, wi, dist, dtype=np.float64):
    dist = np.asarray(dist, np.float32).astype(dtype)
    near, far, a, _ = interval(m, o, wi, np.full(len(dist), np.inf, np.float32), dtype)
    end = np.where(dist < 0, far, np.fmin(far, dist))
    with np.errstate(invalid="ignore"):
        return np.exp(-dtype(m.sigma_t) * np.fmax(dtype(0.0), end - a))


def phase(g, cos_t, dtype=np.float64):
    g, cos_t = dtype(np.float32(g)), np.asarray(cos_t).astype(dtype)
    k = dtype(1.0) + g * g - dtype(2.0) * g * cos_t
    return (dtype(1.0) - g * g) / (dtype(4.0 * np.pi) * (k * np.sqrt(k)))


def sample_cos(g, xi1, dtype=np.float64):
    g, xi1 = dtype(np.float32(g)), np.asarray(xi1, np.float32).astype(dtype)
    if abs(g) < 1e-3:
        ct = dtype(1.0) - dtype(2.0) * xi1
    else:
        q = (dtype(1.0) - g * g) / (dtype(1.0) - g + dtype(2.0) * g * xi1)
        ct = (dtype(1.0) + g * g - q * q) / (dtype(2.0) * g)
    return np.clip(ct, dtype(-1.0), dtype(1.0))


def sample_direction(g, d, xi1, xi2, dtype=np.float64):
    """(direction (n, 3), sampled cos theta (n,)) about the unit directions d"""
    d = np.asarray(d, np.float32).astype(dtype)
    xi2 = np.asarray(xi2, np.float32).astype(dtype)
    ct = sample_cos(g, xi1, dtype)
    st = np.sqrt(np.fmax(dtype(0.0), dtype(1.0) - ct * ct))
    phi = dtype(2.0 * np.pi) * xi2
    sp, cp = np.sin(phi), np.cos(phi)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    sg = np.copysign(dtype(1.0), z)
    A = dtype(-1.0) / (sg + z)
    B = x * y * A
    T = np.stack([dtype(1.0) + sg * x * x * A, sg * B, -sg * x], axis=1)
    U = np.stack([B, sg + y * y * A, -y], axis=1)
    v = (st * cp)[:, None] * T + (st * sp)[:, None] * U + ct[:, None] * d
    return v / np.sqrt((v * v).sum(axis=1))[:, None], ct


def step(m, o, d, t_hit, r, dtype=np.float64):
    """One path segment on the uniforms r (n, 3) = (r, xi1, xi2), as ptmi_debug_medium_step reports it:
    dict(scattered, x, dir, a, b, s, pdf, margin); without an interval s, x, dir and pdf are 0, without a scatter x, dir and pdf are.
    margin = |a + s - b|: how far the scatter decision is from flipping."""
    r = np.asarray(r, np.float32)
    _, _, a, b = interval(m, o, d, t_hit, dtype)
    with np.errstate(invalid="ignore"):
        has = b > a
        s = np.where(has, free_flight(m, r[:, 0], dtype), dtype(0.0))
        t_sc = a + s
        sc = has & (t_sc < b)
        margin = np.where(has, np.abs(t_sc - b), np.inf)
        x = np.asarray(o, np.float32).astype(dtype) + np.where(sc, t_sc, dtype(0.0))[:, None] * np.asarray(d, np.float32).astype(dtype)
    direc, ct = sample_direction(m.g, d, r[:, 1], r[:, 2], dtype)
    pdf = phase(m.g, ct, dtype)
    z3 = np.zeros_like(x)
    return dict(scattered=sc, x=np.where(sc[:, None], x, z3), dir=np.where(sc[:, None], direc, z3), a=a, b=b, s=s,
                pdf=np.where(sc, pdf, dtype(0.0)), margin=margin)


# ---- the inputs of the probes' test (tests/test_gpu_medium.py) and how a result is held against the float64 model ----------------------
BOXES = [((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((-0.75, 0.1, -3.5), (2.25, 1.3, 0.4))]
N_PROBE = 4096
PROBE_SEED = 5
# The largest deviation between medium_ref evaluated in float32 and in float64 on these very inputs, over both boxes and the three g
# (tests/test_medium_host.py measures it again without a GPU and holds the constants to it):
#   a, b, s, x, Tr as |difference| / max(|value|, 1):  7.86e-7 (x: the rounding of o + t d at |x| of a few units)
#   the direction, per component (a unit vector):        3.50e-5 (g = -0.8: sin theta = sqrt(1 - cos^2) next to the backward peak,
#                                                        where an ulp of cos theta is 3e-4 of sin theta; 3.9e-7 for g = 0)
#   the phase density as |difference| / value:           2.28e-6 (g = -0.8; 4e-8 for g = 0)
# each times 4, which leaves room for the device's logf / expf being 1 - 2 ulp and for its fused multiply-adds.
MEASURED_GEOM, MEASURED_DIR, MEASURED_PDF = 7.86e-7, 3.50e-5, 2.28e-6
TOL_GEOM, TOL_DIR, TOL_PDF = 4.0 * MEASURED_GEOM, 4.0 * MEASURED_DIR, 4.0 * MEASURED_PDF
# A whole render in fog against the CPU oracle's (tests/test_gpu_shade_extras.py): the largest deviation of a pixel, |difference| /
# max(|value|, 1) per channel, between the oracle's renders of the fog / sky gauntlet (tests/gauntlet_scenes.py: the two states with fog, every
# bounce limit of fog_gpu_cases, FOG_FRAMES frames) with every result of logf / expf / atan2f / acosf moved by -2 .. 2 float32 steps and
# the render with none moved, over the pixels none of whose paths took another branch for it (the oracle's hash of a path's decisions
# tells; those pixels, some 20 of 3 072 a render, deviate by anything from 1e-9 to 0.08). tests/test_oracle_extras_host.py measures it
# again without a GPU and holds the constant to it. Times 4.
MEASURED_SHADE = 7.52e-6
TOL_SHADE = 4.0 * MEASURED_SHADE


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def probe_inputs(box_index):
    """4 096 rays around BOXES[box_index] and their uniforms: origins inside, outside and on a face, axis-parallel directions, rays that
    miss the box, hit distances inside the box, r = 0"""
    lo, hi = (np.asarray(b, np.float64) for b in BOXES[box_index])
    mid, ext = (lo + hi) / 2, (hi - lo)
    rng = np.random.default_rng(PROBE_SEED + box_index)
    n = N_PROBE
    o = mid + (rng.random((n, 3)) - 0.5) * ext * np.where(np.arange(n)[:, None] % 2, 0.98, 4.0)      # odd: inside; even: around, mostly outside
    target = mid + (rng.random((n, 3)) - 0.5) * ext * 0.9
    d = unit(np.where((np.arange(n)[:, None] % 4) == 0, rng.normal(size=(n, 3)), target - o))       # a quarter anywhere (many miss), the rest at the box
    o = o.astype(np.float32)
    k = np.arange(n)
    face = (k % 16) == 5                                                    # on a face: one coordinate is the box's, exactly
    ax = (k // 16) % 3
    o[face, ax[face]] = np.where(((k // 48) % 2)[:, None], np.float32(hi), np.float32(lo))[face, ax[face]]
    par = (k % 16) == 9                                                     # axis-parallel: two direction components exactly 0
    d[par] = 0.0
    d[par, ax[par]] = np.where((k // 48) % 2, 1.0, -1.0)[par]
    t_hit = np.where(k % 3 == 0, np.float32(np.inf), (rng.random(n) * 1.5 * np.linalg.norm(ext)).astype(np.float32)).astype(np.float32)
    r = rng.random((n, 3), np.float32)
    r[(k % 32) == 7, 0] = 0.0
    r[(k % 64) == 11, 0] = np.float32(1.0)                                  # the RNG's float can be 1: no collision
    return o, d, t_hit, r


def deviation(got, ref, relative_to_value=False):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])                             # an infinite end is the same infinity
    if not fin.any():
        return 0.0
    scale = np.abs(ref[fin]) if relative_to_value else np.maximum(np.abs(ref[fin]), 1.0)
    return float((np.abs(got[fin] - ref[fin]) / scale).max())


def set_aside(m64):
    return m64["margin"] < 1e-4 * np.maximum(m64["b"], 1.0)


def step_deviations(got, m64):
    """(geometry, direction, density) deviations of one step result (a dict like medium_ref.step's) from the float64 model's, and the share of
    scatter decisions set aside; asserts the decisions that are not"""
    aside = set_aside(m64)
    assert np.array_equal(got["scattered"][~aside], m64["scattered"][~aside])
    both = got["scattered"] & m64["scattered"]
    has = m64["b"] > m64["a"]
    geom = max(deviation(got["a"], m64["a"]), deviation(got["b"], m64["b"]), deviation(got["s"][has & ~aside], m64["s"][has & ~aside]),
               deviation(got["x"][both], m64["x"][both]))
    return geom, deviation(got["dir"][both], m64["dir"][both]), deviation(got["pdf"][both], m64["pdf"][both], True), float(aside.mean())


def tr_inputs(box_index):
    o, d, t_hit, _ = probe_inputs(box_index)
    dist = np.where(np.arange(len(o)) % 3 == 0, np.float32(-1.0), t_hit).astype(np.float32)
    return o, d, dist
