"""A numpy model of the medium's density grid (include/ptmi.h ptmi_upload_medium_density): the lookup, delta tracking,
ratio tracking and the kernel RNG they draw from. Every function takes a dtype: float64 is the reference; float32 runs the same formulas
in the kernels' precision, with numpy's own rounding of each step and the kernels' one fused step (the point o + t d), which is what the
tests measure a tolerance from. The draws themselves are the RNG's float32 values in both."""
import functools

import numpy as np

import medium_ref

TRACK_CAP = 65536           # PT_MED_TRACK_CAP: the guard of both loops; nothing here may come near it
MAX_DEPTH = 256.0           # PT_MED_MAX_DEPTH: sigma_t * |box diagonal| up to which a grid is accepted


# ---- the kernel RNG (csrc/pt_math.h rng_word / rng_f) ---------------------------------------------------------------------------------
def rng_next(state):
    """(the state afterwards, the draw as float32) of uint32 states"""
    s = (state.astype(np.uint64) * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    w = (r >> np.uint64(22)) ^ r
    return s.astype(np.uint32), w.astype(np.float32) * np.float32(2.0 ** -32)       # f32(word) rounds to nearest; can be 1.0


# ---- the lookup -------------------------------------------------------------------------------------------------------------------------
def _cell(f, n):
    """clamp(int(f), 0, n - 1) of floored coordinates; NaN reads 0"""
    return np.clip(np.where(np.isnan(f), 0.0, f), 0, n - 1).astype(np.int64)


def lookup(m, grid, filt, p, dtype=np.float64):
    """rho at the points p (n, 3), already of dtype. grid: (nz, ny, nx) float32."""
    grid = np.asarray(grid, np.float32)
    nz, ny, nx = grid.shape
    g = grid.astype(dtype)
    lo, hi = m.box_min.astype(dtype), m.box_max.astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (p - lo) / (hi - lo) * np.array([nx, ny, nz], dtype)
        if filt == 0:
            c = np.floor(u)
            return g[_cell(c[:, 2], nz), _cell(c[:, 1], ny), _cell(c[:, 0], nx)]
        v = u - dtype(0.5)
        b = np.floor(v)
        f = v - b
        i0, i1 = _cell(b[:, 0], nx), _cell(b[:, 0] + 1, nx)
        j0, j1 = _cell(b[:, 1], ny), _cell(b[:, 1] + 1, ny)
        k0, k1 = _cell(b[:, 2], nz), _cell(b[:, 2] + 1, nz)
        one = dtype(1.0)
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        mix = lambda a, bb, t: a * (one - t) + bb * t
        c00, c10 = mix(g[k0, j0, i0], g[k0, j0, i1], fx), mix(g[k0, j1, i0], g[k0, j1, i1], fx)
        c01, c11 = mix(g[k1, j0, i0], g[k1, j0, i1], fx), mix(g[k1, j1, i0], g[k1, j1, i1], fx)
        return mix(mix(c00, c10, fy), mix(c01, c11, fy), fz)


def point(o, d, t, dtype):
    """o + t d: the kernels' one fused multiply-add per component (float32: the exact product and sum, rounded once)"""
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == np.float32:
            return (d.astype(np.float64) * t.astype(np.float64)[:, None] + o.astype(np.float64)).astype(np.float32)
        return d * t[:, None] + o


def _flight(m, r, dtype):
    with np.errstate(divide="ignore"):
        return -np.log(dtype(1.0) - r.astype(dtype)) / dtype(m.sigma_t)


# ---- the trackers -----------------------------------------------------------------------------------------------------------------------
def delta_track(m, grid, filt, o, d, t_end, rng, dtype=np.float64):
    """ptmi_debug_medium_track mode 0: dict(scattered, t, value, steps, rng); without an interval nothing is drawn"""
    o32, d32 = np.asarray(o, np.float32), np.asarray(d, np.float32)
    o_, d_ = o32.astype(dtype), d32.astype(dtype)
    _, _, a, b = medium_ref.interval(m, o32, d32, t_end, dtype)
    n = len(o_)
    state = np.asarray(rng, np.uint32).copy()
    with np.errstate(invalid="ignore"):
        live = b > a
    t = a.copy()
    steps, scattered = np.zeros(n, np.uint32), np.zeros(n, bool)
    value = np.zeros(n, dtype)
    for _ in range(TRACK_CAP):
        if not live.any():
            break
        k = np.flatnonzero(live)
        state[k], r = rng_next(state[k])
        t[k] = t[k] + _flight(m, r, dtype)
        with np.errstate(invalid="ignore"):
            on = t[k] < b[k]
        live[k[~on]] = False
        k = k[on]
        steps[k] += 1
        rho = lookup(m, grid, filt, point(o_[k], d_[k], t[k], dtype), dtype)
        state[k], r2 = rng_next(state[k])
        with np.errstate(invalid="ignore"):
            hit = r2.astype(dtype) < rho
        scattered[k[hit]] = True
        value[k[hit]] = rho[hit]
        live[k[hit]] = False
    assert not live.any(), "the tracking cap was reached"
    return dict(scattered=scattered, t=np.where(scattered, t, dtype(0.0)), value=value, steps=steps, rng=state)


def ratio_track(m, grid, filt, o, wi, dist, rng, dtype=np.float64):
    """ptmi_debug_medium_track mode 1: dict(scattered (never), t = the segment's end, value = T, steps, rng)"""
    o32, w32 = np.asarray(o, np.float32), np.asarray(wi, np.float32)
    o_, w_ = o32.astype(dtype), w32.astype(dtype)
    dist = np.asarray(dist, np.float32).astype(dtype)
    near, far, a, _ = medium_ref.interval(m, o32, w32, np.full(len(o_), np.inf, np.float32), dtype)
    end = np.where(dist < 0, far, np.fmin(far, dist))
    n = len(o_)
    state = np.asarray(rng, np.uint32).copy()
    t = a.copy()
    T = np.ones(n, dtype)
    steps, live = np.zeros(n, np.uint32), np.ones(n, bool)
    for _ in range(TRACK_CAP):
        if not live.any():
            break
        k = np.flatnonzero(live)
        state[k], r = rng_next(state[k])
        t[k] = t[k] + _flight(m, r, dtype)
        with np.errstate(invalid="ignore"):
            on = t[k] < end[k]
        live[k[~on]] = False
        k = k[on]
        steps[k] += 1
        T[k] = T[k] * (dtype(1.0) - lookup(m, grid, filt, point(o_[k], w_[k], t[k], dtype), dtype))
        live[k[T[k] == 0]] = False
    assert not live.any(), "the tracking cap was reached"
    return dict(scattered=np.zeros(n, bool), t=end, value=T, steps=steps, rng=state)


def track(mode, *a, **kw):
    return (ratio_track if mode else delta_track)(*a, **kw)


# ---- the inputs of the probes' test (tests/test_gpu_medium_grid.py) and how a result is held against the models ---------------------------
GRID_DIMS = [(1, 1, 1), (2, 1, 1), (3, 5, 2), (16, 16, 16)]            # (nx, ny, nz); 3 x 5 x 2 tells an index order or an axis mix-up
BOX_INDEX = 1                                                           # medium_ref.BOXES[1]: off centre, three different extents
GRID_SEED, STATE_SEED = 41, 43                                          # the committed seeds (tests/test_medium_grid_host.py holds them)
ASIDE_CAP = 0.02


def probe_medium():
    """sigma_t 3 over a box of diagonal 5: some 15 tentative collisions across it"""
    return medium_ref.Medium(3.0, 0.8, 0.3, *medium_ref.BOXES[BOX_INDEX])


@functools.lru_cache(maxsize=None)
def probe_grid(dims):
    """(nz, ny, nx) float32 in [0, 1] with exact zeros and ones among the cells (a single cell: 0.6)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(GRID_SEED + nx * 10000 + ny * 100 + nz)
    g = rng.random((nz, ny, nx), np.float32)
    flat = g.reshape(-1)
    if flat.size == 1:
        flat[0] = 0.6
    else:
        flat[::7] = 0.0
        flat[3::11] = 1.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def probe_rays(mode):
    """(o, d, t_end, rng states): the rays of medium_ref's probes with a kernel RNG state each"""
    if mode == 0:
        o, d, t_end, _ = medium_ref.probe_inputs(BOX_INDEX)
    else:
        o, d, t_end = medium_ref.tr_inputs(BOX_INDEX)
    state = np.random.default_rng(STATE_SEED + mode).integers(0, 2 ** 32, len(o), dtype=np.uint64).astype(np.uint32)
    return o, d, t_end, state


@functools.lru_cache(maxsize=None)
def lookup_points():
    """4 096 points in and around the box, some on its faces and on cell faces of the 16-cell grid, some far outside, one NaN each axis"""
    lo, hi = (np.asarray(b, np.float64) for b in medium_ref.BOXES[BOX_INDEX])
    rng = np.random.default_rng(GRID_SEED)
    n = medium_ref.N_PROBE
    p = (lo + (rng.random((n, 3)) * 1.2 - 0.1) * (hi - lo)).astype(np.float32)
    k = np.arange(n)
    ax = (k // 16) % 3
    face = (k % 16) == 3
    p[face, ax[face]] = np.where(((k // 48) % 2)[:, None], np.float32(hi), np.float32(lo))[face, ax[face]]
    cell = (k % 16) == 7                                                     # multiples of 1 / 16 of the extent
    p[cell, ax[cell]] = (lo + (hi - lo) * ((k // 48) % 17)[:, None] / 16.0).astype(np.float32)[cell, ax[cell]]
    far = (k % 64) == 21
    p[far] *= np.float32(1e6)
    for a in range(3):
        p[100 + a, a] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def models(dims, filt, mode):
    """(float64 model, float32 model, set-aside) on the probe rays: the rays on which the two precisions take different decisions — another
    number of tentative collisions, or another scatter / no-scatter outcome"""
    m, g = probe_medium(), probe_grid(dims)
    o, d, t_end, state = probe_rays(mode)
    m64 = track(mode, m, g, filt, o, d, t_end, state, dtype=np.float64)
    m32 = track(mode, m, g, filt, o, d, t_end, state, dtype=np.float32)
    aside = (m64["steps"] != m32["steps"]) | (m64["scattered"] != m32["scattered"])
    return m64, m32, aside


HALF_ULP = 2.0 ** -24


def deviation(got, ref):
    """the largest |difference| / max(|value|, 1); values that are not finite must be the same"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)).max())


def tolerance(measured):
    """four times the float32 model's deviation, which leaves room for the device's logf being 1 - 2 ulp; never below four half ulps of
    a float32, the rounding of the result itself"""
    return 4.0 * max(measured, HALF_ULP)
