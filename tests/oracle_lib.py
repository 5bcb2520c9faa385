"""ctypes binding of the CPU oracle (oracle/pt_oracle.h) — test infrastructure.

Used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only.
"""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")


class PtoScene(ctypes.Structure):
    _fields_ = [("tris", ctypes.c_void_p), ("n_tris", ctypes.c_uint32),
                ("mats", ctypes.c_void_p), ("n_mats", ctypes.c_uint32),
                ("nodes", ctypes.c_void_p), ("n_nodes", ctypes.c_uint32),
                ("lights", ctypes.c_void_p), ("n_lights", ctypes.c_uint32),
                ("atlas", ctypes.c_void_p), ("atlas_w", ctypes.c_uint32), ("atlas_h", ctypes.c_uint32),
                ("atlas_fmt", ctypes.c_int32)]


class PtoOptions(ctypes.Structure):
    _fields_ = [("max_bounces", ctypes.c_uint32), ("do_mis", ctypes.c_uint32),
                ("y0", ctypes.c_uint32), ("y1", ctypes.c_uint32), ("threads", ctypes.c_uint32)]


class PtoStats(ctypes.Structure):
    _fields_ = [("paths", ctypes.c_uint64), ("segments", ctypes.c_uint64), ("shadow_rays", ctypes.c_uint64),
                ("nodes_visited", ctypes.c_uint64), ("tris_tested", ctypes.c_uint64),
                ("closest_hits", ctypes.c_uint64), ("max_stack", ctypes.c_uint32), ("threads", ctypes.c_uint32),
                ("seconds", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PtoExtras(ctypes.Structure):
    _fields_ = [("env_texels", ctypes.c_void_p), ("env_prob", ctypes.c_void_p), ("env_alias", ctypes.c_void_p),
                ("env_w", ctypes.c_uint32), ("env_h", ctypes.c_uint32), ("env_sampled", ctypes.c_uint32),
                ("env_intensity", ctypes.c_float), ("env_rotation", ctypes.c_float),
                ("med_on", ctypes.c_uint32), ("sigma_t", ctypes.c_float), ("albedo", ctypes.c_float * 3), ("g", ctypes.c_float),
                ("box_min", ctypes.c_float * 3), ("box_max", ctypes.c_float * 3), ("ulp_nudge", ctypes.c_int32)]


PROBE_MED_STEP, PROBE_MED_TR, PROBE_MED_PHASE, PROBE_ENV_SAMPLE, PROBE_ENV_LOOKUP = range(5)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Oracle:
    def __init__(self, strict=False, literal=False):
        """strict: pt_oracle.c built with literal arithmetic; literal: oracle/pt_literal.c, the independent transcription in the
        reference's own shape (it offers the subset of entry points the literal comparisons use)"""
        name = "libpt_literal.so" if literal else "libpt_oracle_strict.so" if strict else "libpt_oracle.so"
        path = os.path.join(os.environ.get("PT_ORACLE_BUILD_DIR") or os.path.join(ORACLE_DIR, "build"), name)   # (a sanitizer build, tools/sanitize/run_oracle.sh)
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", ORACLE_DIR], stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(path)
        L.pto_seed.restype = ctypes.c_uint32
        L.pto_seed.argtypes = [ctypes.c_uint32] * 3
        L.pto_rand_int.restype = ctypes.c_uint32
        L.pto_rand_int.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
        L.pto_sincos.argtypes = [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
        L.pto_distribution_ggx.restype = ctypes.c_float
        L.pto_distribution_ggx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
        L.pto_power_heuristic.restype = ctypes.c_float
        L.pto_power_heuristic.argtypes = [ctypes.c_float] * 4
        L.pto_eval_bsdf.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self.L = L
        self.strict = bool(L.pto_is_strict())
        self.literal = L.pto_is_strict() == 2
        assert self.literal == literal and self.strict == (strict or literal)

    # -- scene marshalling ---------------------------------------------------
    @staticmethod
    def scene_struct(scene):
        s = PtoScene()
        s.tris, s.n_tris = _ptr(scene.tris), len(scene.tris)
        s.mats, s.n_mats = _ptr(scene.mats), len(scene.mats)
        s.nodes, s.n_nodes = _ptr(scene.nodes), len(scene.nodes)
        s.lights, s.n_lights = _ptr(scene.lights), len(scene.lights)
        if scene.atlas is not None:
            a = scene.atlas
            assert a.dtype in (np.float16, np.float32) and a.ndim == 3 and a.shape[2] == 4 and a.flags.c_contiguous
            s.atlas, s.atlas_h, s.atlas_w = _ptr(a), a.shape[0], a.shape[1]
            s.atlas_fmt = 1 if a.dtype == np.float16 else 2
        return s

    # -- RNG -----------------------------------------------------------------
    def seed(self, x, y, frame):
        return self.L.pto_seed(x, y, frame)

    def rand(self, state, n):
        st = ctypes.c_uint32(state)
        states, words, vals = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.L.pto_rand(ctypes.byref(st), n, _ptr(states), _ptr(words), _ptr(vals))
        return states, words, vals

    def rand_int(self, state, lo, hi):
        st = ctypes.c_uint32(state)
        k = self.L.pto_rand_int(ctypes.byref(st), lo, hi)
        return k, st.value

    def sincos(self, x):
        s, c = ctypes.c_float(), ctypes.c_float()
        self.L.pto_sincos(float(x), ctypes.byref(s), ctypes.byref(c))
        return s.value, c.value

    # -- stages --------------------------------------------------------------
    def raygen(self, cam, xs, ys, frames):
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, frames))
        n = len(xs)
        o, d, rng = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        self.L.pto_raygen(_ptr(cam), n, _ptr(xs), _ptr(ys), _ptr(frames), _ptr(o), _ptr(d), _ptr(rng))
        return o, d, rng

    def intersect(self, scene, o, d):
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = len(o)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        tri = np.zeros(n, np.uint32)
        st = PtoStats()
        s = self.scene_struct(scene)
        self.L.pto_intersect(ctypes.byref(s), n, _ptr(o), _ptr(d), _ptr(t), _ptr(tri), _ptr(u), _ptr(v), ctypes.byref(st))
        return t, tri, u, v, st

    def occluded(self, scene, o, d, dist):
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        dist = np.ascontiguousarray(dist, np.float32)
        occ = np.zeros(len(o), np.uint8)
        s = self.scene_struct(scene)
        self.L.pto_occluded(ctypes.byref(s), len(o), _ptr(o), _ptr(d), _ptr(dist), _ptr(occ), None)
        return occ

    def render(self, scene, cam, n_frames, max_bounces=8, do_mis=1, out=None, y0=0, y1=0, threads=0):
        W, H = int(cam["width"]), int(cam["height"])
        if out is None:
            out = np.zeros((H, W, 4), np.float32)
        assert out.dtype == np.float32 and out.shape == (H, W, 4) and out.flags.c_contiguous
        opt = PtoOptions(max_bounces, do_mis, y0, y1, threads)
        st = PtoStats()
        s = self.scene_struct(scene)
        rc = self.L.pto_render(ctypes.byref(s), _ptr(cam), n_frames, ctypes.byref(opt), _ptr(out), ctypes.byref(st))
        assert rc == 0
        return out, st

    def render_tap(self, scene, cam, frames, y0=0, y1=0, max_rays=1 << 22, max_bounces=8, do_mis=1, threads=0):
        """Every ray the render of rows [y0, y1) (y1 = 0: to the last row) x `frames` frames traces, with the reference traversal's
        result (pto_render_tap): (n, 9) float32 = o, d, dist (0: a closest-hit ray; < 0: a shadow ray to a directional light; > 0: a
        shadow ray, the light's distance), t (-1: a miss), the triangle's bits. With threads = 1 the records stand in the order they
        were traced: pixel by pixel, frame by frame, a path's rays one after the other, a shadow ray right behind the ray whose
        hit it starts from; otherwise in no particular order."""
        fn = self.L.pto_render_tap
        fn.restype = ctypes.c_uint64
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        rec = np.zeros((max_rays, 9), np.float32)
        opt = PtoOptions(max_bounces, do_mis, y0, y1, threads)
        s = self.scene_struct(scene)
        n = fn(ctypes.byref(s), _ptr(cam), frames, ctypes.byref(opt), _ptr(rec), max_rays)
        assert n <= max_rays, "the render traced %d rays, more than the %d there was room for" % (n, max_rays)
        return rec[:n]

    def census_events(self):
        """the names of the census events, in table order (oracle/pt_oracle.h PTO_CENSUS_EVENTS)"""
        self.L.pto_census_event_name.restype = ctypes.c_char_p
        self.L.pto_census_event_name.argtypes = [ctypes.c_int]
        return [self.L.pto_census_event_name(i).decode() for i in range(self.L.pto_census_event_count())]

    def render_census(self, scene, cam, n_frames, max_bounces=8, do_mis=1, out=None, y0=0, y1=0, threads=0):
        """render() plus the branch census: (out, stats, {event name: (64,) uint64 occurrences per bounce})"""
        W, H = int(cam["width"]), int(cam["height"])
        if out is None:
            out = np.zeros((H, W, 4), np.float32)
        assert out.dtype == np.float32 and out.shape == (H, W, 4) and out.flags.c_contiguous
        names = self.census_events()
        table = np.zeros((len(names), 64), np.uint64)
        opt = PtoOptions(max_bounces, do_mis, y0, y1, threads)
        st = PtoStats()
        s = self.scene_struct(scene)
        fn = self.L.pto_render_census
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        rc = fn(ctypes.byref(s), _ptr(cam), n_frames, ctypes.byref(opt), _ptr(out), ctypes.byref(st), _ptr(table))
        assert rc == 0
        return out, st, dict(zip(names, table))

    def blit(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        H, W = rgba.shape[:2]
        out = np.zeros_like(rgba)
        self.L.pto_blit(_ptr(rgba), W, H, _ptr(out))
        return out

    def trace_path(self, scene, cam, x, y, frame, max_bounces=8, do_mis=1):
        opt = PtoOptions(max_bounces, do_mis, 0, 0, 1)
        rad = np.zeros(3, np.float32)
        log = np.zeros((max_bounces + 1, 16), np.float32)
        s = self.scene_struct(scene)
        n = self.L.pto_trace_path(ctypes.byref(s), _ptr(cam), x, y, frame, ctypes.byref(opt), _ptr(rad), _ptr(log))
        return rad, log[:n]

    def trace_paths(self, scene, cam, xs, ys, frames, max_bounces=8, do_mis=1, threads=0):
        """trace_path for arrays of (x, y, frame): per-path radiance (n, 3) float32 (unclamped) and segment count (n,) uint32 (the
        records of trace_path's log with alive = 1), threaded like render"""
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32).ravel() for a in (xs, ys, frames))
        n = len(xs)
        assert len(ys) == n and len(frames) == n
        rad, seg = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        opt = PtoOptions(max_bounces, do_mis, 0, 0, threads)
        s = self.scene_struct(scene)
        fn = self.L.pto_trace_paths
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 6
        rc = fn(ctypes.byref(s), _ptr(cam), n, _ptr(xs), _ptr(ys), _ptr(frames), ctypes.byref(opt), _ptr(rad), _ptr(seg))
        assert rc == 0
        return rad, seg

    # -- extras: the environment and the medium (oracle/pt_oracle.h pto_extras) ---------------------------------------------
    @staticmethod
    def extras(env=None, medium=None, ulp_nudge=0):
        """pto_extras, and the arrays it points into (keep both alive for the call).
        env: dict(texels (H, W, 4) float32 with alpha, c (H, W), prob, alias — the last three from native.env_table —, intensity,
        rotation, sampled) or None; medium: dict(sigma_t, albedo, g, box=(min, max)) (what native.Context.set_medium takes) or None."""
        ex, keep = PtoExtras(), []
        if env is not None:
            t = np.ascontiguousarray(env["texels"], np.float32).copy()
            t[..., 3] = np.asarray(env["c"], np.float32)
            prob, alias = np.ascontiguousarray(env["prob"], np.float32), np.ascontiguousarray(env["alias"], np.uint32)
            assert t.ndim == 3 and t.shape[2] == 4 and len(prob) == len(alias) == t.shape[0] * t.shape[1]
            rot, inten = float(env.get("rotation", 0.0)), float(env.get("intensity", 1.0))
            assert abs(rot) <= np.pi and inten > 0.0          # as ptmi_upload_environment resolves them
            keep += [t, prob, alias]
            ex.env_texels, ex.env_prob, ex.env_alias = _ptr(t), _ptr(prob), _ptr(alias)
            ex.env_h, ex.env_w, ex.env_sampled = t.shape[0], t.shape[1], int(env.get("sampled", 1))
            ex.env_intensity, ex.env_rotation = inten, rot
        if medium is not None:
            f3 = ctypes.c_float * 3
            ex.med_on, ex.sigma_t, ex.g = 1, medium["sigma_t"], medium.get("g", 0.0)
            ex.albedo = f3(*np.broadcast_to(np.asarray(medium.get("albedo", 1.0), np.float32), (3,)))
            ex.box_min, ex.box_max = f3(*medium["box"][0]), f3(*medium["box"][1])
        ex.ulp_nudge = int(ulp_nudge)
        return ex, keep

    def render_ext(self, scene, cam, n_frames, extras=None, max_bounces=8, do_mis=1, out=None, y0=0, y1=0, threads=0, census=False):
        """render() / render_census() with extras (from Oracle.extras; None: none): (out, stats, border[, census]); border (H, W)
        float32 = per pixel the smallest distance of a sky lookup from a texel border, in texels (inf: no lookup). The per-pixel
        hash of the decisions its paths took (pto_render_ext's branches) is left in self.last_branches, (H, W) uint32."""
        W, H = int(cam["width"]), int(cam["height"])
        if out is None:
            out = np.zeros((H, W, 4), np.float32)
        assert out.dtype == np.float32 and out.shape == (H, W, 4) and out.flags.c_contiguous
        border = np.full((H, W), np.inf, np.float32)
        self.last_branches = branches = np.zeros((H, W), np.uint32)
        opt, st, s = PtoOptions(max_bounces, do_mis, y0, y1, threads), PtoStats(), self.scene_struct(scene)
        ex = ctypes.byref(extras[0]) if extras is not None else None
        if not census:
            fn = self.L.pto_render_ext
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6
            assert fn(ctypes.byref(s), _ptr(cam), n_frames, ctypes.byref(opt), ex, _ptr(out), _ptr(border), _ptr(branches), ctypes.byref(st)) == 0
            return out, st, border
        names = self.census_events()
        table = np.zeros((len(names), 64), np.uint64)
        fn = self.L.pto_render_census_ext
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 7
        assert fn(ctypes.byref(s), _ptr(cam), n_frames, ctypes.byref(opt), ex, _ptr(out), _ptr(border), _ptr(branches), ctypes.byref(st),
                  _ptr(table)) == 0
        return out, st, border, dict(zip(names, table))

    def render_census_ext(self, scene, cam, n_frames, extras=None, **kw):
        return self.render_ext(scene, cam, n_frames, extras, census=True, **kw)

    def trace_path_ext(self, scene, cam, x, y, frame, extras=None, max_bounces=8, do_mis=1):
        opt = PtoOptions(max_bounces, do_mis, 0, 0, 1)
        rad, log = np.zeros(3, np.float32), np.zeros((max_bounces + 1, 16), np.float32)
        s = self.scene_struct(scene)
        fn = self.L.pto_trace_path_ext
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 4
        n = fn(ctypes.byref(s), _ptr(cam), x, y, frame, ctypes.byref(opt), ctypes.byref(extras[0]) if extras is not None else None,
               _ptr(rad), _ptr(log))
        return rad, log[:n]

    def trace_paths_ext(self, scene, cam, xs, ys, frames, extras=None, max_bounces=8, do_mis=1, threads=0):
        """trace_paths with extras: (radiance (n, 3) unclamped, segments (n,), border (n,): the path's smallest distance of a sky
        lookup from a texel border, in texels); the paths' decision hashes are left in self.last_branches, (n,) uint32"""
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32).ravel() for a in (xs, ys, frames))
        n = len(xs)
        assert len(ys) == n and len(frames) == n
        rad, seg, border = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.last_branches = branches = np.zeros(n, np.uint32)
        opt, s = PtoOptions(max_bounces, do_mis, 0, 0, threads), self.scene_struct(scene)
        fn = self.L.pto_trace_paths_ext
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 9
        assert fn(ctypes.byref(s), _ptr(cam), n, _ptr(xs), _ptr(ys), _ptr(frames), ctypes.byref(opt),
                  ctypes.byref(extras[0]) if extras is not None else None, _ptr(rad), _ptr(seg), _ptr(border), _ptr(branches)) == 0
        return rad, seg, border

    def ext_probe(self, extras, op, inputs):
        """pto_ext_probe: inputs (n, <= 8) float32, padded with zeros; returns (n, 8) float32"""
        a = np.asarray(inputs, np.float32)
        inp = np.zeros((len(a), 8), np.float32)
        inp[:, :a.shape[1]] = a
        out = np.zeros((len(a), 8), np.float32)
        fn = self.L.pto_ext_probe
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(ctypes.byref(extras[0]), op, len(a), _ptr(inp), _ptr(out)) == 0
        return out

    # -- probes ----------------------------------------------------------------
    def eval_bsdf(self, albedo, rough, metal, trans, ior, n, v, l, front=True):
        a, n, v, l = (np.ascontiguousarray(q, np.float32) for q in (albedo, n, v, l))
        out = np.zeros(4, np.float32)
        self.L.pto_eval_bsdf(_ptr(a), rough, metal, trans, ior, _ptr(n), _ptr(v), _ptr(l), int(front), _ptr(out))
        return out

    def distribution_ggx(self, n, h, rough):
        n, h = np.ascontiguousarray(n, np.float32), np.ascontiguousarray(h, np.float32)
        return self.L.pto_distribution_ggx(_ptr(n), _ptr(h), rough)

    def power_heuristic(self, nf, fp, ng, gp):
        return self.L.pto_power_heuristic(nf, fp, ng, gp)

    def cosine_direction(self, state):
        st = ctypes.c_uint32(state)
        out = np.zeros(3, np.float32)
        self.L.pto_cosine_direction(ctypes.byref(st), _ptr(out))
        return out, st.value

    def sample_ggx_normal(self, state, n, rough):
        st = ctypes.c_uint32(state)
        n = np.ascontiguousarray(n, np.float32)
        out = np.zeros(3, np.float32)
        self.L.pto_sample_ggx_normal.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
        self.L.pto_sample_ggx_normal(ctypes.byref(st), _ptr(n), rough, _ptr(out))
        return out, st.value
