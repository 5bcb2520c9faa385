"""Gauntlet scenes: small rooms built to take the bounce loop (shade.hip / oracle trace()) through the branches the ordinary
parity scenes never reach, at every bounce. Which branches a render takes is measured by Oracle.render_census
(tests/test_shade_census_host.py holds the coverage condition); nothing here is tuned to a kernel's output.

Both scenes are the room [-1, 1] x [0, 2] x [-1, 1] seen from inside, every wall cut into a grid of patches that cycle through
a list of variants (material, vertex normals, UVs), so that a path meets every variant with the same chance at every bounce.

  gauntlet_materials()  degenerate materials and normals: ior 0 and 1, transmission 0.5 with metallic 0.5, metallic above 1,
                        roughness 0, base colour 1e25 (throughput reaches Inf at the second such hit), a material index past
                        the table, zero and flipped vertex normals, a normal map on triangles with two equal UVs; glass boxes
                        for back faces and total internal reflection; an emissive patch and an opening in the back wall.
  gauntlet_lights()     degenerate lights over a bright closed room with one opening: point lights 100 units from the room's
                        middle (beyond 100 for one half of it), at 1e20 and at NaN; a directional light whose direction
                        vector has length 1e-20; emissive triangles of area ~1e-40, at 1e31 (the distance overflows) and a
                        backdrop of 1e16 behind the opening (hit with t ~ 1e16, area overflows as a light).
"""
import numpy as np

from ptmi import layout, scene_host, scenes

CAMERA = dict(position=(0.15, 1.05, 0.85), forward=(0.0, 0.0, -1.0), fov=1.9)
SIZE = (64, 48)
FRAMES = 8


def camera(width=SIZE[0], height=SIZE[1], **kw):
    return layout.make_camera(width, height, **{**CAMERA, **kw})


def _walls():
    """(origin, du, dv, inward normal) of the six walls of the room"""
    return [((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1)),      # back, z = -1
            ((-1, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, -1)),      # front
            ((-1, 0, -1), (0, 0, 2), (0, 2, 0), (1, 0, 0)),      # -x
            ((1, 0, -1), (0, 0, 2), (0, 2, 0), (-1, 0, 0)),      # +x
            ((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0)),      # floor
            ((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0))]     # ceiling


def _patch_room(variants, grid, holes=()):
    """The walls as grid x grid patches; patch k takes variants[k % len(variants)] = (material, normals, uvs) with normals in
    'keep' / 'zero' / 'flip' / 'tilt' and uvs in 'keep' / 'equal'. holes: (wall, i, j) patches left out."""
    parts, k = [], 0
    for w, (o, du, dv, nrm) in enumerate(_walls()):
        o, du, dv = (np.array(a, np.float64) for a in (o, du, dv))
        for i in range(grid):
            for j in range(grid):
                k += 1
                if (w, i, j) in holes:
                    continue
                mat, normals, uvs = variants[k % len(variants)]
                a, b = o + du * i / grid + dv * j / grid, o + du * (i + 1) / grid + dv * (j + 1) / grid
                q = scenes._quad(a, a + du / grid, b, a + dv / grid, nrm, mat)
                for key in ("n0", "n1", "n2"):
                    if normals == "zero":
                        q[key] = 0.0
                    elif normals == "flip":
                        q[key] = -q[key]
                    elif normals == "tilt":                       # un-normalised and off the geometric normal
                        q[key] = q[key] * 3.0 + np.array([0.9, 0.7, -0.8], np.float32)
                if uvs == "equal":
                    q["uv1"] = q["uv0"]                           # zero UV determinant: the tangent frame divides by zero
                parts.append(q)
    return parts


def _finish(name, parts, mats, punctual, atlas=None):
    """scenes._finish for a scene whose triangles may name a material past the table (the shader reads a zeroed material there,
    pt.wgsl:200): the host's light list refuses such an index, so it is built from a copy in which those triangles name
    material 0, which like the zeroed one does not emit."""
    tris = np.ascontiguousarray(np.concatenate(parts))
    marr = np.array(mats, layout.MATERIAL)
    assert not np.any(marr[0]["emission"])
    nodes, depth = scene_host.build_bvh(tris)
    listed = tris.copy()
    listed["material_index"][listed["material_index"] >= len(marr)] = 0
    return scenes.Scene(name, tris, marr, nodes, scene_host.emissive_lights(listed, marr, punctual), atlas, depth)


def gauntlet_materials():
    atlas, rects = scenes._procedural_atlas(size=128, tile=32, n_sets=1)
    r = rects[0]
    M = scenes._material
    mats = [
        M((0.92, 0.92, 0.92)),                                                   # 0 plain
        M((0.95, 0.95, 0.95), roughness=0.1, transmission=1.0, ior=0.0),         # 1 ior 0
        M((0.95, 0.95, 0.95), roughness=0.1, transmission=1.0, ior=1.0),         # 2 ior 1
        M((0.9, 0.9, 0.9), metallic=0.5, roughness=0.3, transmission=0.5),       # 3 half transmissive, half metallic
        M((0.9, 0.9, 0.9), metallic=1.5, roughness=0.3),                         # 4 diffuse probability negative
        M((0.95, 0.95, 0.95), metallic=1.0, roughness=0.0),                      # 5 roughness clamped to 0.04
        M((1e25, 1e25, 1e25)),                                                   # 6 throughput overflows at the second hit
        M((1, 1, 1), roughness=0.6, albedo_map=r["albedo"], normal_map=r["normal"]),   # 7 normal-mapped
        M((0.8, 0.8, 0.8), emission=(1.0, 0.9, 0.8), strength=4.0),              # 8 light
        M((0.95, 1.0, 0.95), roughness=0.05, transmission=1.0, ior=1.5),         # 9 glass
    ]
    oob = len(mats)
    variants = [(0, "keep", "keep"), (4, "keep", "keep"), (0, "zero", "keep"), (5, "keep", "keep"), (7, "keep", "keep"),
                (0, "flip", "keep"), (3, "keep", "keep"), (6, "keep", "keep"), (oob, "keep", "keep"), (7, "keep", "equal"),
                (0, "tilt", "keep"), (9, "zero", "keep"), (0, "keep", "keep"), (1, "keep", "keep"), (5, "tilt", "keep"),
                (7, "tilt", "keep"), (0, "keep", "keep"), (2, "keep", "keep"), (oob + 7, "keep", "keep")]
    parts = _patch_room(variants, 5, holes={(0, 2, 3), (0, 3, 3)})
    parts.append(scenes._quad((-0.4, 1.999, -0.4), (0.4, 1.999, -0.4), (0.4, 1.999, 0.4), (-0.4, 1.999, 0.4), (0, -1, 0), 8))
    # free-standing boxes, hit from outside and from inside: back faces, total internal reflection, refraction
    parts.append(scenes._box((-0.5, 0.45, -0.35), (0.5, 0.9, 0.5), 9))
    parts.append(scenes._box((0.55, 0.4, -0.45), (0.45, 0.8, 0.45), 1))
    parts.append(scenes._box((0.5, 1.45, -0.3), (0.4, 0.4, 0.4), 3))
    parts.append(scenes._box((-0.55, 1.5, -0.4), (0.4, 0.4, 0.4), 2))
    # one-sided sheets that turn their back to the camera: a back face at bounce 0, opaque and transmissive
    parts.append(scenes._quad((-0.15, 0.9, -0.1), (0.25, 0.9, -0.1), (0.25, 1.3, -0.1), (-0.15, 1.3, -0.1), (0, 0, -1), 0))
    parts.append(scenes._quad((0.3, 0.9, 0.1), (0.6, 0.9, 0.1), (0.6, 1.3, 0.1), (0.3, 1.3, 0.1), (0, 0, -1), 9))
    parts.append(scenes._quad((-0.9, 0.2, 0.3), (-0.9, 0.2, 0.8), (-0.9, 1.0, 0.8), (-0.9, 1.0, 0.3), (-1, 0, 0), 4))
    punctual = np.zeros(2, layout.LIGHT)
    punctual[0]["position"], punctual[0]["light_type"] = (0.1, 1.2, 0.3), layout.LIGHT_POINT
    punctual[0]["color"], punctual[0]["intensity"] = (1.0, 0.9, 0.8), 1.5
    punctual[1]["position"], punctual[1]["light_type"] = (0.2, -1.0, -0.3), layout.LIGHT_DIRECTIONAL
    punctual[1]["color"], punctual[1]["intensity"] = (0.7, 0.8, 1.0), 1.0
    return _finish("gauntlet_materials", parts, mats, punctual, atlas)


def gauntlet_lights():
    M = scenes._material
    mats = [
        M((0.97, 0.97, 0.97)),                                                   # 0 bright wall: paths live long
        M((0.8, 0.8, 0.8), emission=(1.0, 1.0, 1.0), strength=3.0),              # 1 lights
        M((0.97, 0.97, 0.97), metallic=0.6, roughness=0.2),                      # 2
        M((1e25, 1e25, 1e25)),                                                   # 3 Inf throughput for the way out
    ]
    variants = [(0, "keep", "keep")] * 5 + [(2, "keep", "keep"), (0, "zero", "keep"), (3, "keep", "keep")]
    parts = _patch_room(variants, 4, holes={(0, 1, 1), (0, 2, 1), (0, 1, 2), (0, 2, 2)})
    parts.append(scenes._quad((-0.3, 1.999, -0.3), (0.3, 1.999, -0.3), (0.3, 1.999, 0.3), (-0.3, 1.999, 0.3), (0, -1, 0), 1))
    up = np.array([[(0, 1, 0)] * 3], np.float32)
    uv0 = np.zeros((1, 3, 2), np.float32)
    # area ~ 1e-40: |cross|^2 underflows, 1 / area overflows, so does the pdf
    tiny = scenes._tri_array(np.array([[(0.3, 1.0, 0.2), (0.3 + 1e-20, 1.0, 0.2), (0.3, 1.0, 0.2 + 1e-20)]], np.float32), up, uv0, 1)
    tiny["v1"], tiny["v2"] = tiny["v0"] + np.float32([1e-20, 0, 0]), tiny["v0"] + np.float32([0, 0, 1e-20])
    # at 1e31 (never hit: it subtends 1e-6): |to_light|^2 overflows, the distance is Inf, the direction zero
    far = scenes._tri_array(np.array([[(1e31, 1e31, -1e31), (1.00001e31, 1e31, -1e31), (1e31, 1.00001e31, -1e31)]], np.float32),
                            np.zeros((1, 3, 3), np.float32), uv0, 1)
    # behind the opening, covering the directions with x > 0: hit at t ~ 1e16 (1 + t^2 > 2^100), |cross|^2 overflows
    back = scenes._tri_array(np.array([[(0.0, -4e16, -1e16), (8e16, 0.0, -1e16), (0.0, 4e16, -1e16)]], np.float32),
                             np.array([[(0, 0, 1)] * 3], np.float32), uv0, 1)
    parts += [tiny, far, back]
    punctual = np.zeros(6, layout.LIGHT)
    for k, (pos, typ, inten) in enumerate([((0.2, 1.3, 0.1), layout.LIGHT_POINT, 1.0),
                                           ((0.0, 1.0, 100.0), layout.LIGHT_POINT, 4000.0),     # 100 from the room's middle
                                           ((1e20, 0.0, 0.0), layout.LIGHT_POINT, 1.0),
                                           ((np.nan, 1.0, 0.0), layout.LIGHT_POINT, 1.0),
                                           ((0.3, -1.0, 0.2), layout.LIGHT_DIRECTIONAL, 1.0),
                                           ((-2e-21, -1e-20, 3e-21), layout.LIGHT_DIRECTIONAL, 1.0)]):
        punctual[k]["position"], punctual[k]["light_type"] = pos, typ
        punctual[k]["color"], punctual[k]["intensity"] = (1.0, 0.95, 0.9), inten
    return _finish("gauntlet_lights", parts, mats, punctual)


SCENES = {"gauntlet_materials": gauntlet_materials, "gauntlet_lights": gauntlet_lights}


# ---- the fog / sky gauntlet: the branches of `shade`'s ENV and MED instantiations (tests/test_oracle_extras_host.py holds the coverage
# condition, tests/test_gpu_shade_extras.py compares these renders with the oracle's extras) ----
def gauntlet_fog():
    """The room with openings in the back wall and the ceiling (misses at every bounce, the camera ray's too), well-behaved materials
    (no roughness below 0.3 on an opaque surface: a rounding of the scatter point must stay a rounding of the radiance), a glass box
    inside the fog, an emissive patch, a point and a directional light (the API's two punctual kinds; with the emissive triangles
    every kind of light record), a point light of intensity 0 (a sample whose contribution is exactly zero) and an emissive
    triangle at 1e31 that is never hit (its area overflows: a sample whose pdf is NaN)."""
    M = scenes._material
    mats = [
        M((0.9, 0.9, 0.9)),                                                      # 0 bright wall: paths live long
        M((0.8, 0.8, 0.8), emission=(1.0, 0.9, 0.8), strength=3.0),              # 1 lights
        M((0.9, 0.85, 0.8), metallic=0.6, roughness=0.35),                       # 2
        M((0.95, 1.0, 0.95), roughness=0.3, transmission=1.0, ior=1.5),          # 3 glass
        M((0.85, 0.3, 0.3), roughness=0.6),                                      # 4
    ]
    variants = [(0, "keep", "keep")] * 3 + [(2, "keep", "keep"), (4, "keep", "keep")]
    parts = _patch_room(variants, 4, holes={(0, 1, 1), (0, 2, 1), (0, 1, 2), (0, 2, 2), (5, 0, 3), (5, 1, 3), (5, 3, 0), (1, 0, 3)})
    parts.append(scenes._quad((-0.3, 1.999, -0.3), (0.3, 1.999, -0.3), (0.3, 1.999, 0.3), (-0.3, 1.999, 0.3), (0, -1, 0), 1))
    parts.append(scenes._box((-0.25, 0.45, -0.3), (0.45, 0.7, 0.45), 3))        # inside the fog box
    parts.append(scenes._box((0.75, 0.3, 0.7), (0.3, 0.6, 0.3), 2))             # outside it
    far = scenes._tri_array(np.array([[(1e31, 1e31, -1e31), (1.00001e31, 1e31, -1e31), (1e31, 1.00001e31, -1e31)]], np.float32),
                            np.zeros((1, 3, 3), np.float32), np.zeros((1, 3, 2), np.float32), 1)
    parts.append(far)
    punctual = np.zeros(3, layout.LIGHT)
    for k, (pos, typ, inten) in enumerate([((0.3, 1.5, 0.2), layout.LIGHT_POINT, 1.2), ((0.3, -1.0, 0.25), layout.LIGHT_DIRECTIONAL, 0.8),
                                           ((-0.5, 1.0, 0.6), layout.LIGHT_POINT, 0.0)]):
        punctual[k]["position"], punctual[k]["light_type"] = pos, typ
        punctual[k]["color"], punctual[k]["intensity"] = (1.0, 0.95, 0.9), inten
    return _finish("gauntlet_fog", parts, mats, punctual)


FOG_BOX = ((-0.7, 0.0, -1.25), (0.65, 1.45, 0.5))         # a part of the room, and a little beyond the back wall's opening
FOG_CAMERA_INSIDE = dict(position=(0.1, 0.95, 0.3), forward=(0.0, 0.0, -1.0), fov=1.9)      # CAMERA stands outside it
FOG_SKY_INTENSITY, FOG_SKY_ROTATION = 0.5, 0.7


def fog_sky(W=16, H=8):
    """a small non-uniform map: every texel its own radiance, a quarter of them black (never sampled; a miss that adds nothing), two bright"""
    rng = np.random.default_rng(29)
    t = np.ones((H, W, 4), np.float32)
    t[..., :3] = rng.random((H, W, 3), np.float32) * 1.5 + 0.05
    t[rng.random((H, W)) < 0.25, :3] = 0.0
    t[1, 5, :3], t[2, 12, :3] = (9.0, 8.0, 7.0), (4.0, 5.0, 6.0)
    return t


# feature states: what is in place (sky: None / "lookup" / "sampled"; fog: None or the medium), and where the camera stands
_FOG = dict(sigma_t=1.6, albedo=(0.9, 0.0, 0.8), g=0.4, box=FOG_BOX)
FOG_STATES = {
    "sky_lookup": dict(sky="lookup", fog=None, camera=CAMERA),
    "sky_sampled": dict(sky="sampled", fog=None, camera=CAMERA),
    "fog": dict(sky=None, fog=_FOG, camera=CAMERA),
    "fog_sky_sampled": dict(sky="sampled", fog=_FOG, camera=FOG_CAMERA_INSIDE),
    "fog_black": dict(sky="lookup", fog=dict(_FOG, albedo=(0.0, 0.0, 0.0)), camera=FOG_CAMERA_INSIDE),   # every scatter ends its path
}
FOG_GPU_STATES = ["sky_lookup", "sky_sampled", "fog", "fog_sky_sampled"]
# Fewer than FRAMES, for the shares of pixels the comparisons set aside, which must stay under 1 %: with 8 frames 1.1 % (sky sampled) of the
# pixels have a lookup within env_ref.BORDER_BAND of a texel border — a sampled sky is looked up at every vertex for the bounce ray's
# weight —, and with 4 frames 1.0 % (fog and sky, 8 bounces) have a path that takes another branch when logf / expf / atan2f / acosf move by
# 2 ulp; 2 frames give 0.3 % and 0.5 % (tests/test_oracle_extras_host.py prints and holds both)
FOG_FRAMES = 2


def fog_camera(state, width=SIZE[0], height=SIZE[1]):
    return layout.make_camera(width, height, **FOG_STATES[state]["camera"])


def fog_env(state, env_table):
    """the environment of a state as Oracle.extras takes it (env_table: native.env_table), or None"""
    kind = FOG_STATES[state]["sky"]
    if kind is None:
        return None
    t = fog_sky()
    c, prob, alias, _ = env_table(t)
    return dict(texels=t, c=c, prob=prob, alias=alias, intensity=FOG_SKY_INTENSITY, rotation=FOG_SKY_ROTATION, sampled=int(kind == "sampled"))


def fog_gpu_cases():
    """Option sets of tests/test_gpu_shade_extras.py, the same for every state: bounce limits 1, at the repack bounce (no roulette
    yet), one and two above it (roulette on the last bounce; one bounce from the repacked arrays) and 8; both sides of emit_records;
    both traversal picks; the bounce-0 instantiation with planes; one frame and many per batch; a row range ending in a partial wave."""
    rb = repack_bounce()
    auto, glob = 0, 1
    c = lambda mb, overlap, trav, planes, fpb, tile=False: dict(max_bounces=mb, overlap=overlap, traversal=trav, planes=planes,
                                                               frames_per_batch=fpb, tile=tile)
    return [c(1, 0, auto, False, 0), c(1, 2, glob, True, 1), c(rb, 2, auto, True, 0), c(rb, 0, glob, False, 1),
            c(rb + 1, 0, auto, True, 1), c(rb + 2, 2, glob, False, 1), c(8, 2, glob, False, 0), c(8, 0, auto, True, 1),
            c(8, 2, auto, False, 0, tile=True)]


def fog_oracle_renders():
    return sorted({(c["max_bounces"], c["tile"]) for c in fog_gpu_cases()})


def render_fog(oracle, scene, state, env_table, max_bounces, tile, threads=0, ulp_nudge=0, frames=None, do_mis=1):
    """(image, stats, border, census) of one state's render through the oracle's extras"""
    if tile:
        cam, (y0, y1) = fog_camera(state, TILE_CASE["width"], TILE_CASE["height"]), TILE_CASE["rows"]
    else:
        cam, (y0, y1) = fog_camera(state), (0, 0)
    ex = oracle.extras(fog_env(state, env_table), FOG_STATES[state]["fog"], ulp_nudge)
    return oracle.render_census_ext(scene, cam, FOG_FRAMES if frames is None else frames, ex, max_bounces=max_bounces, do_mis=do_mis,
                                    y0=y0, y1=y1, threads=threads)


def gpu_figures_ext(census, max_bounces):
    """gpu_figures with the extras' events: samples at scatter points and of the environment are shadow rays like any other"""
    nee = sum(census[k] for k in ("nee_directional", "nee_point", "nee_emissive", "nee_env", "med_nee_directional", "med_nee_point",
                                  "med_nee_emissive", "med_nee_env"))
    return dict(segments_by_bounce=[int(v) for v in census["segment"][:min(max_bounces, 64)]],
                shadow_rays=int(nee.sum() - census["point_light_beyond_100"].sum()),
                shadow_traced=int(census["would_leave_record"].sum() + census["med_would_leave_record"].sum()))


# ---- the renders of tests/test_gpu_shade_census.py; the coverage condition of tests/test_shade_census_host.py is over their union ----
def repack_bounce():
    """the first bounce that plays Russian roulette (pt.wgsl:699 `bounce > 2`; csrc/pt_device.h pt_repack_bounce): from the next
    bounce on the kernels keep path state in the repacked tail arrays"""
    b = 0
    while not b > 2:
        b += 1
    return b


TILE_CASE = dict(width=60, height=48, rows=(5, 42))       # 37 rows of 60: the bounce-0 queue ends in a partial wave


def gpu_cases():
    """Option sets of the GPU test, the same for every scene. Every value of every factor (overlap, which decides whether `shade`
    emits records or adds to the radiance itself; traversal; max_bounces below, at and above the repack; first-hit planes plus
    moments; frames_per_batch; a row range) appears at least once."""
    rb = repack_bounce()
    auto, glob = 0, 1                                     # native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL
    c = lambda mb, overlap, trav, planes, fpb, tile=False: dict(max_bounces=mb, overlap=overlap, traversal=trav, planes=planes,
                                                               frames_per_batch=fpb, tile=tile)
    return [c(1, 0, auto, False, 0), c(1, 2, glob, True, 1),
            c(rb + 1, 2, glob, True, 1), c(rb + 1, 0, auto, False, 0),
            c(rb + 2, 0, glob, True, 0), c(rb + 2, 2, auto, False, 1),
            c(rb + 3, 2, auto, False, 1), c(rb + 3, 0, glob, True, 0),
            c(8, 0, auto, True, 1), c(8, 2, auto, False, 0),
            c(64, 2, glob, False, 0), c(64, 0, auto, True, 0),
            c(8, 2, auto, False, 0, tile=True), c(rb + 2, 0, glob, True, 1, tile=True)]


def oracle_renders():
    """the distinct oracle renders behind gpu_cases(): (max_bounces, tile)"""
    return sorted({(c["max_bounces"], c["tile"]) for c in gpu_cases()})


def render_census(oracle, scene, max_bounces, tile, threads=0):
    if tile:
        cam, (y0, y1) = camera(TILE_CASE["width"], TILE_CASE["height"]), TILE_CASE["rows"]
    else:
        cam, (y0, y1) = camera(), (0, 0)
    return oracle.render_census(scene, cam, FRAMES, max_bounces=max_bounces, y0=y0, y1=y1, threads=threads)


def gpu_figures(census, max_bounces):
    """What ptmi_stats reports, from a census table:
      segments_by_bounce[b] = segment[b];
      shadow_rays   = next-event samples whose shadow ray the reference traces = nee_* - point_light_beyond_100
                      (`shade` counts a sample it drops, contribution zero or pdf not > 0, as a shadow ray without tracing it);
      shadow_traced = would_leave_record: k_tile_sums adds the popcount of `shade`'s record mask to stats[1] and stats[2]; with
                      overlap != 0 that mask also holds the records of emissive hits and non-finite misses, which `shade` counts
                      in stats[3], and ptmi_get_stats reports stats[1] - stats[3] and stats[2] - stats[3]: neither figure
                      includes them, with any overlap."""
    nee = census["nee_directional"] + census["nee_point"] + census["nee_emissive"]
    return dict(segments_by_bounce=[int(v) for v in census["segment"][:min(max_bounces, 64)]],
                shadow_rays=int(nee.sum() - census["point_light_beyond_100"].sum()),
                shadow_traced=int(census["would_leave_record"].sum()))


# ---- what the device's logf / expf / atan2f / acosf, 1 - 2 ulp from libm's, may change in a render with fog: measured on the oracle ----
NUDGES = (-2, -1, 1, 2)
FLIP_FROM = 1e-2          # no pixel whose paths all kept their branches comes within a factor 100 of this deviation


def pixel_deviation(img, ref):
    """(H, W): per pixel the largest |img - ref| / max(|ref|, 1) of the three channels (medium_ref.deviation's scale)"""
    a, r = np.asarray(img)[..., :3].astype(np.float64), np.asarray(ref)[..., :3].astype(np.float64)
    assert np.isfinite(a).all() and np.isfinite(r).all()
    return (np.abs(a - r) / np.maximum(np.abs(r), 1.0)).max(axis=-1)


def rendered_rows(tile):
    return slice(*TILE_CASE["rows"]) if tile else slice(None)


def nudge_study(oracle, scene, state, env_table, max_bounces, tile, threads=0):
    """One render of a fog state with ulp_nudge 0 (the reference) and with every value of NUDGES: dict(ref, stats, border, census of the
    reference; dev (H, W): the largest deviation of any variant; flips: the pixels where a path of some variant took another branch
    than the reference's, by the oracle's hash of a path's decisions (pto_render_ext's `branches`), whatever that did to the pixel;
    drift: the largest deviation of the others, which is rounding)"""
    ref, st, border, cen = render_fog(oracle, scene, state, env_table, max_bounces, tile, threads)
    branches = oracle.last_branches
    dev, flips = np.zeros(ref.shape[:2]), np.zeros(ref.shape[:2], bool)
    for k in NUDGES:
        img = render_fog(oracle, scene, state, env_table, max_bounces, tile, threads, ulp_nudge=k)[0]
        dev = np.maximum(dev, pixel_deviation(img, ref))
        flips |= oracle.last_branches != branches
    ref.setflags(write=False)
    return dict(ref=ref, stats=st, border=border, census=cen, dev=dev, flips=flips, drift=float(dev[~flips].max()))
