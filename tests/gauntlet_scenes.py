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
