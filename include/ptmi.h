/*
 * ptmi.h — C ABI of the MI355X wavefront path tracer (libptmi.so).
 *
 * Drop-in boundary for the reference's compute pass: the bind group of
 * src/renderer/renderer.ts:368-381 (bindings 0..6 of src/shader/pt.wgsl:104-110)
 * plus the per-frame camera write and dispatch of renderer.ts:403-431. Every
 * blob is the exact WGSL-layout byte image the reference uploads
 * (include/ptmi_layout.h). Plain pointers and sizes only — no HIP or torch
 * types; a caller binds this with cgo / JNI / N-API / ctypes.
 *
 * There is no CPU backend behind this ABI. ptmi_create fails when no gfx950
 * device is present.
 *
 * All functions return 0 on success and a negative PTMI_E_* code on failure;
 * ptmi_last_error(ctx) (ctx may be NULL for creation errors) gives the text.
 * A context is not thread-safe (like the reference's single-queue Renderer);
 * work is ordered on one HIP stream per context.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>
#include "ptmi_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_ABI_VERSION 4

enum {
    PTMI_OK = 0,
    PTMI_E_INVALID = -1,     /* bad argument / malformed blob */
    PTMI_E_NODEVICE = -2,    /* no usable GPU */
    PTMI_E_HIP = -3,         /* a HIP runtime call failed */
    PTMI_E_STATE = -4,       /* call order (e.g. dispatch before upload/resize) */
    PTMI_E_UNSUPPORTED = -5  /* scene exceeds an implementation limit */
};

enum { PTMI_ATLAS_RGBA16F = 1, PTMI_ATLAS_RGBA32F = 2 };   /* reference uploads rgba16float (renderer.ts:246-261) */
/* AUTO: the scene's traversal image lives in LDS when it fits, else it is walked from global memory. GLOBAL / LDS force
 * one (LDS fails for scenes that do not fit). GLOBAL_EXACT: global memory, on the exact 64-byte nodes instead of the
 * quantised 32-byte image GLOBAL uses (same results; kept for tests and comparisons). */
enum { PTMI_TRAVERSAL_AUTO = 0, PTMI_TRAVERSAL_GLOBAL = 1, PTMI_TRAVERSAL_LDS = 2, PTMI_TRAVERSAL_GLOBAL_EXACT = 3 };

typedef struct ptmi_ctx ptmi_ctx;

/* Runtime options. The reference fixes these at shader-compile time
 * (pt.wgsl:5 MAX_BOUNCES = 8, :636 DO_MIS = true). */
typedef struct ptmi_options {
    uint32_t max_bounces;       /* 1..64; default 8 */
    uint32_t do_mis;            /* 0/1; default 1 */
    uint32_t tile_y0, tile_y1;  /* rows [y0,y1) this context renders; y1 = 0 -> height. Other rows are untouched */
    uint32_t frames_per_batch;  /* frames traced together as one wavefront batch; 0 -> auto (up to 64 frames / ~128 Mi paths, ~23 GB of
                                   path state at 1920x1080; a dispatch of fewer frames is one smaller batch) */
    uint32_t traversal;         /* PTMI_TRAVERSAL_*; AUTO picks LDS when the scene fits */
    uint32_t cull;              /* 1 (default): ordered traversal with conservative distance cull;
                                   0: every box-overlapping leaf is tested, as pt.wgsl:248-291 does */
    uint32_t timing;            /* 0: none; 1: HIP events around each dispatch (gpu_ms); 2: also around every
                                   extend launch (extend_ms); 3: around every kernel launch (extend, shade, shadow,
                                   raygen, compaction, accumulate — the per-kernel times then add up to gpu_ms).
                                   Each event pair costs a few microseconds of stream time. */
    uint32_t keep_reference_tree; /* read by ptmi_upload_scene. 0 (default): when every node box of the uploaded BVH contains
                                   its children's boxes, traversal walks a SAH hierarchy rebuilt over the SAME leaves (same
                                   results, about half the box tests); 1: always walk the tree as uploaded */
    uint32_t tile_parts, tile_part, tile_strip; /* interleaved row sharding: with tile_parts = N > 1 this context renders, of the
                                   rows [tile_y0, tile_y1), the strips of tile_strip rows (0 -> 1) numbered tile_part,
                                   tile_part + N, ... — N contexts with tile_part = 0..N-1 cover the range exactly once, each
                                   with an even sample of the picture. 0 / 1 = all rows of the range (default) */
    uint32_t perf_mode;         /* 0 (default): the parity arithmetic of DESIGN.md §3 — results equal the oracle's bit for bit.
                                   1: `shade` may use the device's fast reciprocal / reciprocal square root / square root
                                   (1 ulp) instead of the correctly rounded forms. Same RNG streams and control flow; radiance
                                   agrees statistically (tests/test_gpu_perf_mode.py), not bit for bit. Never the headline. */
    uint32_t reserved_a;        /* must be 0 (ABI <= 3: ray_sort — survivors grouped by direction octant; measured slower and removed,
                                   profiles/README.md "Removed in round 4") */
    uint32_t overlap;           /* 0: every kernel of a dispatch on the context's one stream, in order; 1: the any-hit `shadow` kernel of
                                   bounce b runs on a second stream beside `extend` / `shade` of bounce b + 1 — it is
                                   the only kernel that adds to the radiance then, in bounce order, so results are unchanged;
                                   2 = library default (currently 1) */
    uint32_t reserved_b[4];     /* must be 0 (ABI 3: worklist, tails, state, pipeline — four ways to compute the same bits, each measured
                                   slower or level and removed in round 4; numbers and the last commit that had them: profiles/README.md) */
    uint32_t tree_builder;      /* read by ptmi_upload_scene: who builds the hierarchy the traversal walks (when keep_reference_tree = 0).
                                   1 = the host. leaves = 1: full-sweep / binned SAH + rotations over the uploaded leaves (137 ms for the
                                   334 174 leaves of the 1 M-triangle scene); leaves = 2: the same over the triangles, collapsed into own
                                   leaves (313 ms for that scene).
                                   2 = the GPU. leaves = 1: Morton-order linear BVH over the uploaded leaves (radix sort + radix tree +
                                   bottom-up fit, a few ms); leaves = 2: for scenes above 4 096 triangles, PLOC clustering of the
                                   triangles (Morton-sorted, nearest neighbour in a window of +-16), collapsed with the host's cost model,
                                   padded and quantised on the device; smaller scenes, which get the 16-bit images and whose LDS variant
                                   turns on a few tens of nodes, keep the host builder (a few ms).
                                   Either way the results are the same (any topology over conservative boxes); only the
                                   work per ray differs (profiles/README.md). A device build that fails (allocation, more than 60 levels)
                                   falls back to the host; ptmi_stats.tree_builder_used reports who built. 0 = library default (1) */
    /* ABI 4 */
    uint32_t leaves;            /* read by ptmi_upload_scene: which leaves the traversal kernels test triangles in.
                                   1 = the uploaded BVH's own leaves (bvh.ts:86-127 cuts <= 4 triangles from 11 equal-count candidates on one
                                       axis): a triangle is tested iff the box of ITS reference leaf passes, exactly as pt.wgsl:248-291 does;
                                   2 = the library's own leaves: a full-sweep SAH hierarchy over the TRIANGLES (leaf_tris at most per leaf),
                                       boxes padded outward so that they are conservative for the kernels' fused slab test. A ray then tests
                                       a quarter of the triangles (Cornell: 9.8 -> 2.4 per closest-hit ray). A sliver (longest edge
                                       squared above 16 x twice its area) enters the hierarchy with its reference leaf's box. The closest
                                       hit is verified against the reference leaf's box before it is reported, and a ray whose winner fails
                                       that test — or whose direction has a zero / non-finite component, or whose origin lies far outside
                                       the scene — is traced again over the uploaded tree. Results equal mode 1's on every ray of the
                                       benchmark renders and on slivers, but NOT on every ray: a ray within ~1e-2 rad of an ordinary
                                       triangle's plane can be accepted by Moller-Trumbore outside the triangle's padded box, and then
                                       the own leaves miss a hit the reference reports (measured: 1 - 4 closest hits per 10^5 rays
                                       aimed at triangle edges at 1e-7 ... 1e-2 rad, none at larger angles).
                                       On scenes made mostly of slivers the own leaves do more work than mode 1 (a strip floor: about
                                       2 x the closest-hit and 8 x the any-hit estimate). 1 is the strict mode;
                                   0 = library default (2) */
    uint32_t leaf_tris;         /* leaves = 2: most triangles per own leaf, 1 .. 32; 0 = library default (measured: profiles/README.md) */
    uint32_t reserved[1];       /* must be 0 */
} ptmi_options;

typedef struct ptmi_stats {
    uint64_t paths;             /* (pixel, frame) samples traced since the last reset (adaptive dispatches: those of the listed pixels) */
    uint64_t segments;          /* path segments = bounce-loop iterations reaching sceneIntersect (pt.wgsl:643-644) */
    uint64_t shadow_rays;       /* shadow traversals of the reference (pt.wgsl:392/421/463). Those whose contribution is
                                   exactly zero (light behind the surface) are counted here but not traced: they cannot
                                   change the radiance */
    uint64_t dispatches;        /* ptmi_dispatch and ptmi_dispatch_adaptive calls */
    uint64_t frames;            /* frames traced by ptmi_dispatch */
    uint64_t segments_by_bounce[64];
    double   gpu_ms;            /* device time of all dispatches (HIP events on the context's stream) */
    double   extend_ms;         /* ... of the closest-hit traversal kernel only, and its launch count */
    uint64_t extend_launches;
    double   shade_ms;
    double   shadow_ms;
    uint32_t bvh_depth;         /* of the uploaded tree */
    uint32_t traversal_used;    /* PTMI_TRAVERSAL_GLOBAL or _LDS */
    uint32_t frames_per_batch_used;
    uint32_t radiance_stride_bytes;  /* of the last dispatch's per-path radiance buffer: 12, or 16 for scenes walked from memory (was reserved) */
    /* ABI 2 */
    uint64_t shadow_traced;     /* shadow records the any-hit kernel actually traced (shadow_rays minus the zero-contribution ones) */
    uint64_t shade_launches, shadow_launches;
    double   raygen_ms, compact_ms, accumulate_ms;   /* timing >= 3 */
    double   upload_ms;         /* wall time of the last ptmi_upload_scene, and its parts: validation + traversal image, */
    double   upload_tree_ms;    /* ... the hierarchy rebuilt over the uploaded leaves, */
    double   upload_copy_ms;    /* ... host-to-device copies */
    /* ABI 4 (ABI 3 had worklist_used, tails_used, state_used, pipeline_used here) */
    uint32_t leaves_used;       /* 1 / 2: ptmi_options.leaves as the uploaded scene's traversal image was built */
    uint32_t leaf_tris_used;    /* most triangles in a leaf of that image */
    uint32_t extend_variant, shadow_variant;   /* of the last dispatch, the memory variant the closest-hit / any-hit kernel ran as:
                                                * variant number * 10 + workgroups per CU (e.g. 102: variant 10 with two) */
    /* leaves = 2: closest hits / occluders whose reference leaf's box did not pass and rays that were therefore traced again over the
     * uploaded tree (both kernels together), since the last reset. Also counted: a lane whose stack ran out and that reported its hit
     * unverified (cannot happen while the stack is deeper than the tree; counted so that a count equal to tools/own_sim.c's — whose
     * stack never runs out — shows it did not) */
    uint64_t verify_failed;
    uint32_t tree_builder_used; /* who built the hierarchy the last upload's regular rays walk: 1 the host, 2 the device (both leaf modes);
                                   0 none: the uploaded tree is walked as it is (keep_reference_tree, an empty scene, a tree whose
                                   root is a leaf — there is no hierarchy over a single leaf —, a tree with non-finite boxes) */
    uint32_t shade_tables;      /* of the last dispatch (was reserved): bits 0-23 the bytes of LDS a workgroup of `shade` may fill with the
                                   scene's materials, lights and light triangles; bit 28 set: the materials were served from LDS, bit 29: the
                                   lights and their triangles (a table that does not fit is read from memory; same results either way) */
} ptmi_stats;

/* ---- lifetime ----------------------------------------------------------- */
int ptmi_abi_version(void);
/* device_ordinal >= 0 selects the HIP device. Replaces requestAdapter/requestDevice +
 * createPipelines (renderer.ts:203-214, :513-533). */
int ptmi_create(int device_ordinal, ptmi_ctx **out);
int ptmi_destroy(ptmi_ctx *ctx);                              /* renderer.ts:482-494 destroy() */
const char *ptmi_last_error(const ptmi_ctx *ctx);

/* ---- resources (createBuffers, renderer.ts:242-355) --------------------- */
/* The four storage buffers of bindings 1, 2, 4, 5. Host blobs are copied during the call. */
int ptmi_upload_scene(ptmi_ctx *ctx,
                      const ptmi_triangle *triangles, uint32_t n_triangles,
                      const ptmi_material *materials, uint32_t n_materials,
                      const ptmi_bvh_node *bvh_nodes, uint32_t n_nodes,
                      const ptmi_light *lights, uint32_t n_lights);
/* Binding 6. texels: width*height RGBA, row-major, texel (0,0) first. NULL/0 removes the atlas. An unknown format or a
 * width*height*texel size that does not fit in size_t gives PTMI_E_INVALID; a call that fails leaves the current atlas in place. */
int ptmi_upload_atlas(ptmi_ctx *ctx, const void *texels, uint32_t width, uint32_t height, int format);
/* Binding 0: (re)allocates the width*height*16-byte output buffer, zero-filled (renderer.ts:272-279, :496-510). A failed call
 * leaves the previous state in place: the size, every plane with its contents, and the output binding. */
int ptmi_resize(ptmi_ctx *ctx, uint32_t width, uint32_t height);
int ptmi_set_options(ptmi_ctx *ctx, const ptmi_options *opt);
int ptmi_get_options(const ptmi_ctx *ctx, ptmi_options *opt);

/* ---- the compute pass (updateCamera + dispatch, renderer.ts:403-431) ---- */
/* Traces n_frames consecutive frames starting at camera->frame_index (one sample per
 * pixel per frame, pt.wgsl:719) and folds them into the output buffer in frame
 * order (pt.wgsl:753-761). Equals n_frames single-frame dispatches with the
 * frame index incremented by the caller (renderer.ts:453). Asynchronous. */
int ptmi_dispatch(ptmi_ctx *ctx, const ptmi_camera *camera, uint32_t n_frames);
int ptmi_synchronize(ptmi_ctx *ctx);

/* ---- camera projections: orthographic and equirectangular beside the pinhole ----------------
 * The camera record carries its projection in the two words at offset 88, which the reference pads with (ptmi_layout.h: PTMI_PROJ_*,
 * ptmi_camera_set_projection). They are honoured only while the context's switch is on. While it is off, the default, the words are
 * not read, every launch is the kernel it was and every result keeps its bits: a caller that leaves garbage in the padding is
 * unaffected. While it is on, every entry that takes a camera - ptmi_dispatch, ptmi_dispatch_adaptive, ptmi_reproject (both cameras),
 * ptmi_debug_raygen, ptmi_debug_center_rays and their ptmi_multi counterparts - reads word 0:
 *   PTMI_PROJ_PERSPECTIVE   the kernels of the switch off; word 1 is not read.
 *   PTMI_PROJ_ORTHOGRAPHIC  word 1 = the bits of ymag, the half-height in world units; not finite or not > 0: PTMI_E_INVALID.
 *   PTMI_PROJ_EQUIRECT      word 1 is not read; fov and aspect are not read.
 *   anything else           PTMI_E_INVALID.
 * A rejected camera means nothing was enqueued or written.
 * The rays, operation by operation in the kernels' float32 (pt_math.h: scale3 / add3 are per-component * and +, normalize3 and
 * sincos are the kernels' own, ptmi_debug_math op 5 / 6), with uvx = (px / width) * 2 - 1, uvy = (py / height) * 2 - 1 at the
 * point (px, py) = (x + jitter x, y + jitter y) of pixel (x, y), as for the pinhole:
 *   orthographic   a = ((right * uvx) * ymag) * aspect,  b = (up * uvy) * ymag,  origin0 = (position + a) + b,  dir = normalize(forward)
 *                  (the pinhole's expression with ymag where tan(fov / 2) stands, applied to the origin)
 *   equirect       lon = uvx * pi, lat = uvy * (pi * 0.5f), (so, co) = sincos(lon), (sl, cl) = sincos(lat),
 *                  dir = normalize((forward * (cl * co) + right * (cl * so)) + up * sl),  origin0 = position
 *                  (forward at the image centre, right at a quarter of the width to its right, up at the top row)
 * The lens (aperture > 0) is the pinhole's with origin0 where position stands: the focal point is origin0 + dir * focus_distance,
 * the disc lies in right / up, and the same two draws are taken. The centre rays of ptmi_reproject use the same formulas at
 * (x + 0.5, y + 0.5) without the lens. Both projections expect forward, right, up orthonormal to within rounding; this is not
 * validated. Consequence: pixel (x, y, frame) of either projection is pixel (x, y, frame) of a pinhole camera with position = origin0,
 * forward = the direction before normalize, fov = 0 and everything else equal - the same seed, draws, lens and path, bit for bit
 * (where no component of that forward is a zero: the pinhole adds +0 to it).
 * ptmi_reproject: an orthographic `from` projects sx = dot(v, right) / (ymag * aspect), sy = dot(v, up) / ymag where zf > 0, and its
 * depth is dist = zf - the t along a ray that starts on the camera plane - in the tolerance test and the motion plane's z. An
 * orthographic `to` needs only its centre rays, so any pairing of pinhole and orthographic works. An equirectangular `from` or `to`
 * is PTMI_E_INVALID with nothing written: its inverse needs atan2 / asin, which are outside the arithmetic contract.
 * on: 0 or 1 (else PTMI_E_INVALID). Synchronises. Nothing is allocated either way. The ABI version stays 4: the record's size and
 * members are unchanged. */
int ptmi_set_projections(ptmi_ctx *ctx, uint32_t on);
int ptmi_get_projections(const ptmi_ctx *ctx, uint32_t *on);

/* ---- lightmap baking: paths that start at surface texels instead of a camera -----------------
 * A bake answers "what light arrives at this surface?": the output buffer is read as a lightmap, texel (x, y) = entry y * width + x
 * (row 0 at the bottom, as everywhere) standing for lightmap coordinate ((x + 0.5) / width, (y + 0.5) / height). The caller says where
 * each texel lies in the scene (ptmi_bake_texel, ptmi_layout.h: position, normal, covered); ptmi/bake.py and host/bake.js rasterise a
 * mesh's lightmap UVs into such records.
 *
 * ptmi_upload_bake_surface: width x height records, which must be the context's current size (else PTMI_E_INVALID). A covered record
 * whose position is not finite, or whose normal is not finite or has a squared length (float32) of zero or infinity, is
 * PTMI_E_INVALID, and the surface that was in place stays in place. The device keeps the records (width * height * 32 bytes) and the
 * list of the covered texels in ascending texel index, which is the order paths and folds walk them in. texels NULL removes the
 * surface; so does a ptmi_resize to another size. Synchronises.
 *
 * ptmi_dispatch_bake: n_frames frames of every covered texel, from params->first_frame on, through the bounce loop of ptmi_dispatch
 * and everything that belongs to it: batch sizing, the traversal pick, the side stream, statistics, sky, medium, both alpha modes,
 * in-place edits and poses. Only the first ray differs. For covered texel (x, y) at frame f, in the kernels' float32 (pt_math.h):
 *   rng = seed(x, y, f);  r1 = rand(rng);  r2 = rand(rng)              the pinhole's two jitter draws, and nothing else
 *   n = normalize(normal);  (sp, cp) = sincos((2 pi) * r1);  z = sqrt(1 - r2);  sr = sqrt(r2)
 *   (T, B) = the frame shade builds around n (pt.wgsl:624-634);  raw = lincomb3(T, cp * sr, B, sp * sr, n, z)
 *   origin = fma(raw, bias, position) per component;  dir = normalize(raw)
 * which is the continuation of a path that bounced diffusely at the texel (pt.wgsl:299-307, :691 with bias where EPSILON stands), so
 * a bake inherits the renderer's self-intersection behaviour. It is also pixel (x, y, f) of a pinhole camera with position = origin,
 * forward = raw, fov = 0, aperture = 0: the same seed, draws and path, bit for bit (where no component of raw is a zero).
 * Per sample the clamp is the reference's 2.5, and the output buffer holds the running mean of the incoming radiance under
 * cosine-weighted directions: E / pi, the radiance a white Lambertian texel would reflect; the engine multiplies by albedo. Frame
 * first_frame = 0 overwrites, as for a camera. Uncovered texels are neither read nor written. While the moments plane is on
 * (ptmi_set_moments), covered texels fold their moments too, with the count first_frame + n_frames.
 * LIMIT: punctual lights reach a texel only through later bounces - a ray cannot hit them, and there is no next-event sample at the
 * texel itself. Emissive triangles and the sky are seen directly. This is the usual baked-indirect split.
 * params NULL: first_frame 0, bias 1e-6f (the reference's EPSILON). bias must be finite and >= 0 and is used exactly as given; the
 * reserved words must be 0. PTMI_E_INVALID, with nothing enqueued or written: no surface in place, a first-hit plane on
 * (ptmi_set_aovs mask non-zero), tile options that do not cover the whole frame, a bad bias. n_frames = 0 or no covered texel:
 * PTMI_OK, nothing written. Asynchronous, like ptmi_dispatch.
 *
 * ptmi_bake_dilate: gutter fill. Leaves the output buffer alone and writes a dilated copy to dst_rgba (width * height * 4 floats,
 * else PTMI_E_INVALID); needs a surface. Per texel a state: 1 covered, 2 filled by an earlier pass, 0 empty. Pass k: every state-0
 * texel looks at its 8 neighbours in the order dy = -1, 0, 1 outer, dx = -1, 0, 1 inner (itself and anything outside the frame
 * skipped), takes those whose state was non-zero BEFORE this pass, sums their rgb in that order in float32 starting from +0, and if
 * any were taken becomes sum / (float)count (one IEEE division per channel) with state 2. dst.w carries the state as a float; rgb of
 * state-0 texels is 0. passes = 0 is the masked copy. Synchronises.
 *
 * ptmi_debug_bake_rays: the first ray of texel (xs[i], ys[i]) at frames[i] under params, as ptmi_debug_raygen returns a camera's:
 * origin, direction, and the RNG state it leaves. An uncovered texel returns zeros; a texel outside the surface is PTMI_E_INVALID.
 * The ABI version stays 4: new calls only. */
typedef struct ptmi_bake_params { uint32_t first_frame; float bias; uint32_t _reserved[2]; } ptmi_bake_params;
struct ptmi_bake_status { uint32_t present, width, height, covered; };
int ptmi_upload_bake_surface(ptmi_ctx *ctx, const ptmi_bake_texel *texels, uint32_t width, uint32_t height);
int ptmi_dispatch_bake(ptmi_ctx *ctx, const ptmi_bake_params *params, uint32_t n_frames);
int ptmi_bake_status(ptmi_ctx *ctx, struct ptmi_bake_status *out);
int ptmi_bake_dilate(ptmi_ctx *ctx, uint32_t passes, float *dst_rgba, size_t n_floats);
int ptmi_debug_bake_rays(ptmi_ctx *ctx, const ptmi_bake_params *params, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                         const uint32_t *frames, float *o3, float *d3, uint32_t *rng);

/* ---- denoising a lightmap: a chart-aware a-trous filter over the bake surface ------------------
 * ptmi_bake_denoise filters the output buffer, read as the lightmap of the surface in place, with the 5x5 B3-spline a-trous wavelet of
 * ptmi_denoise (taps at offsets of 2^i texels in pass i), guided by the surface instead of by first-hit planes: a bake has none, and
 * neighbours in a lightmap atlas need not be neighbours in the scene. It reads the surface's records, the output buffer and the
 * moments plane (ptmi_set_moments must be on during the bake, so that covered texels have folded theirs) and writes none of them; the
 * result is a context-owned plane. Uncovered texels are never read. Single device, like the rest of the bake. Not on the parity path:
 * its contract is a tolerance against tests/bake_denoise_ref.py, which restates every expression (csrc/bake_denoise.hip lists them):
 *   prepass  per covered texel: n^ = normal / |normal|; the footprint f = the smallest non-zero distance to a covered 4-neighbour's
 *            position (0 if there is none); variance of the mean = max(0, m2 - m1^2) / max(frames, 1) from the moments plane
 *   pass i   a covered centre p with finite values takes the taps q inside the map that are covered and finite, each weighted
 *            h h w_n w_x w_l:  w_n = max(0, n^_p . n^_q)^phi_normal,
 *            w_l = exp(-|l_p - l_q| / (phi_color sqrt(g3x3(var)_p) + 1e-6)) as in ptmi_denoise,
 *            w_x = exp(-e / (phi_position f_p + 1e-6)),  e = max(|n^_p . D|, |D| - 4 |offset| f_p),  D = P_q - P_p, |offset| in texels.
 *            colour = sum w c / sum w, variance = sum w^2 var / (sum w)^2. A covered centre that is not finite keeps its value.
 *            A tap on the centre's plane within 4 footprints per texel of offset (the chart stretch tolerated) has e = 0; a parallel
 *            surface is cut by the plane term, a far part of the same plane by the distance term; a tap of another chart that does
 *            agree in the scene is accepted, which is what heals seams.
 *   then     (rgb, 1) for covered texels and zeros for the others, and `dilate` passes of ptmi_bake_dilate's rule on that plane.
 * dst_rgba NULL: asynchronous on the context's stream (read the result through ptmi_bake_denoised_device_ptr after
 * ptmi_synchronize); else synchronises and copies width * height float4, w being the state ptmi_bake_dilate documents (1 covered,
 * 2 filled, 0 empty). PTMI_E_INVALID: no surface in place, a negative or non-finite phi, iterations > 10, a non-zero reserved word, a
 * wrong n_floats. PTMI_E_STATE: the moments plane off, no output buffer. A refused call writes nothing. */
typedef struct ptmi_bake_denoise_params {
    uint32_t iterations;    /* 1..10; 0 -> 5 */
    uint32_t dilate;        /* gutter passes on the filtered result, ptmi_bake_dilate's rule; 0: none */
    float phi_color;        /* 0 -> 4 */
    float phi_normal;       /* 0 -> 128 */
    float phi_position;     /* 0 -> 1, in texel footprints */
    uint32_t reserved[3];   /* must be 0 */
} ptmi_bake_denoise_params;
int ptmi_bake_denoise(ptmi_ctx *ctx, const ptmi_bake_denoise_params *params, float *dst_rgba, size_t n_floats);
/* the filtered plane's device address; NULL before the first ptmi_bake_denoise since the last ptmi_resize */
void *ptmi_bake_denoised_device_ptr(ptmi_ctx *ctx);

/* ---- light probes: radiance gathered at points in free space -----------------------------------
 * A probe answers "what light arrives at this point?", for the objects that move through a baked scene. The context's frame
 * (ptmi_resize) is read as the probe ATLAS: with tile size N (a power of two, 4 ... 64; 8 is the practical minimum, see the errors
 * below), cols = width / N and rows = height / N, probe i owns the N x N texels of tile (i % cols, i / cols), row 0 at the bottom as
 * everywhere. A texel of a tile stands for a solid angle about the probe under the octahedral map below (the one DDGI atlases use).
 *
 * ptmi_upload_probes: count probes (ptmi_probe, ptmi_layout.h: position, enabled) with tile size `tile`. PTMI_E_INVALID, with the
 * probes that were in place left in place: tile not a power of two in [4, 64]; the context's width or height not a multiple of tile
 * (or no output buffer); count 0 or above cols * rows; an enabled probe whose position is not finite. The device keeps the records,
 * the two tables below and the list of the frame indices of every texel of every enabled probe in ascending frame index, which is
 * the order paths and folds walk them in. probes NULL removes the probes; so does a ptmi_resize to another size. Probes and a bake
 * surface are independent state. Synchronises.
 *
 * ptmi_dispatch_probes: n_frames frames of every listed texel, from params->first_frame on, through the bounce loop of ptmi_dispatch
 * exactly as ptmi_dispatch_bake runs it: batch sizing, the 2^32 limit, statistics over the listed texels, the moments fold while
 * ptmi_set_moments is on, sky, medium, both alpha modes, edits and poses. Only the first ray differs. For texel (x, y) of an enabled
 * probe at frame f, in the kernels' float32, each operation rounded once and none fused (pt_math.h):
 *   rng = seed(x, y, f);  r1 = rand(rng);  r2 = rand(rng)                  the pinhole's two jitter draws, and nothing else
 *   s = 2 / N (exact);  a = ((float)(x % N) + r1) * s - 1;  b = ((float)(y % N) + r2) * s - 1        sum, product, difference
 *   w = (1 - |a|) - |b|
 *   if (w < 0) { a' = copysign(1 - |b|, a);  b' = copysign(1 - |a|, b); } else { a' = a;  b' = b; }
 *   raw = (a', b', w) in world axes;  origin = position;  dir = normalize(raw)
 * It is pixel (x, y, f) of a pinhole camera with position = origin, forward = raw, fov = 0, aperture = 0: the same seed, draws and
 * path, bit for bit (where no component of raw is a zero). Per sample the clamp is the reference's 2.5, and a texel of the output
 * buffer holds the running mean of the incoming radiance over the texel's footprint. Frame first_frame = 0 overwrites. Texels of
 * disabled probes and of tiles past count are neither read nor written.
 * LIMIT: punctual lights are deltas and reach a probe only through later bounces - a ray cannot hit them, and there is no next-event
 * sample at the probe itself. Emissive triangles and the sky are seen directly.
 * params NULL: first_frame 0; the reserved words must be 0. PTMI_E_INVALID, with nothing enqueued or written and the statistics as
 * they were: no probes in place, a first-hit plane on (ptmi_set_aovs mask non-zero), tile options that do not cover the whole frame,
 * a non-zero reserved word. n_frames = 0 or no enabled probe: PTMI_OK, nothing written. Asynchronous, like ptmi_dispatch.
 *
 * THE TABLES depend on N only; they are built on the host in float64 with + - * / and sqrt alone and rounded once to float32. For
 * texel t = ty * N + tx, its centre put through the map above: a = (tx + 0.5) * (2 / N) - 1, b likewise from ty, w, a', b' as above,
 *   p = (a', b', w);  len = sqrt((a' a' + b' b') + w w);  d_t = p / len (three divisions)
 *   dw_t = (4 / (N N)) / ((len len) len)                                    the map's Jacobian, du dv / |p|^3
 *   every dw_t is then multiplied by (4 pi) / sum, the sum taken over ascending t from 0, pi = 3.141592653589793
 *   basis[t][k] = Y_k(d_t) * dw_t, with (x, y, z) = d_t and
 *     Y_0 = 0.28209479177387814
 *     Y_1 = 0.4886025119029199 * y        Y_2 = 0.4886025119029199 * z        Y_3 = 0.4886025119029199 * x
 *     Y_4 = (1.0925484305920792 * x) * y  Y_5 = (1.0925484305920792 * y) * z  Y_6 = 0.31539156525252005 * ((3 * z) * z - 1)
 *     Y_7 = (1.0925484305920792 * x) * z  Y_8 = 0.5462742152960396 * (x * x - y * y)
 * The rule is second order in 1 / N. Largest absolute SH9 coefficient error against the analytic value, N = 8 / 16 / 32 / 64:
 * constant radiance 0.085 / 0.020 / 0.0050 / 0.0012, a clamped cosine 0.029 / 0.0053 / 0.0014 / 0.00034; N = 4 is allowed but
 * coarse (1.4 on the constant).
 * ptmi_debug_probe_tables (host only, no context): dir_dw4 = N * N * 4 floats (d_t, dw_t), basis9 = N * N * 9 floats; either may be
 * NULL. Any power of two in [2, 64] (2 is the smallest irradiance tile's table); else PTMI_E_INVALID.
 *
 * ptmi_probe_sh: c[i][k][ch] = sum_t basis[t][k] * L_i[t][ch] over probe i's tile of the output buffer as it stands (owned or bound,
 * read in place): count * 27 floats, k major and rgb minor; a disabled probe gives zeros. One wave per probe, in float32: lane l
 * starts from +0 and takes texels t = l, l + 64, ... in ascending order, each term acc = acc + (basis * L) - a rounded product, then
 * a rounded sum, never fused; then for s = 32, 16, ..., 1: v[l] = v[l] + v[l + s]; lane 0 holds the result. Synchronises.
 * PTMI_E_INVALID: no probes in place, n_floats != count * 27.
 *
 * ptmi_probe_irradiance: per probe an m x m octahedral tile (m a power of two, 2 ... 16, m <= N; else PTMI_E_INVALID), texel j =
 *   (1 / pi) * sum_t max(0, dot(n_j, d_t)) * dw_t * L_i[t][ch]
 * with n_j the float32 direction d_j of the table built at tile m. This is E / pi, the unit a bake's texel has, so one shader term
 * serves lightmap and probe. dst_rgba: count * m * m * 4 floats, probe major, then j = jy * m + jx; w = 1 for an enabled probe, and
 * a disabled probe's texels are all zeros. In float32, one wave per output texel with the lanes splitting t as above:
 *   c = fma(n.z, d.z, fma(n.y, d.y, n.x * d.x));  c = c > 0 ? c : 0;  wgt = c * dw_t;  acc = acc + (wgt * L)       nothing else fused
 * then the same butterfly, and lane 0 writes acc * 0.318309886f. Synchronises. PTMI_E_INVALID: no probes, a bad m, a wrong n_floats.
 *
 * ptmi_debug_probe_rays: the first ray of texel (xs[i], ys[i]) at frames[i], as ptmi_debug_bake_rays returns a bake's; zeros for a
 * texel of a disabled probe or of a tile past count; a texel outside the atlas is PTMI_E_INVALID.
 * The ABI version stays 4: new calls only. */
typedef struct ptmi_probe_params { uint32_t first_frame; uint32_t _reserved[3]; } ptmi_probe_params;
struct ptmi_probe_status { uint32_t present, tile, count, enabled, texels; };
int ptmi_upload_probes(ptmi_ctx *ctx, const ptmi_probe *probes, uint32_t count, uint32_t tile);
int ptmi_dispatch_probes(ptmi_ctx *ctx, const ptmi_probe_params *params, uint32_t n_frames);
int ptmi_probe_status(ptmi_ctx *ctx, struct ptmi_probe_status *out);
int ptmi_probe_sh(ptmi_ctx *ctx, float *dst, size_t n_floats);
int ptmi_probe_irradiance(ptmi_ctx *ctx, uint32_t m, float *dst_rgba, size_t n_floats);
int ptmi_debug_probe_rays(ptmi_ctx *ctx, const ptmi_probe_params *params, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                          const uint32_t *frames, float *o3, float *d3, uint32_t *rng);
int ptmi_debug_probe_tables(uint32_t tile, float *dir_dw4, float *basis9);

/* ---- probe visibility: first-hit depth moments and Chebyshev tiles -----------------------------
 * A probe lattice leaks light through walls unless every probe also knows how far it sees. While the switch below is on, a probe
 * dispatch records per radiance texel the mean distance, the mean squared distance and the hit fraction of the texel's first rays
 * (the DEPTH PLANE), and ptmi_probe_visibility filters each probe's depth tile into a small octahedral tile a shader tests with
 * Chebyshev's inequality (INTEGRATION.md §1.21 has the recipe).
 *
 * ptmi_set_probe_depth: params->max_distance must be finite and > 0 and the reserved words 0, else PTMI_E_INVALID with the previous
 * state left in place (the switch, max_distance and the plane's contents). params NULL turns the switch off. While it is on the
 * context owns one more frame plane, a float4 per texel of the frame: made with the frame, zeroed when made, following ptmi_resize
 * exactly as the moments plane does (a resize gives a fresh zeroed plane); turning the switch on while it is on keeps the plane's
 * contents and takes the new max_distance. With the switch off the plane does not exist: ptmi_read_probe_depth,
 * ptmi_write_probe_depth and ptmi_probe_visibility return PTMI_E_STATE (so they do before the first ptmi_resize), and
 * ptmi_probe_depth_device_ptr NULL. Synchronises. ptmi_get_probe_depth: *on, and in *out (may be NULL) the params while on.
 * ptmi_read_probe_depth / ptmi_write_probe_depth: the whole plane, width * height * 4 floats (else PTMI_E_INVALID); both synchronise.
 * Writing restores a plane cached elsewhere.
 *
 * With the switch on ptmi_dispatch_probes keeps the first-hit record of every path's first ray - (albedo, t) and (normal,
 * bits(triangle)), 32 bytes a path, the record the first-hit planes of ptmi_set_aovs are folded from, written by the same kernel
 * instantiation - and after the radiance fold of a batch folds it into the depth plane. Per listed texel, for the batch's frames in
 * ascending order, in float32, each operation rounded once and none fused except inside mix:
 *   hit = bits(rec[2 li + 1].w) != 0xFFFFFFFF                               li = k * listed + j: frame first_frame + k of entry j
 *   d   = hit ? min(rec[2 li].w, max_distance) : max_distance
 *   x   = (d, d * d, hit ? 1 : 0)
 *   frame f = 0: acc = x;  f > 0: t = 1 / (float)(f + 1), acc = mix(acc, x, t) = fma(x, t, acc * (1 - t))   the radiance's running mean
 *   plane[texel] = (acc[0], acc[1], acc[2], 0)
 * first_frame = 0 overwrites; n frames in one call equal n calls of one; texels of disabled probes and of tiles past count are neither
 * read nor written. A miss counts as max_distance: for a probe nothing closer than the clamp is as good as nothing at all.
 * WHAT DEPTH MEANS is what the record holds. The alpha resolve loops run before shade, so the depth is that of the first surface
 * that is PRESENT: a ray through the hole of a cutout, or through a blended surface that is absent for this sample, records what
 * lies behind. Under a medium it is the distance to the surface behind the fog: a scatter event on the first ray ends the segment
 * early but does not shorten the record, which is the surface hit the ray had been given all the same. Fog changes a probe's
 * radiance, not what it can see.
 * The radiance, the moments plane and the statistics of a probe dispatch keep their bits with the switch on; ptmi_dispatch,
 * ptmi_dispatch_adaptive and ptmi_dispatch_bake keep their launches and their bits whatever the switch says, and get no record array
 * on its account. A probe dispatch with the switch on counts the record array in its automatic batch size. ptmi_dispatch_probes
 * with a first-hit plane on (ptmi_set_aovs) stays refused.
 *
 * ptmi_probe_visibility: per probe a side x side tile, side = m + 2 * border, m a power of two in 2 ... 16 with m <= N (the rule of
 * ptmi_probe_irradiance), sharpness_log2 = s in 0 ... 6, border 0 or 1. Interior texel j = (jx, jy), stored at (jx + border,
 * jy + border), is the depth tile D of the probe filtered by a power-cosine lobe about n_j, the float32 direction d_j of the table
 * built at tile m:
 *   v_j = sum_t w_jt * D[t].xyz / sum_t w_jt,   w_jt = max(0, dot(n_j, d_t))^(2^s) * dw_t,   written as (v_j.x, v_j.y, v_j.z, 1)
 * The exponent is a power of two so that the lobe is s squarings - the same bits on every machine and in numpy, where powf has
 * none to offer; s = 6 is cos^64, next to DDGI's cos^50. In float32, one workgroup per probe and one wave per output texel, lane l
 * from +0 over tile texels t = l, l + 64, ... in ascending order:
 *   c = fma(n.z, d.z, fma(n.y, d.y, n.x * d.x));  c = c > 0 ? c : 0              as ptmi_probe_irradiance
 *   p = c;  s times: p = p * p;  wgt = p * dw_t
 *   a0 = a0 + wgt * D[t].x;  a1 = a1 + wgt * D[t].y;  a2 = a2 + wgt * D[t].z;  a3 = a3 + wgt     rounded product, rounded sum
 * then the butterfly of ptmi_probe_sh over the four sums, and lane 0 writes (a0 / a3, a1 / a3, a2 / a3, 1), IEEE divisions. a3 is
 * positive because m <= N: both tables are texel centres of the same map and N / m is a whole number, so n_j's point of the square
 * is the centre of one of the tile's texels (N / m odd) or the corner four of them share (even), and the nearest of those has a
 * cosine to n_j above 0.5 (the worst pair, N = 4 with m = 2, has 0.89). Its weight is then above 2^-64 * dw_t with dw_t above 1e-4
 * at N = 64, a normal float32, and adding non-negative terms to it never takes it away. A disabled probe's tile is all zeros, border
 * included.
 * border = 1 surrounds the m x m interior with the texels a bilinear tap finds across the edge of the octahedral square, copies
 * written by the same kernel after the interior. With e = m - 1, in interior coordinates:
 *   (-1, y) <- (0, e - y)     (m, y) <- (e, e - y)     (x, -1) <- (e - x, 0)     (x, m) <- (e - x, e)
 *   corners (-1, -1) <- (e, e)   (m, -1) <- (0, e)   (-1, m) <- (e, 0)   (m, m) <- (0, 0)
 * dst_rgba: count * side * side * 4 floats, probe major, rows from the bottom. Reads the depth plane in place; synchronises.
 * PTMI_E_STATE: the switch is off. PTMI_E_INVALID: params NULL, no probes in place, a bad m, s or border, a non-zero reserved word,
 * n_floats wrong. A refusal writes nothing. There are no ptmi_multi_* counterparts, because probes have none.
 * The ABI version stays 4: new calls only. */
typedef struct ptmi_probe_depth_params { float max_distance; uint32_t _reserved[3]; } ptmi_probe_depth_params;
typedef struct ptmi_probe_visibility_params { uint32_t m, sharpness_log2, border, _reserved; } ptmi_probe_visibility_params;
int ptmi_set_probe_depth(ptmi_ctx *ctx, const ptmi_probe_depth_params *params);
int ptmi_get_probe_depth(ptmi_ctx *ctx, uint32_t *on, ptmi_probe_depth_params *out);
int ptmi_read_probe_depth(ptmi_ctx *ctx, float *dst_rgba, size_t n_floats);
int ptmi_write_probe_depth(ptmi_ctx *ctx, const float *src_rgba, size_t n_floats);
void *ptmi_probe_depth_device_ptr(ptmi_ctx *ctx);
int ptmi_probe_visibility(ptmi_ctx *ctx, const ptmi_probe_visibility_params *params, float *dst_rgba, size_t n_floats);
/* Back-pressure for a caller that enqueues dispatches from a loop without reading results — a preview loop; the reference paces
 * itself on requestAnimationFrame (renderer.ts:456-473). Blocks until at most max_in_flight of this context's dispatches have
 * not yet finished on the device and reports how many still are (in_flight may be NULL). max_in_flight = 0xFFFFFFFF only polls.
 * Independently of this call the library never lets more than 256 dispatches queue up: ptmi_dispatch then waits for the oldest. */
int ptmi_throttle(ptmi_ctx *ctx, uint32_t max_in_flight, uint32_t *in_flight);

/* ---- output buffer (binding 0) ------------------------------------------ */
/* width*height float4 (xyz = running mean, w = 0), index y*width+x. Synchronises. */
int ptmi_read_output(ptmi_ctx *ctx, float *dst_rgba, size_t n_floats);
int ptmi_write_output(ptmi_ctx *ctx, const float *src_rgba, size_t n_floats);
/* Device-side access for zero-copy consumers (blit, RCCL gather): the buffer's
 * device address, or a caller-owned device buffer of >= width*height*16 bytes to
 * render into instead (like binding a GPUBuffer the caller created). */
void *ptmi_output_device_ptr(ptmi_ctx *ctx);
int ptmi_bind_output_device(ptmi_ctx *ctx, void *device_ptr, size_t bytes);
/* Order this context's work on a caller-owned hipStream_t (NULL = the context's own). */
int ptmi_set_stream(ptmi_ctx *ctx, void *hip_stream);

/* ---- first-hit planes ("AOVs": the guides a denoiser takes, depth for compositing, ids for picking) -------------------
 * Off by default. While a plane is on, every dispatch also folds, per pixel and in the same frame order as the output buffer, what
 * each frame's camera ray found at its first hit. Each plane is width*height entries, index y*width+x, like the output buffer:
 *   PTMI_AOV_ALBEDO  float4: xyz = the hit's albedo (base colour x albedo-map texel, what the BSDF sees), w = coverage (1 hit, 0 miss)
 *   PTMI_AOV_NORMAL  float4: xyz = the hit's world-space shading normal (after the normal map; not flipped toward the viewer),
 *                            w = t, the distance from the camera ray's origin (on the lens with depth of field), 0 on a miss
 *   PTMI_AOV_ID      uint32 x 2: the triangle (index as uploaded) and its material_index, of the LAST frame folded in;
 *                            0xFFFFFFFF twice on a miss. Not averaged.
 * ALBEDO and NORMAL follow the output buffer's fold exactly, without its clamp: frame 0 overwrites, frame f > 0 mixes with weight
 * 1 / (f + 1). A mean of unit normals is not of unit length: normalise it before use. A plane turned on after accumulation has
 * started (frame_index > 0) mixes with zeros until the next frame-0 dispatch, as the output buffer would. The radiance is the same
 * bits with the planes on or off. Only the rows this context renders (tile_y0 / tile_y1, tile_parts) are written; the others keep
 * their contents. Over a ptmi_multi, ptmi_multi_set_aovs turns the planes on on every device, each holds its own strips, and
 * ptmi_multi_gather_planes / ptmi_multi_read_aov assemble them on device 0.
 * Cost while on: 32 bytes of device memory per path of a batch (the automatic batch size counts it) and one more pass per batch. */
enum { PTMI_AOV_ALBEDO = 1u, PTMI_AOV_NORMAL = 2u, PTMI_AOV_ID = 4u };
/* mask: any combination of PTMI_AOV_* (0 = none, the default; other bits PTMI_E_INVALID). A plane turned on is allocated and
 * zero-filled, planes already on keep their contents, a plane turned off is freed. ptmi_resize re-allocates the enabled planes,
 * zero-filled. A failed call leaves the previous mask and planes in place. Synchronises. */
int ptmi_set_aovs(ptmi_ctx *ctx, uint32_t mask);
int ptmi_get_aovs(const ptmi_ctx *ctx, uint32_t *mask);
/* which: exactly one PTMI_AOV_* bit; n_bytes: width*height*16 (width*height*8 for PTMI_AOV_ID), else PTMI_E_INVALID. A plane that
 * is off (or before ptmi_resize) gives PTMI_E_STATE. Synchronises. */
int ptmi_read_aov(ptmi_ctx *ctx, uint32_t which, void *dst, size_t n_bytes);
/* the plane's device address for zero-copy consumers (a denoiser on the same device); NULL when that plane is off */
void *ptmi_aov_device_ptr(ptmi_ctx *ctx, uint32_t which);

/* ---- sample moments and the denoiser (an SVGF-style a-trous filter over the first-hit planes) -------------------------------
 * The sample-moments plane is off by default. While on, every dispatch also folds per pixel, in the output buffer's frame order and
 * with its fold rule (frame 0 overwrites, frame f > 0 mixes with weight 1 / (f + 1)), a float4:
 *   x = mean of l, y = mean of l^2, z = frames folded (frame + 1 of the last one), w = 0,
 * with l = 0.2126 r + 0.7152 g + 0.0722 b of exactly the clamped per-frame radiance the output buffer folds. The variance of the
 * mean is then max(0, y - x^2) / max(z, 1). The radiance keeps its bits with the plane on. Its life cycle is an AOV plane's: turning
 * it on allocates it zero-filled (a plane turned on after accumulation has started mixes with those zeros until the next frame-0
 * dispatch), ptmi_resize re-allocates it zero-filled, only the rows this context renders are written, a failed call keeps the
 * previous state. It is not a PTMI_AOV_* bit. Cost while on: one more pass per batch, no per-path memory. */
/* on: 0 or 1 (else PTMI_E_INVALID). Synchronises. */
int ptmi_set_moments(ptmi_ctx *ctx, uint32_t on);
int ptmi_get_moments(const ptmi_ctx *ctx, uint32_t *on);
/* n_floats: width*height*4, else PTMI_E_INVALID; the plane off (or before ptmi_resize): PTMI_E_STATE. Synchronises. */
int ptmi_read_moments(ptmi_ctx *ctx, float *dst, size_t n_floats);
/* The counterpart of ptmi_write_output for the plane: width*height*4 floats replace its contents, so that a checkpointed render or
 * bake that had the plane on can be resumed (write both, then go on from the next frame), and a filter can be given chosen variances.
 * The same sizes and errors as ptmi_read_moments. Synchronises. */
int ptmi_write_moments(ptmi_ctx *ctx, const float *src, size_t n_floats);
/* NULL while the plane is off */
void *ptmi_moments_device_ptr(ptmi_ctx *ctx);

/* ptmi_denoise filters the whole width x height output buffer with an edge-avoiding a-trous wavelet (Dammertz et al. 2010) whose
 * colour weight is scaled by the moments plane's variance (Schied et al. 2017, spatial part only), guided by the NORMAL plane
 * (normal and depth) and, when demodulating, the ALBEDO plane. It needs the NORMAL and the moments planes on (else PTMI_E_STATE)
 * and writes a context-owned width*height float4 plane, (rgb, 0) in the output buffer's layout; the output buffer and the other
 * planes are not written. It is not on the parity path: its contract is a tolerance against tests/denoise_ref.py. The variance
 * estimate shrinks as frames accumulate, so the filter backs off as the image converges. Over a ptmi_multi, ptmi_multi_denoise first
 * gathers the planes the filter reads onto device 0 and then runs it there on the whole frame (a context's own ptmi_denoise sees only
 * the rows it holds). */
typedef struct ptmi_denoise_params {
    uint32_t iterations;   /* a-trous passes, step 2^i pixels for pass i; 1..10; 0 -> 5 */
    uint32_t demodulate;   /* 0: on iff the ALBEDO plane is on; 1: never; 2: always (ALBEDO off -> PTMI_E_STATE) */
    float    phi_color;    /* luminance edge-stopping, in standard deviations; 0 -> 4 */
    float    phi_normal;   /* exponent on the normals' dot product; 0 -> 128 */
    float    phi_depth;    /* depth edge-stopping, in units of the local depth gradient; 0 -> 1 */
    uint32_t reserved[3];  /* must be 0 */
} ptmi_denoise_params;
/* params NULL: the defaults. A negative or non-finite phi, iterations > 10, an unknown demodulate, a non-zero reserved word or (with
 * dst_rgba) n_floats != width*height*4: PTMI_E_INVALID; before ptmi_resize: PTMI_E_STATE. dst_rgba NULL: asynchronous on the
 * context's stream (read the result through ptmi_denoised_device_ptr after ptmi_synchronize); else synchronises and copies the
 * width*height float4 result out. */
int ptmi_denoise(ptmi_ctx *ctx, const ptmi_denoise_params *params, float *dst_rgba, size_t n_floats);
/* the denoised plane's device address; NULL before the first ptmi_denoise since the last ptmi_resize */
void *ptmi_denoised_device_ptr(ptmi_ctx *ctx);
/* ptmi_blit's contract, on the denoised plane (PTMI_E_STATE before the first ptmi_denoise since the last ptmi_resize) */
int ptmi_blit_denoised(ptmi_ctx *ctx, float *dst_rgba_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes);

/* ---- adaptive sampling: further frames only for the pixels that have not converged ---------------------------------------------
 * ptmi_dispatch traces every pixel of the context's rows for every frame. ptmi_dispatch_adaptive lets every pixel be at its own
 * frame index: the per-pixel sample count is the moments plane's z (ptmi_set_moments(1) is required, else PTMI_E_STATE), and since
 * the RNG is seeded per (x, y, frame) and every fold is per pixel in frame order, a pixel that has received its frames 0 .. n-1
 * holds, bit for bit, what an n-frame ptmi_dispatch leaves at that pixel - in the output buffer, the first-hit planes and the moments
 * plane - whatever its neighbours received.
 * One call = `rounds` rounds, each entirely on the device. A round
 *   1. selects. With (m1, m2, n) = moments.xyz of a pixel, all in float32, evaluated left to right, no FMA, no square root, no
 *      transcendental, and max(a, b) = (a < b ? b : a):
 *        var = max(m2 - m1 * m1, 0), e = threshold * max(m1, floor), bound = e * e * n;
 *      a pixel is NOISY iff n < min_frames, or n < max_frames and NOT var <= bound (so a NaN moment stays noisy until max_frames).
 *      With neighbourhood = 1 a pixel is ACTIVE iff its own n < max_frames and it or one of its 8 neighbours inside the context's
 *      rows and the image is noisy; with neighbourhood = 0 active = noisy;
 *   2. lists the active pixels in ascending order (the segment statistics are not touched);
 *   3. traces, for every active pixel, its frames n .. n + step - 1 through the bounce loop of ptmi_dispatch (`step` is split into
 *      sub-batches by options.frames_per_batch or by memory like any dispatch; the list is fixed before the first sub-batch), and
 *   4. folds them, frames ascending, with the arithmetic of ptmi_dispatch's folds; n grows by step.
 * A pixel is selected or not as a whole, so its count may pass max_frames by less than step. The counts are exact in float up to 2^24.
 * Deciding from the samples being averaged biases the mean: min_frames and neighbourhood exist to bound that.
 * camera.frame_index == 0 restarts: the first round treats every count of the context's rows as 0, so frame 0 overwrites; any other
 * value continues from the plane and is otherwise unused. ptmi_dispatch followed by ptmi_dispatch_adaptive is defined (the uniform
 * fold keeps z true). A plain ptmi_dispatch after adaptive rounds folds every pixel with the camera's frame index as it always has,
 * whatever the pixels' own counts: that is the caller's business. Asynchronous, like ptmi_dispatch.
 * ptmi_stats after one call: paths grows by the samples actually traced (counted on the device, read where ptmi_get_stats
 * synchronises), frames by nothing, dispatches by one. ptmi_multi_dispatch_adaptive is the call over several devices: there the
 * neighbours of rule 1 are those inside the image, whichever device holds their row. */
typedef struct ptmi_adaptive_params {
    float    threshold;      /* relative standard error of the pixel's mean luminance; > 0 */
    float    floor;          /* luminance under which the error is taken relative to `floor`; 0 -> 1 (an absolute error below luminance 1) */
    uint32_t min_frames;     /* every pixel gets at least this many; 0 -> 16 */
    uint32_t max_frames;     /* and at most this many (plus less than step); 0 -> 4096; <= 2^24 */
    uint32_t step;           /* frames an active pixel receives per round; 0 -> 16 */
    uint32_t neighbourhood;  /* 0 / 1 */
    uint32_t reserved[2];    /* must be 0 */
} ptmi_adaptive_params;      /* 32 bytes */
/* a struct tag only (no typedef): the call below has the same name, so write `struct ptmi_adaptive_status` */
struct ptmi_adaptive_status {
    uint64_t active;         /* pixels the last round's list held (0 before the first round since ptmi_resize or ptmi_set_moments) */
    uint64_t samples;        /* sum of the per-pixel counts over the context's rows */
    uint32_t min_count, max_count;   /* smallest / largest count in the context's rows */
    uint32_t rounds;         /* rounds since the last restart, ptmi_resize or change of ptmi_set_moments */
    uint32_t reserved;
};                           /* 32 bytes */
/* PTMI_E_STATE: no scene, no output buffer, or the moments plane off. PTMI_E_INVALID: params or camera NULL, a camera of another
 * size, threshold not > 0 (NaN included), floor negative or not finite, a non-zero reserved word, neighbourhood > 1,
 * min_frames > max_frames (after the defaults), max_frames > 2^24, step > 2^16. rounds = 0 does nothing. */
int ptmi_dispatch_adaptive(ptmi_ctx *ctx, const ptmi_camera *camera, const ptmi_adaptive_params *params, uint32_t rounds);
/* Synchronises. PTMI_E_STATE while the moments plane is off or before ptmi_resize. */
int ptmi_adaptive_status(ptmi_ctx *ctx, struct ptmi_adaptive_status *out);

/* ---- reprojection: carry the accumulated samples across a camera move (the temporal half of Schied et al. 2017) -------------------
 * A frame-0 dispatch after a camera move throws away every sample. ptmi_reproject instead rewrites the output buffer, the moments
 * plane (per-pixel counts included) and the first-hit planes for the camera `to` from what they hold for the camera `from`, so that
 * ptmi_dispatch_adaptive(to, frame_index != 0) continues every pixel from the count it is left with: a pixel that shows a surface
 * the old view had seen keeps (a bilinear blend of) its history, a disoccluded pixel is at count 0 and is overwritten by its frame 0.
 * It needs the NORMAL plane (its w is the mean first-hit distance) and the moments plane (else PTMI_E_STATE); ALBEDO and ID are
 * carried while on. A post-process like the denoiser: not on the parity path, nothing else changes behaviour unless it is called.
 * The pass, over the pixels of the context's rows (tile_y0 / tile_y1, tile_parts); rows of other contexts are neither read nor written:
 *   1. snapshot: device-to-device copies of the output buffer (the caller's, when one is bound), moments, NORMAL and, while on,
 *      ALBEDO and ID into context-owned history planes (made by the first call since ptmi_resize, all or nothing). The live planes
 *      are then rewritten in place.
 *   2. the centre ray of every pixel under `to`: the camera ray of ptmi_dispatch with the jitter replaced by (0.5, 0.5), no lens
 *      sample and no RNG (aperture is ignored): origin = to.position, or the pixel's point of the camera plane of an orthographic
 *      `to` (ptmi_set_projections) (ptmi_debug_center_rays returns them).
 *   3. their closest hits (t, tri), by the traversal kernel of ptmi_dispatch, as ptmi_debug_intersect runs it.
 *   4. per pixel, all in float32, left to right, no FMA, with the correctly rounded / and sqrt, and dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z:
 *      MISS (tri == 0xFFFFFFFF): every live plane of the pixel becomes zero, the ids 0xFFFFFFFF twice, the count 0. Else
 *        P = o + t d (per component: multiply, then add), v = P - from.position, zf = dot(v, from.forward), dist = sqrt(dot(v, v)),
 *        th = tan(from.fov * 0.5f) (the kernels' tan: ptmi_debug_math op 11);
 *        !(zf > 0): DISOCCLUDED. Else sx = dot(v, from.right) / (zf * th * from.aspect), sy = dot(v, from.up) / (zf * th) (from's basis
 *        is taken as orthonormal), fx = (sx + 1) * 0.5f * W - 0.5f, fy = (sy + 1) * 0.5f * H - 0.5f; fx or fy not finite: DISOCCLUDED.
 *        x0 = floor(fx), ax = fx - x0, y0 = floor(fy), ay = fy - y0. The four taps (x0 + i, y0 + j) are visited in the order
 *        (0,0), (1,0), (0,1), (1,1) with weight w = (i ? ax : 1 - ax) * (j ? ay : 1 - ay). A tap q is VALID iff it lies inside the
 *        image and in a row of this context, its snapshot count n_q = moments.z >= 1, its snapshot depth t_q = normal.w > 0,
 *        |t_q - dist| <= depth_tolerance * dist, every snapshot float read for it (output xyz, moments xyz, normal xyzw, albedo xyzw
 *        while on) is finite, and - when ids are compared - its snapshot material id equals triangles[tri].material_index.
 *        sw = the sum of the valid weights in tap order. No valid tap, or !(sw > 0): DISOCCLUDED: the planes are zeroed as for a
 *        miss, ids = (tri, material), count 0. Else CARRIED: output xyz, moments xy, albedo xyzw and normal xyz each become
 *        (sum over the valid taps, in tap order, of w * value) / sw; normal.w = t, ids = (tri, material), output.w = moments.w = 0,
 *        count = min(min over the valid taps of n_q, max_history) with min(a, b) = a < b ? a : b (an integer, as its inputs are).
 * After the call the planes are what a render with per-pixel counts leaves. Caveat: with from == to and max_history below a pixel's
 * count, the pixel traces seeds again that it has already used (frames count .. are those of its earlier samples): reprojection is
 * for a camera that moved. There is no ptmi_multi counterpart: each context of a ptmi_multi holds only its own strips, a reprojected
 * sample would have to come from another device's, and the planes gather of ptmi_multi assembles frames on device 0 only. */
typedef struct ptmi_reproject_params {
    uint32_t max_history;      /* a carried count is capped here; 0 -> 32; <= 2^24 */
    float    depth_tolerance;  /* relative: a tap is rejected when |t_tap - dist| > depth_tolerance * dist; 0 -> 0.02 */
    uint32_t match_ids;        /* 0: compare material ids iff the ID plane is on; 1: never; 2: always (ID off -> PTMI_E_STATE) */
    uint32_t reserved[5];      /* must be 0 */
} ptmi_reproject_params;       /* 32 bytes */
/* of the last ptmi_reproject, over the context's rows: carried + disoccluded + missed = their pixels; samples = the sum of the new
 * counts (all zero before the first call). A struct tag only, like ptmi_adaptive_status */
struct ptmi_reproject_status { uint64_t carried, disoccluded, missed, samples; };   /* 32 bytes */
/* Asynchronous on the context's stream. params NULL: the defaults. PTMI_E_STATE: no scene, no output buffer, the NORMAL or the
 * moments plane off, match_ids = 2 with the ID plane off. PTMI_E_INVALID: from or to NULL, a camera of another size than the
 * context's, depth_tolerance negative or not finite, max_history > 2^24, match_ids > 2, a non-zero reserved word; with
 * ptmi_set_projections on, a camera whose projection words are rejected, or an equirectangular camera on either side (its inverse
 * needs atan2 / asin, outside the arithmetic contract: left for later). A failed call writes nothing. */
int ptmi_reproject(ptmi_ctx *ctx, const ptmi_camera *from, const ptmi_camera *to, const ptmi_reproject_params *params);
int ptmi_reproject_status(ptmi_ctx *ctx, struct ptmi_reproject_status *out);    /* synchronises */

/* ---- motion: carry the samples across a geometry edit too ------------------------------------
 * ptmi_reproject as stated above projects the new hit point into the old camera, which is the wrong place in the old image for a
 * surface that ptmi_update_triangles has moved since the history was rendered. With motion on, the context keeps the vertex
 * positions the history was rendered with (the previous positions: v0, v1, v2 as three float4 with w = 0, 48 bytes per uploaded
 * triangle) and the range of triangles updated since (the dirty range), ptmi_reproject projects a hit on a moved triangle from where
 * its point was, and the per-pixel screen motion is written to a plane: the guide temporal denoisers and upscalers ask for beside
 * albedo, normal and depth. A post-process, off by default: while off every call issues the launches and gives the bits it gave
 * before, and no buffer is allocated.
 *   ptmi_set_motion(1) allocates the previous positions (filled from the triangles now on the device; with the other scene buffers)
 *     and the motion plane (width*height float4, zero-filled; re-made zero-filled by ptmi_resize like an AOV plane), clears the dirty
 *     range and sets epochs to 0. Allowed before an upload or a resize: the buffers then appear with the scene and the size. A failed
 *     call leaves the previous state in place. ptmi_set_motion(0) frees both.
 *   ptmi_upload_scene while on re-makes the previous positions from the new scene, clears the dirty range, epochs = 0.
 *   ptmi_update_triangles while on does its work unchanged and widens the dirty range to the union with [first, first + count). The
 *     previous positions are not touched: several updates between two commits accumulate against the same epoch.
 *   ptmi_motion_commit copies the current v0, v1, v2 over the dirty range into the previous positions (one kernel), clears the range
 *     and increments epochs. A host that restarts accumulation with a frame-0 dispatch after an edit calls it: the history is then
 *     rendered with the current geometry. Asynchronous on the context's stream. PTMI_E_STATE while off.
 *   ptmi_reproject while on runs its steps 1 to 3, recomputes (u, v) of the centre rays' resolved hits as ptmi_debug_intersect
 *     reports them, runs step 4 with the moved rule, writes the motion plane for every pixel of the context's rows, and commits at
 *     its end as ptmi_motion_commit does. A failed call writes nothing and commits nothing.
 * The moved rule. A hit on triangle tri is MOVED iff tri lies in the dirty range AND at least one of the nine previous-position
 * floats of tri differs in its bits from the current v0, v1, v2. A MOVED hit computes, with (u, v) as ptmi_debug_intersect reports
 * them for that ray, in float32, left to right, no FMA, per component k:
 *     e1_k = v1p_k - v0p_k,  e2_k = v2p_k - v0p_k,  Pprev_k = (v0p_k + u * e1_k) + v * e2_k      (v0p, v1p, v2p: the previous positions)
 * and v = Pprev - from.position replaces v = P - from.position in step 4. Everything after it is unchanged: zf, dist, sx, sy, fx, fy,
 * the four taps, the depth and id tests, the blends, the counts, and normal.w = t of the NEW hit. A hit that is not MOVED uses
 * P = o + t d exactly as before: motion on with no edit gives the bits of motion off, pixel for pixel, and triangles outside the dirty
 * range cost nothing extra (the range bounds are kernel arguments, so the test is uniform for most waves).
 * The motion plane at a pixel (px, py) of the context's rows (integer coordinates as floats, row 0 at the bottom like the output
 * buffer), from the fx, fy, dist its rule computed: x = fx - px, y = fy - py: where the surface was in `from`, in pixels, relative
 * to the pixel; z = dist; w = 0 / 1 / 2 for CARRIED / DISOCCLUDED / MISSED. x = y = z = 0 on a miss, where !(zf > 0), or where fx or
 * fy is not finite. Rows of other contexts are not written.
 * Limits. The carried radiance and normals are the old ones: moved lighting, shadows cast by the moved object and rotated normals
 * are stale until new frames dilute them; max_history is the bound, as in Schied et al. 2017. Topology changes are out of scope
 * (ptmi_update_triangles never changes it; an upload restarts). With an alpha cutoff table active, (u, v) are those of the resolved
 * hit on the caller's centre ray. There is no ptmi_multi counterpart, because reprojection has none. */
int ptmi_set_motion(ptmi_ctx *ctx, uint32_t on);          /* 0 / 1, else PTMI_E_INVALID; synchronises */
int ptmi_get_motion(const ptmi_ctx *ctx, uint32_t *on);
int ptmi_motion_commit(ptmi_ctx *ctx);                    /* previous positions := current, over the dirty range */
struct ptmi_motion_status {              /* 32 bytes; a struct tag only, like ptmi_reproject_status */
    uint32_t on, epochs;                 /* commits since the last upload or ptmi_set_motion(1) */
    uint32_t dirty_first, dirty_count;   /* union of the ranges updated since the last commit (0, 0: none) */
    uint64_t moved, moved_carried;       /* pixels of the last ptmi_reproject that took the moved rule / of those, CARRIED */
};
int ptmi_motion_status(ptmi_ctx *ctx, struct ptmi_motion_status *out);   /* synchronises */
/* n_floats: width*height*4, else PTMI_E_INVALID; motion off (or before ptmi_resize): PTMI_E_STATE. Synchronises. */
int ptmi_read_motion(ptmi_ctx *ctx, float *dst, size_t n_floats);
void *ptmi_motion_device_ptr(ptmi_ctx *ctx);                             /* NULL while off */
/* per-stage: the previous positions of triangles [first, first+count): 9 floats each (v0, v1, v2). PTMI_E_STATE while off or
 * without a scene; a range beyond the uploaded count: PTMI_E_INVALID. Synchronises. */
int ptmi_debug_motion_prev(ptmi_ctx *ctx, uint32_t first, uint32_t count, float *v9);

/* ---- environment lighting: an HDR sky behind every miss, importance-sampled ------------------
 * Without an environment a ray that leaves the scene adds throughput * 0 (pt.wgsl:646-648) and nothing changes: every result keeps
 * its bits. With one, a ray of bounce b that misses adds throughput * (W_b * Le(d)) where an emissive hit's addition goes, the camera
 * ray included (W_0 = 1); the first-hit planes of a miss stay zeros / 0xFFFFFFFF.
 * The map is equirectangular, width x height RGBA texels in either atlas format (alpha is ignored), row 0 at the +Y pole, texel (0,0)
 * first. LOOKUP of a unit direction d: phi = atan2(d.z, d.x) - rotation, u = phi / 2pi + 0.5 wrapped into [0, 1),
 * v = acos(clamp(d.y, -1, 1)) / pi, texel (min(floor(u W), W - 1), min(floor(v H), H - 1)), nearest, unfiltered;
 * Le = texel.rgb * intensity, one float32 multiply per channel. atan2 and acos are the device's own: which texel a direction within
 * rounding of a texel border reads is outside the bit-exact arithmetic contract, like ptmi_blit.
 * DISTRIBUTION, built on the host at upload in double precision: w_t = lum(rgb_t) * (cos(theta_top) - cos(theta_bottom)) of the
 * texel's row, lum = 0.2126 r + 0.7152 g + 0.0722 b; P_t = w_t / sum(w); a Vose alias table (prob: float, alias: uint32) over the
 * N = W * H texels; c_t = float(P_t * N / (2 pi^2)) beside the texel's rgb. pdf(d) = c_t / max(sqrt(max(0, 1 - d.y^2)), 1e-6) is the
 * solid-angle density of "texel t with probability P_t, then uniform in (u, v) inside it". A map whose sum(w) is 0 (all black) is
 * looked up but never sampled.
 * SAMPLING (next-event estimation, do_mis = 1): while a map is in place and sampled it is light number n_lights: sampleLight draws
 * its index from 0 .. n_lights and every light's pdf takes 1 / (n_lights + 1). Chosen, it draws r1 .. r4: k = min(floor(r1 N), N - 1),
 * t = r2 < prob[k] ? k : alias[k], u = (t mod W + r3) / W, v = (t / W + r4) / H, theta = v pi, phi = (u - 0.5) 2pi + rotation,
 * d = (sin theta cos phi, cos theta, sin theta sin phi) with the kernels' sin / cos (ptmi_debug_math ops 5, 6), density
 * c_t / max(sin theta, 1e-6), radiance the texel's: a directional shadow record (any hit occludes), weighted like every light sample.
 * The bounce ray of a vertex that ran next-event estimation with a sampled map carries W = powerHeuristic(1, bsdf pdf, 1,
 * pdf(direction) / (n_lights + 1)) for the bounce that may miss; every other ray carries 1 (do_mis = 0, a transmissive hit, a back
 * face, sample = 1). */
typedef struct ptmi_environment {
    float    intensity;   /* radiance scale; 0 -> 1; negative / non-finite: PTMI_E_INVALID */
    float    rotation;    /* radians about +Y, added to the azimuth; must be finite (kept as its remainder by 2 pi, in [-pi, pi]) */
    uint32_t sample;      /* 0: next-event samples include the sky (default); 1: lookup only (misses see it, NEE never picks it) */
    uint32_t reserved[5]; /* must be 0 */
} ptmi_environment;       /* 32 bytes */
/* texels NULL or width / height 0: removes the environment. params NULL: the defaults. PTMI_E_INVALID: an unknown format, a size that
 * does not fit (more than 2^28 texels included), a texel whose r, g or b is negative or not finite, bad params. A call that fails
 * leaves the current environment in place. Synchronises. */
int ptmi_upload_environment(ptmi_ctx *ctx, const void *texels, uint32_t width, uint32_t height, int format,
                            const ptmi_environment *params);
/* intensity / rotation / sample of the map in place, without a re-upload. PTMI_E_STATE: none is in place. Synchronises. */
int ptmi_set_environment(ptmi_ctx *ctx, const ptmi_environment *params);
/* width = height = 0: none in place. sampled: 1 iff next-event estimation picks it (sample = 0 and sum(w) > 0). A struct tag only. */
struct ptmi_environment_status { uint32_t width, height, sampled, reserved; double weight_sum; };   /* 24 bytes */
int ptmi_environment_status(ptmi_ctx *ctx, struct ptmi_environment_status *out);

/* ---- a homogeneous participating medium: scattering fog inside a box --------------------------
 * Without a medium light travels through vacuum and nothing changes: the kernels launched are the ones of before and every result
 * keeps its bits. With one, there is ONE homogeneous medium per context inside an axis-aligned box: a scalar (grey) extinction
 * sigma_t, which keeps distance sampling exact for all three channels, a single-scattering albedo per channel, and the
 * Henyey-Greenstein phase function of asymmetry g. Per PATH SEGMENT, in the shade kernel, with the ray (o, d) of the path state (d is
 * the unit direction it holds) and t_hit the hit distance, or +inf on a miss:
 * 1. INTERVAL. Per axis k: inv = 1 / d_k, t1 = (min_k - o_k) inv, t2 = (max_k - o_k) inv; near = max_k min(t1, t2),
 *    far = min_k max(t1, t2), a = max(near, 0), b = min(far, t_hit), with fmin / fmax semantics (a NaN from 0 * inf drops out). If NOT
 *    b > a the segment is handled exactly as without a medium and draws nothing extra. (A box with min == max on an axis has no such
 *    segment, but for a ray that lies in that plane with a direction component of exactly 0 across it: both of its NaNs drop out.)
 *    A ray whose t1 and t2 are NaN on all three axes, the NaN origin or direction of a degenerate path, has no interval: b = a.
 * 2. FREE FLIGHT. One draw r, before any other draw of the segment: s = -ln(1 - r) / sigma_t. The path SCATTERS iff a + s < b, at
 *    x = o + (a + s) d; otherwise the surface hit or the miss is handled as without a medium, the throughput unchanged (distance
 *    sampling and the transmittance cancel).
 * 3. AT A SCATTER the throughput is multiplied by the albedo; all zero, the path ends. Otherwise next-event estimation runs when
 *    do_mis is on and there is a light or a sampled sky: sampleLight at x, with the phase value
 *    p = (1 - g^2) / (4 pi (1 + g^2 - 2 g cos)^1.5), cos = dot(d, wi), where evalBSDF's value and pdf stand (f = (p, p, p), pdf = p),
 *    the same powerHeuristic and `direct` arithmetic (the reference's pdf constants of punctual lights included), times Tr (below); the
 *    record is an ordinary shadow record from x, a zero contribution is counted and not recorded. The bounce direction takes two
 *    draws xi1, xi2: cos = 1 - 2 xi1 for |g| < 1e-3, else (1 + g^2 - ((1 - g^2) / (1 - g + 2 g xi1))^2) / (2 g), clamped to [-1, 1];
 *    sin = sqrt(max(0, 1 - cos^2)); phi = 2 pi xi2 with the kernels' sin / cos; the frame about d is Duff et al. 2017:
 *    sg = copysign(1, d.z), A = -1 / (sg + d.z), B = d.x d.y A, T = (1 + sg d.x^2 A, sg B, -sg d.x), U = (B, sg + d.y^2 A, -d.y); the
 *    direction is sin cos(phi) T + sin sin(phi) U + cos d, normalised. Its density is its phase value: the throughput takes no further
 *    factor. Roulette as at a surface; a scatter is one bounce and one segment. Under a sampled sky the bounce ray carries
 *    W = powerHeuristic(1, p, 1, pdf_env(direction) / (n_lights + 1)) where next-event estimation ran, else 1.
 * 4. TRANSMITTANCE of every next-event sample, those from surfaces too (the one change to the surface branch while a medium is in
 *    place): Tr(o, wi, dist) = exp(-sigma_t max(0, min(far, dist) - max(near, 0))) with near / far of the ray (o, wi), far alone for
 *    directional and sky samples; it multiplies the contribution before the "exactly zero" test.
 * 5. UNCHANGED: the additions of emissive hits and misses; the first-hit planes, which record the camera ray's SURFACE hit whether or
 *    not the path scattered in front of it (every plane has the same bits with and without a medium); the moments plane; the fold.
 * ln, exp and the free-flight comparison use the device's logf / expf: they are outside the bit-exact arithmetic contract, like the
 * sky lookup and ptmi_blit; the CPU oracle models the medium with the C library's (oracle/pt_oracle.h pto_extras). A ray that
 * starts at a scatter point outside the scene's bounds takes the own-leaf kernels' re-trace over the tree as uploaded: correct, and
 * slower. */
typedef struct ptmi_medium {
    float    sigma_t;                 /* extinction per unit length; finite, > 0 */
    float    albedo[3];               /* each in [0, 1] */
    float    g;                       /* |g| <= 0.99 */
    float    box_min[3], box_max[3];  /* finite, min <= max per axis; an axis with min == max makes a medium no ray traverses */
    uint32_t reserved[5];             /* must be 0 */
} ptmi_medium;                        /* 64 bytes */
/* medium NULL removes it. A bad field: PTMI_E_INVALID, and the medium in place stays. Takes effect at the next dispatch. Synchronises. */
int ptmi_set_medium(ptmi_ctx *ctx, const ptmi_medium *medium);
/* *present = 1 and *out = the medium as it was set, or *present = 0 and *out zeroed. Either pointer may be NULL. */
int ptmi_get_medium(const ptmi_ctx *ctx, ptmi_medium *out, uint32_t *present);

/* ---- a density grid for the medium: smoke, a cloud, a mist that thins with height -------------
 * nx * ny * nz float32 multipliers rho in [0, 1], stretched over the medium's box: the local extinction is sigma_t * rho(x), so the
 * medium's sigma_t is the majorant by construction. Albedo, g and the box stay those of ptmi_medium. Without a grid nothing changes: the
 * kernels launched and every result are those of the homogeneous medium.
 * LAYOUT: x fastest, cell (i, j, k) is entry (k * ny + j) * nx + i and covers box_min + (i .. i + 1) / nx * extent on x, likewise y, z.
 * LOOKUP at p, float32 in the order written, a plain '/', no fused step (under the arithmetic contract):
 *    u_k = (p_k - min_k) / (max_k - min_k) * n_k.  filter 0 (nearest): i_k = clamp(int(floor(u_k)), 0, n_k - 1).
 *    filter 1 (trilinear over cell centres): v_k = u_k - 0.5, i0 = floor(v_k), f_k = v_k - i0, taps i0 and i0 + 1 each clamped to
 *    [0, n_k - 1], interpolated along x, then y, then z, each as a * (1 - f) + b * f. A NaN coordinate reads index 0 on that axis.
 * DELTA TRACKING replaces the free-flight draw (step 2 above) on a segment with an interval (a, b), b > a:
 *    t = a;  repeat:  r = draw;  t += -ln(1 - r) / sigma_t;  if NOT t < b: no scatter, stop
 *                     rho = lookup(o + t d);  r' = draw (always);  if r' < rho: SCATTER at t, stop
 *    All tracking draws of a segment come before any other draw of it; the RNG state behind them is handed on as the state behind the
 *    single draw is. A scatter is handled as above (step 3), a segment without one keeps its throughput.
 * RATIO TRACKING replaces Tr (step 4) where Tr is evaluated (the sample's pdf > 0), with near / far / end as there:
 *    T = 1, t = max(near, 0);  repeat:  r = draw;  t += -ln(1 - r) / sigma_t;  stop if NOT t < end;  T *= 1 - lookup(o + t wi);
 *    stop if T == 0.  Its draws come after sampleLight's and before any later draw of the vertex. T multiplies the contribution before
 *    the "exactly zero" test.
 * TERMINATION: a grid is accepted only while sigma_t * |box diagonal| <= 256 (at most 256 expected tentative collisions a segment);
 * both loops stop after 65 536 iterations, a guard nothing should reach: a delta-tracking segment then ends its path, a ratio-tracking
 * sample gives T = 0. The tracking decisions are outside the bit-exact arithmetic contract, like the free-flight draw they replace. */
typedef struct ptmi_medium_grid {
    uint32_t filter;                  /* 0 nearest, 1 trilinear */
    uint32_t reserved[7];             /* must be 0 */
} ptmi_medium_grid;                   /* 32 bytes */
/* rho NULL or a zero dimension removes the grid: the medium is homogeneous again (without a medium: nothing to do, PTMI_OK). Otherwise
 * PTMI_E_STATE: no medium in place. PTMI_E_INVALID: a value that is not finite or outside [0, 1], filter > 1, a non-zero reserved word,
 * a dimension above 1024. PTMI_E_UNSUPPORTED: the optical-depth limit. A failed call leaves the grid in place. params NULL: nearest.
 * ptmi_set_medium with a new medium keeps the grid, stretched over the new box; it checks the optical-depth limit again
 * (PTMI_E_UNSUPPORTED leaves everything as it was). ptmi_set_medium(NULL) removes the medium and the grid. Synchronises. */
int ptmi_upload_medium_density(ptmi_ctx *ctx, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz, const ptmi_medium_grid *params);
/* nx = ny = nz = 0: none in place. rho_mean: the mean over the cells. A struct tag only. */
struct ptmi_medium_grid_status { uint32_t nx, ny, nz, filter; float rho_min, rho_max; double rho_mean; };   /* 32 bytes */
int ptmi_medium_grid_status(ptmi_ctx *ctx, struct ptmi_medium_grid_status *out);

/* ---- presentation (the reference's blit pass, src/shader/blit.wgsl:43-155; renderer.ts:434-449) ---- */
/* Tone-maps the output buffer (exposure 2^1, AgX, gamma 1/2.2) into a width*height canvas, row 0 = top.
 * dst_rgba_f32 (n_floats must be width*height*4, alpha 1) and/or dst_rgba8 (n_bytes must be width*height*4);
 * either pointer may be NULL (its count is then ignored). A wrong count is PTMI_E_INVALID: nothing is written.
 * Synchronises. Uses the device's log2/pow: compared with a tolerance, not bit for bit. */
int ptmi_blit(ptmi_ctx *ctx, float *dst_rgba_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes);
/* Size of the output buffer as last set by ptmi_resize (0 x 0 before). */
int ptmi_get_size(const ptmi_ctx *ctx, uint32_t *width, uint32_t *height);

/* ---- several GPUs of one node behind the same boundary (BASELINE configs[4]) ----------------------------------
 * The caller this serves is the frame loop of src/renderer/renderer.ts:415-454: one host thread, one `Renderer`, now over N
 * devices. Pixels are independent (pt.wgsl:753-761) and the RNG is seeded per (x, y, frame) (random.wgsl:3-5), so the frame's
 * rows are dealt to the devices as interleaved strips (tile_parts / tile_part / tile_strip above) with no data-path collective:
 * every device holds the whole scene, traces all frames of ITS rows and accumulates them locally. ptmi_multi_gather packs each
 * device's rows into one contiguous buffer, moves them to device 0 with ONE RCCL gather over xGMI (ncclGather,
 * /opt/rocm/include/rccl/rccl.h:745; single process, ncclCommInitAll over the listed devices) and unpacks them by row index into
 * device 0's output buffer, which then holds the frame exactly as one device would have rendered it — bit for bit.
 * librccl.so.1 is loaded when the first multi-device handle is created (not by single-device users of this library).
 * All calls are made from one host thread; work is enqueued asynchronously on one stream per device (ptmi_multi_dispatch itself
 * enqueues every device from a thread of its own for the duration of the call: ~0.3 ms of host time per device and 64-frame batch).
 * STATUS: what a one-GPU machine can check is checked — N = 1 through RCCL gives the un-sharded bits; N = 2 .. 8 contexts on one
 * device with copies in place of the collective (PTMI_MULTI_LOOPBACK) assemble the single-device frame bit for bit. The real N > 1
 * path (ncclCommInitAll over several devices, one grouped ncclGather with a NULL receive buffer on the non-roots, the unpack of slots
 * 1 .. N-1) HAS NEVER RUN: every machine this library was built and tested on has one GPU. tests/test_gpu_multi.py holds the
 * 2-device test; it skips itself below two GPUs. */
typedef struct ptmi_multi ptmi_multi;
enum {
    PTMI_MULTI_LOOPBACK = 1u    /* device-to-device copies in place of the collective: lets ONE device stand in for several (the same
                                   ordinal may then be listed more than once) — for tests of the packing on a one-GPU box; RCCL is not loaded */
};
/* ptmi_multi_gather_planes: with the PTMI_AOV_* bits, what to assemble on device 0 */
enum {
    PTMI_MULTI_PLANE_MOMENTS = 0x100u,   /* the sample-moments plane */
    PTMI_MULTI_PLANE_OUTPUT = 0x200u     /* the output buffer (what ptmi_multi_gather assembles) */
};
/* ordinals: n_devices HIP device ordinals (NULL = 0 .. n_devices-1); the first one is the root that ends up with the frame. */
int ptmi_multi_create(int n_devices, const int *ordinals, uint32_t flags, ptmi_multi **out);
int ptmi_multi_destroy(ptmi_multi *m);
const char *ptmi_multi_last_error(const ptmi_multi *m);       /* m may be NULL for creation errors */
int ptmi_multi_count(const ptmi_multi *m);
ptmi_ctx *ptmi_multi_context(ptmi_multi *m, int i);           /* device i's context (statistics, per-stage entry points); owned by m */
/* ptmi_upload_scene / _atlas / ptmi_resize on every device (the scene is replicated: <= 163 MB in BASELINE's configs) */
int ptmi_multi_upload_scene(ptmi_multi *m,
                            const ptmi_triangle *triangles, uint32_t n_triangles,
                            const ptmi_material *materials, uint32_t n_materials,
                            const ptmi_bvh_node *bvh_nodes, uint32_t n_nodes,
                            const ptmi_light *lights, uint32_t n_lights);
int ptmi_multi_upload_atlas(ptmi_multi *m, const void *texels, uint32_t width, uint32_t height, int format);
int ptmi_multi_resize(ptmi_multi *m, uint32_t width, uint32_t height);
/* ptmi_upload_environment / ptmi_set_environment on every device (replicated, like the atlas; checked once before any device changes) */
int ptmi_multi_upload_environment(ptmi_multi *m, const void *texels, uint32_t width, uint32_t height, int format,
                                  const ptmi_environment *params);
int ptmi_multi_set_environment(ptmi_multi *m, const ptmi_environment *params);
/* ptmi_set_medium on every device (replicated; checked once before any device changes) */
int ptmi_multi_set_medium(ptmi_multi *m, const ptmi_medium *medium);
/* ptmi_upload_medium_density on every device (replicated; checked once before any device changes) */
int ptmi_multi_upload_medium_density(ptmi_multi *m, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz,
                                     const ptmi_medium_grid *params);
/* Options for every device. tile_parts / tile_part are set by the library (device i renders the strips i, i + N, ...);
 * tile_strip = 0 picks the strip height: 4 rows, or the largest smaller height that makes the frame a whole number of rounds
 * (3840x2160 over 8 devices: 3), so that all devices get equal shares; tile_y0 / tile_y1 must be 0. */
int ptmi_multi_set_options(ptmi_multi *m, const ptmi_options *opt);
int ptmi_multi_get_options(const ptmi_multi *m, ptmi_options *opt);
/* ptmi_dispatch on every device, each for its own strips. Asynchronous. */
int ptmi_multi_dispatch(ptmi_multi *m, const ptmi_camera *camera, uint32_t n_frames);
/* Assembles the frame in device 0's output buffer (pack -> ncclGather -> unpack), ordered after the dispatches so far on every
 * device's stream. Asynchronous. Call it after the last frame, or every k frames for a preview (the rows keep accumulating on
 * their devices; the gather only copies). With one device it is a no-op. */
int ptmi_multi_gather(ptmi_multi *m);
int ptmi_multi_synchronize(ptmi_multi *m);
int ptmi_multi_throttle(ptmi_multi *m, uint32_t max_in_flight, uint32_t *in_flight);   /* ptmi_throttle on every device; reports the maximum */
/* gather + synchronise + copy device 0's output buffer out (width*height float4) */
int ptmi_multi_read_output(ptmi_multi *m, float *dst_rgba, size_t n_floats);
/* resume: the frame is written to every device (each keeps accumulating its rows on top of it) */
int ptmi_multi_write_output(ptmi_multi *m, const float *src_rgba, size_t n_floats);
/* gather + the blit pass on device 0 (see ptmi_blit) */
int ptmi_multi_blit(ptmi_multi *m, float *dst_rgba_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes);
/* counters summed over the devices; times (gpu_ms, *_ms) are the maximum over the devices; the rest is device 0's */
int ptmi_multi_get_stats(ptmi_multi *m, ptmi_stats *out);
int ptmi_multi_reset_stats(ptmi_multi *m);
/* time of the last ptmi_multi_gather on device 0's stream — from the moment every device has rendered its rows: pack + collective +
 * unpack, not the wait for the slowest device — in ms (-1 before the first; synchronises) */
int ptmi_multi_gather_ms(ptmi_multi *m, double *ms);          /* ... or ptmi_multi_gather_planes, whichever ran last */

/* ---- first-hit planes, moments, adaptive rounds and the denoiser over several devices ---------------------------------------------
 * ptmi_set_aovs / ptmi_set_moments on every device. The argument is checked once, before any device changes; a device that fails
 * leaves the devices already changed back at the earlier mask (the contents of a plane that had been turned off are gone). */
int ptmi_multi_set_aovs(ptmi_multi *m, uint32_t mask);
int ptmi_multi_get_aovs(const ptmi_multi *m, uint32_t *mask);
int ptmi_multi_set_moments(ptmi_multi *m, uint32_t on);
int ptmi_multi_get_moments(const ptmi_multi *m, uint32_t *on);
/* ptmi_set_projections on every device (checked once, before any device changes): ptmi_multi_dispatch and
 * ptmi_multi_dispatch_adaptive then honour the camera's projection words, and reject a bad camera before any device enqueues. */
int ptmi_multi_set_projections(ptmi_multi *m, uint32_t on);
int ptmi_multi_get_projections(const ptmi_multi *m, uint32_t *on);
/* Assembles the named planes in device 0's own planes, ordered after every device's work so far. Asynchronous, like ptmi_multi_gather.
 * planes: any combination of PTMI_AOV_*, PTMI_MULTI_PLANE_MOMENTS and PTMI_MULTI_PLANE_OUTPUT. An unknown bit: PTMI_E_INVALID; a bit
 * of a plane that is off: PTMI_E_STATE; 0 does nothing. ONE pass whatever the set: one pack kernel per device writes its rows of every
 * named plane into one contiguous share (plane after plane, rows_max x width entries each, 16 bytes an entry, 8 for PTMI_AOV_ID; every
 * device sends the largest share's size, the padding is never unpacked), one grouped ncclGather (loopback: one copy per device) moves
 * the shares, one unpack kernel on device 0 scatters them by row. Device 0's rows are in place already; rows of planes that are not
 * named are not touched. The buffers are sized for the planes that are on and remade when that set, the size or the strip height
 * changes: with everything on 72 bytes per pixel arrive on device 0.
 * STATUS: as for ptmi_multi_gather: N = 1 through RCCL and N = 2 .. 8 in loopback are tested bit for bit; the N > 1 RCCL leg of this
 * gather HAS NEVER RUN. */
int ptmi_multi_gather_planes(ptmi_multi *m, uint32_t planes);
/* gather the plane if device 0 does not hold it whole + synchronise + ptmi_read_aov / ptmi_read_moments of device 0's plane */
int ptmi_multi_read_aov(ptmi_multi *m, uint32_t which, void *dst, size_t n_bytes);
int ptmi_multi_read_moments(ptmi_multi *m, float *dst, size_t n_floats);
/* ptmi_dispatch_adaptive over every device's strips: afterwards every plane of every pixel holds, bit for bit, what
 * ptmi_dispatch_adaptive on ONE device with the same parameters leaves there (a pixel's frames are seeded per (x, y, frame) and folded
 * per pixel: the devices only have to take the same selection). Validation and error codes are ptmi_dispatch_adaptive's, checked on
 * every device before anything is enqueued. neighbourhood = 0: every device runs all rounds on its own rows. neighbourhood = 1: per
 * round, without a host synchronisation, every device writes the NOISY flag of each pixel of its rows (one byte), the flags go to every
 * device (ncclAllGather; loopback: copies ordered by events), and every device selects over its own rows from the whole-frame flags.
 * Asynchronous. STATUS: N = 1 through RCCL and loopback are tested; the N > 1 ncclAllGather HAS NEVER RUN. */
int ptmi_multi_dispatch_adaptive(ptmi_multi *m, const ptmi_camera *camera, const ptmi_adaptive_params *params, uint32_t rounds);
/* active and samples summed over the devices, min_count / max_count over the devices that have rows, rounds device 0's. Synchronises. */
int ptmi_multi_adaptive_status(ptmi_multi *m, struct ptmi_adaptive_status *out);
/* Gathers what device 0 does not hold whole of the output buffer, NORMAL, the moments plane and (when demodulating) ALBEDO, then
 * ptmi_denoise / ptmi_blit_denoised on device 0's context: the single-device planes and kernels, hence its result bit for bit.
 * The NORMAL or the moments plane off: PTMI_E_STATE; otherwise ptmi_denoise's errors. */
int ptmi_multi_denoise(ptmi_multi *m, const ptmi_denoise_params *params, float *dst_rgba, size_t n_floats);
int ptmi_multi_blit_denoised(ptmi_multi *m, float *dst_rgba_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes);

/* ---- editing a loaded scene in place -----------------------------------------------------------
 * Each call copies the records [first, first + count) over the loaded scene's, waits for the work in flight as an upload does, and is
 * synchronous. The output buffer and every plane are left alone: the caller restarts accumulation, as after any scene change. The
 * topology never changes: the node array, the leaf ranges, the triangle order and the length of every table stay as uploaded.
 * ptmi_update_triangles brings everything an upload derives from vertex positions to the values an upload of the edited triangles with
 * the uploaded tree's boxes refitted (leaf box = min / max over its triangles' vertices, inner box = union of its children) would
 * make, on the device: the triangle images, the light triangles of the shade tables, the boxes of the tree as uploaded and of the
 * walked hierarchy (own leaves: unit boxes, slivers, padding, the 16-bit grid and the quantised nodes), the root boxes and the image
 * header (ptmi_debug_read_image). Renders and the per-stage entry points give the bits of that fresh upload. With leaves = 1 the
 * quantised nodes and the leaf stream are dropped at the first update and the exact nodes are walked (quantised_kept = 0).
 * PTMI_E_INVALID: no scene, a range beyond the uploaded count, count > 0 with a NULL pointer, a vertex that is not finite (own leaves:
 * or whose edge arithmetic a + (b - a) is not). PTMI_E_UNSUPPORTED: the uploaded tree was not nested and finite (it is walked as
 * uploaded and its boxes mean what the caller made them mean). A refused call leaves the context unchanged. count = 0 is fine.
 * ptmi_update_materials / ptmi_update_lights rewrite the records and their copies in the shade tables (an emissive light's triangle
 * included); lights are checked as at upload (PTMI_E_INVALID: an unknown type, triangle_index >= n_triangles). Neither touches a tree. */
int ptmi_update_triangles(ptmi_ctx *ctx, uint32_t first, uint32_t count, const ptmi_triangle *triangles);
int ptmi_update_materials(ptmi_ctx *ctx, uint32_t first, uint32_t count, const ptmi_material *materials);
int ptmi_update_lights(ptmi_ctx *ctx, uint32_t first, uint32_t count, const ptmi_light *lights);
/* A refitted tree degrades as geometry moves. cost = the sum over every child box stored in the walked hierarchy of its surface area,
 * divided by the root box's: cost_built when the plan was made (before the first refit), cost_now after the last update. The host
 * decides from the ratio when to call ptmi_rebuild_tree (below); the library never rebuilds on its own. Before the first update after an
 * upload everything is zero. A struct tag only. */
struct ptmi_scene_update_status {
    uint32_t updates;         /* ptmi_update_triangles calls since the last upload */
    uint32_t quantised_kept;  /* 1: the walked image still has its quantised nodes */
    double   plan_ms;         /* one-time preparation at the first update after an upload (levels, numbering, scratch) */
    double   refit_ms;        /* wall time of the last ptmi_update_triangles */
    double   cost_built, cost_now;
    float    root_min[3], root_max[3];   /* the refitted root box of the tree as uploaded */
    uint32_t reserved[4];
};                            /* 80 bytes */
int ptmi_scene_update_status(ptmi_ctx *ctx, struct ptmi_scene_update_status *out);
/* the three updates on every device; the status of device 0 */
int ptmi_multi_update_triangles(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_triangle *triangles);
int ptmi_multi_update_materials(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_material *materials);
int ptmi_multi_update_lights(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_light *lights);
int ptmi_multi_scene_update_status(ptmi_multi *m, struct ptmi_scene_update_status *out);

/* ---- rebuilding the walked tree in place -------------------------------------------------------
 * A refit keeps the topology, so the walked hierarchy degrades as geometry moves (ptmi_scene_update_status: cost_now / cost_built).
 * ptmi_rebuild_tree builds the own-leaf hierarchy (leaves = 2) anew from what is on the device - the current triangles and the leaf
 * boxes of the refitted uploaded tree - and swaps it in. Afterwards ptmi_debug_read_image returns the walked image a fresh
 * ptmi_upload_scene of the current triangles, with the uploaded node array refitted as ptmi_update_triangles defines it, would build
 * under the context's current options with leaves = 2, keep_reference_tree = 0 and tree_builder = params->builder: both builders are
 * deterministic, so the same bytes (wide nodes, leaf-ordered triangle images, quantised nodes and grid, root box, pad / safe_origin,
 * depth, n_leaves, max_leaf_tris, and the 16-bit copies of scenes of at most 4 096 triangles). Renders and the per-stage entry points
 * give that upload's bits. Synchronous; waits for the work in flight as an update does. All-or-nothing: it builds into new buffers and
 * swaps on success, and a failure leaves the context exactly as it was. Nothing else is touched: the triangle order, the triangles, the
 * uploaded tree and its images, the leaf boxes, materials, lights, the shade tables, the atlas, the environment, the medium, the alpha
 * table and its counters, the motion state, the output buffer and every plane. A rebuild without an edit is allowed; with the builder
 * the upload used it reproduces the image byte for byte. The update plan is re-made for the new topology before the call returns:
 * ptmi_scene_update_status then reports cost_built = cost_now = the new tree's cost, quantised_kept as the new image has it, plan_ms
 * of the re-plan, and `updates` unchanged; ptmi_stats.tree_builder_used / leaf_tris_used follow the new image. On the device path
 * (builder 2, scenes above 4 096 triangles) nothing per triangle crosses the bus; a device build that fails (allocation, more than 60
 * levels, too many passes) falls back to the host builder as an upload does, and builder_used says 1.
 * PTMI_E_INVALID: no scene, builder > 2, a non-zero reserved word. PTMI_E_UNSUPPORTED: the loaded image has no own leaves (leaves = 1,
 * keep_reference_tree, a tree that is not nested, a single leaf, an empty scene; the message says which). ptmi_upload_scene zeroes
 * the status. */
typedef struct ptmi_rebuild_params {
    uint32_t builder;      /* who builds, with ptmi_options.tree_builder's meaning: 1 the host, 2 the device where it applies
                              (scenes above 4 096 triangles; smaller ones take the host builder); 0 -> 2 */
    uint32_t reserved[7];  /* must be 0 */
} ptmi_rebuild_params;     /* 32 bytes */
struct ptmi_rebuild_status {          /* a struct tag only; 32 bytes */
    uint32_t rebuilds;                /* since the last upload */
    uint32_t builder_used;            /* 1 / 2 of the last rebuild (0: none yet) */
    double   build_ms;                /* wall time of the last ptmi_rebuild_tree */
    double   cost_before, cost_after; /* the walked hierarchy's cost (ptmi_scene_update_status's definition) around it */
};
int ptmi_rebuild_tree(ptmi_ctx *ctx, const ptmi_rebuild_params *params /* NULL: defaults */);
int ptmi_rebuild_status(ptmi_ctx *ctx, struct ptmi_rebuild_status *out);
/* on every device, checked once before any device changes; the status of device 0 */
int ptmi_multi_rebuild_tree(ptmi_multi *m, const ptmi_rebuild_params *params);
int ptmi_multi_rebuild_status(ptmi_multi *m, struct ptmi_rebuild_status *out);

/* ---- moving objects on the device: triangle groups ---------------------------------------------
 * ptmi_set_triangle_groups tags every uploaded triangle with a group id (one uint32 per triangle, in uploaded order) and snapshots the
 * REST POSE: v0, v1, v2, n0, n1, n2 of every triangle as they stand on the device now. Every group's matrix becomes "none" and
 * `transforms` is zeroed. n_groups = the largest id + 1. group NULL or n_triangles 0 removes the table. PTMI_E_INVALID: no scene,
 * n_triangles different from the uploaded count. PTMI_E_UNSUPPORTED: more than 65 536 groups. A failed call keeps the previous table.
 * ptmi_upload_scene removes the table; ptmi_rebuild_tree, ptmi_update_materials and ptmi_update_lights leave it alone.
 * ptmi_transform_groups sets the matrix of each group an op names. Transforms are ABSOLUTE, from the rest pose: every member
 * triangle's live record becomes T(rest), so a host that composes matrices gets no drift. Groups that are not named keep their
 * records (they are not rewritten). Per member triangle, in float32, in the order written, no FMA:
 *   vertex p:  p'_k = ((m[4k] * p.x + m[4k+1] * p.y) + m[4k+2] * p.z) + m[4k+3]                                  k = x, y, z
 *   normal n:  q_k = (nm[3k] * n.x + nm[3k+1] * n.y) + nm[3k+2] * n.z;  l2 = (q.x * q.x + q.y * q.y) + q.z * q.z;
 *              n'_k = q_k / sqrt(l2) where l2 > 0 (both correctly rounded), else n' = q
 * The uvs, material_index and the seven padding words keep their bits. Afterwards the call runs the refit of ptmi_update_triangles:
 * the state is bit for bit what ptmi_update_triangles(0, n_triangles, the transformed records) leaves (triangle images, light triangles,
 * both trees, root boxes, image header, quantised_kept, cost_now; ptmi_scene_update_status.updates grows by one), except that while
 * motion is on the dirty range is widened to [lowest member, highest member] of the groups named only. n_ops = 0, or ops whose groups
 * have no members, do what ptmi_update_triangles(0, 0, NULL) does. Point and directional lights are NOT moved: that is
 * ptmi_update_lights' business (an emissive light follows its triangle, as after any triangle update).
 * All-or-nothing. On the host: PTMI_E_STATE without a table; PTMI_E_INVALID for ops NULL with n_ops > 0, a matrix entry that is not
 * finite, a non-zero reserved word, group >= n_groups, a group named twice; PTMI_E_UNSUPPORTED where ptmi_update_triangles gives it.
 * On the device, before anything of the scene is written, a check pass applies ptmi_update_triangles' vertex checks to the
 * transformed vertices (every component finite; own leaves: a + (b - a) and a + (d - a) finite too). On a failure the call returns
 * PTMI_E_INVALID, first_bad holds the smallest offending triangle index and the context is otherwise unchanged; on success first_bad
 * is 0xFFFFFFFF. ptmi_update_triangles while a table is in place re-bases: the records it writes become the rest pose of their
 * triangles (the groups' matrices stay; they apply to the new rest pose at the next ptmi_transform_groups that names them).
 * ptmi_normal_matrix (host only, no context): nm = the cofactor matrix of the upper 3 x 3 of m, each entry a*b - c*d in double in
 * that order, rounded to float. It handles non-uniform scale; a mirror flips the normals with the winding. */
typedef struct ptmi_group_transform {
    uint32_t group;
    uint32_t reserved0;      /* must be 0 */
    float    m[12];          /* 3 x 4 affine, row-major: row k = m[4k .. 4k+3] */
    float    nm[9];          /* 3 x 3 applied to the normals, row-major */
    uint32_t reserved1;      /* must be 0 */
} ptmi_group_transform;      /* 96 bytes */
struct ptmi_transform_status {        /* a struct tag only; 32 bytes. Without a table every word is zero. */
    uint32_t present, n_groups;       /* a table is in place; the largest id + 1 */
    uint32_t transforms;              /* successful ptmi_transform_groups calls since the table was set */
    uint32_t last_moved;              /* member triangles the last of them rewrote */
    uint32_t first_bad, reserved;     /* the last call's check pass: the smallest offending triangle, 0xFFFFFFFF for none */
    double   transform_ms;            /* wall time of the last successful ptmi_transform_groups, its refit included */
};
int ptmi_set_triangle_groups(ptmi_ctx *ctx, const uint32_t *group, uint32_t n_triangles);
int ptmi_transform_groups(ptmi_ctx *ctx, const ptmi_group_transform *ops, uint32_t n_ops);
void ptmi_normal_matrix(const float m[12], float nm[9]);
int ptmi_transform_status(ptmi_ctx *ctx, struct ptmi_transform_status *out);
/* the live records [first, first + count) as they stand on the device; synchronises. PTMI_E_INVALID: no scene, a range beyond the
 * uploaded count, count > 0 with out NULL */
int ptmi_debug_read_triangles(ptmi_ctx *ctx, uint32_t first, uint32_t count, ptmi_triangle *out);
/* on every device, checked once before any device changes; the status of device 0 */
int ptmi_multi_set_triangle_groups(ptmi_multi *m, const uint32_t *group, uint32_t n_triangles);
int ptmi_multi_transform_groups(ptmi_multi *m, const ptmi_group_transform *ops, uint32_t n_ops);
int ptmi_multi_transform_status(ptmi_multi *m, struct ptmi_transform_status *out);

/* ---- skinned meshes on the device: linear-blend skinning ---------------------------------------
 * ptmi_set_skin takes a LIST of skinned triangles (triangle[]: indices in uploaded order, strictly ascending) and three corner records
 * per listed triangle (v0, v1, v2): four joint indices and four weights each. It snapshots the REST (bind) POSE of the listed
 * triangles - v0, v1, v2, n0, n1, n2, 96 bytes each, as they stand on the device now - keeps the corner records on the device and zeroes
 * `poses`. Triangles that are not listed cost nothing. triangle NULL or n_skinned 0 removes the skin. PTMI_E_INVALID: no scene, an
 * index >= the uploaded count, a list that is not strictly ascending, corners NULL, a joint[k] >= n_joints (every slot, whatever its
 * weight), a weight that is not finite, n_joints 0. PTMI_E_UNSUPPORTED: more than 65 536 joints. A failed call keeps the previous skin.
 * ptmi_upload_scene removes the skin; ptmi_rebuild_tree, ptmi_update_materials and ptmi_update_lights leave it alone.
 * ptmi_pose_skin takes a COMPLETE pose: n_joints must be the skin's, joints[i].group must be i and the reserved words 0 (a record
 * array describes itself; a shuffled one is refused). Transforms are ABSOLUTE, from the rest pose. Per corner with the joints j0..j3
 * and the weights w0..w3 of its record, in float32, in the order written, no FMA:
 *   B.m[e]  = ((w0 * J[j0].m[e]  + w1 * J[j1].m[e])  + w2 * J[j2].m[e])  + w3 * J[j3].m[e]                          e = 0..11
 *   B.nm[e] = ((w0 * J[j0].nm[e] + w1 * J[j1].nm[e]) + w2 * J[j2].nm[e]) + w3 * J[j3].nm[e]                         e = 0..8
 *   vertex' = the vertex formula of ptmi_transform_groups with B.m;  normal' = its normal formula with B.nm
 * All four slots are always evaluated: a zero weight is not skipped (so 0 * a matrix entry adds a signed zero, as written). This is
 * glTF's blended-matrix form of linear-blend skinning. The blended cofactor matrix B.nm is the usual approximation of the cofactor
 * matrix of the blend B.m (exact where one joint has all the weight). Weights are used as given: normalising them is the loader's
 * job. The uvs, material_index and the seven padding words keep their bits; triangles that are not listed are not written.
 * Afterwards the call runs the refit of ptmi_update_triangles: the state is bit for bit what ptmi_update_triangles(0, n_triangles,
 * the skinned records) leaves and ptmi_scene_update_status.updates grows by one, except that while motion is on the dirty range is
 * widened to [lowest listed, highest listed] only.
 * All-or-nothing. On the host: PTMI_E_STATE without a skin; PTMI_E_INVALID for joints NULL, n_joints different from the skin's,
 * group != i, a non-zero reserved word, a matrix entry that is not finite; PTMI_E_UNSUPPORTED where ptmi_update_triangles gives it.
 * On the device, before anything of the scene is written, a check pass applies ptmi_update_triangles' vertex checks to the skinned
 * vertices (as ptmi_transform_groups does): on a failure the call returns PTMI_E_INVALID, first_bad holds the smallest offending
 * triangle index and the context is otherwise unchanged; on success first_bad is 0xFFFFFFFF.
 * Interactions. ptmi_update_triangles while a skin is in place re-bases: the records it writes become the rest pose of the listed
 * triangles inside its range (listed triangles outside it keep theirs). The skin and the triangle groups keep separate rest poses and
 * neither call re-bases the other's: a triangle that is both listed and a member of a moved group takes the last writer's record.
 * (The glTF loader never produces that overlap: glTF ignores a skinned mesh's node transform.) */
typedef struct ptmi_skin_corner {
    uint32_t joint[4];
    float    weight[4];
} ptmi_skin_corner;          /* 32 bytes */
typedef ptmi_group_transform ptmi_joint_transform;   /* the same 96-byte record; `group` is the joint index */
struct ptmi_skin_status {             /* a struct tag only; 32 bytes. Without a skin every word is zero. */
    uint32_t present, n_joints;       /* a skin is in place; the joints it was set with */
    uint32_t n_skinned;               /* listed triangles */
    uint32_t poses;                   /* successful ptmi_pose_skin calls since the skin was set */
    uint32_t first_bad, reserved;     /* the last call's check pass: the smallest offending triangle, 0xFFFFFFFF for none */
    double   pose_ms;                 /* wall time of the last successful ptmi_pose_skin, its refit included */
};
int ptmi_set_skin(ptmi_ctx *ctx, const uint32_t *triangle, const ptmi_skin_corner *corners, uint32_t n_skinned, uint32_t n_joints);
int ptmi_pose_skin(ptmi_ctx *ctx, const ptmi_joint_transform *joints, uint32_t n_joints);
int ptmi_skin_status(ptmi_ctx *ctx, struct ptmi_skin_status *out);
/* on every device, checked once before any device changes; the status of device 0 */
int ptmi_multi_set_skin(ptmi_multi *m, const uint32_t *triangle, const ptmi_skin_corner *corners, uint32_t n_skinned, uint32_t n_joints);
int ptmi_multi_pose_skin(ptmi_multi *m, const ptmi_joint_transform *joints, uint32_t n_joints);
int ptmi_multi_skin_status(ptmi_multi *m, struct ptmi_skin_status *out);

/* ---- morphed meshes on the device: morph targets / blend shapes -----------------------------
 * ptmi_set_morph takes a LIST of morphed triangles (triangle[]: indices in uploaded order, strictly ascending, as for the skin) and a
 * sparse table of deltas in compressed-row form: row e, the records of listed triangle e, is deltas[row_start[e] .. row_start[e + 1])
 * with row_start[0] == 0 (n_morphed + 1 words). A row holds one record per target that displaces the triangle, strictly ascending by
 * `target`, and may be empty; a loader drops a record whose 18 numbers are all zero. row_start NULL together with deltas NULL: every
 * row is empty. The call snapshots the REST POSE of the listed triangles from the live records, keeps the list, the rows, the records
 * and the rest pose on the device and zeroes `poses`. triangle NULL or n_morphed 0 removes the morph. PTMI_E_INVALID: no scene, an
 * index >= the uploaded count, a list that is not strictly ascending, row_start or deltas NULL where records exist, a row_start that
 * is not non-decreasing from 0, a target >= n_targets or not strictly ascending within its row, a non-zero reserved word, a delta
 * component that is not finite, n_targets 0. PTMI_E_UNSUPPORTED: more than 8 192 targets (the weights of a pose live in LDS: 32 KB).
 * A failed call keeps the previous morph. ptmi_upload_scene removes the morph; ptmi_rebuild_tree, ptmi_update_materials and
 * ptmi_update_lights leave it alone.
 * ptmi_pose_morph takes one weight per target. Poses are ABSOLUTE, from the rest pose. Per corner of a listed triangle (vertex p,
 * normal q, both starting as the rest record's), in float32, in the order written, no FMA, denormals kept:
 *   for the records of the row, in order, with w = weights[record.target]:
 *       w == 0 (either sign): the record is SKIPPED (not loaded, not added)
 *       else, per component k:  p_k = p_k + w * dv_k      q_k = q_k + w * dn_k          (the product rounded, then the sum)
 *   vertex' = p.   normal' = q / sqrt(l2) where l2 = (q.x * q.x + q.y * q.y) + q.z * q.z > 0, else q (ptmi_transform_groups' tail)
 * A triangle of which no record was applied keeps its rest bits, normals included: nothing is renormalised, so an all-zero pose
 * restores the rest pose bit for bit (the skip is part of the contract: -0 + 0 * d would be +0). The uvs, material_index and the
 * padding words keep their bits. Afterwards the call runs the refit of ptmi_update_triangles: the state is bit for bit what
 * ptmi_update_triangles(0, n_triangles, the morphed records) leaves and ptmi_scene_update_status.updates grows by one, except that
 * while motion is on the dirty range is [lowest, highest] of the triangles whose live record was written.
 * All-or-nothing. On the host: PTMI_E_STATE without a morph; PTMI_E_INVALID for weights NULL, n_targets different from the morph's,
 * a weight that is not finite; PTMI_E_UNSUPPORTED where ptmi_update_triangles gives it. On the device, before anything is written,
 * a check pass applies ptmi_update_triangles' vertex checks to the morphed vertices (as ptmi_pose_skin does): on a failure the call
 * returns PTMI_E_INVALID, first_bad holds the smallest offending triangle index and the context is otherwise unchanged; on success
 * first_bad is 0xFFFFFFFF.
 * Interactions. ptmi_update_triangles re-bases the morph's rest rows inside its range. The morph and the triangle groups keep separate
 * rest poses, under the last-writer rule. MORPH AND SKIN COMPOSE, in glTF's order (morph, then skin): for a triangle that the morph
 * and the skin in place both list, ptmi_pose_morph writes its result to the SKIN'S REST ROW of that triangle, not to the live record,
 * and sets skin_stale = 1; the next successful ptmi_pose_skin brings the live records up to date and clears it. Which entries those
 * are is settled by whichever of ptmi_set_skin / ptmi_set_morph ran last (removals included; skin_stale is cleared then). If every
 * listed triangle is in the skin, no live record changes and ptmi_pose_morph runs no refit: `updates` does not grow. */
typedef struct ptmi_morph_delta {    /* 96 bytes: one target's displacement of one listed triangle */
    float dv0[3]; uint32_t target;   /* which target this record belongs to */
    float dv1[3]; uint32_t reserved0;    /* reserved words must be 0 */
    float dv2[3]; uint32_t reserved1;
    float dn0[3]; uint32_t reserved2;
    float dn1[3]; uint32_t reserved3;
    float dn2[3]; uint32_t reserved4;
} ptmi_morph_delta;
struct ptmi_morph_status {            /* a struct tag only; 48 bytes. Without a morph every word is zero. */
    uint32_t present, n_targets, n_morphed, n_records;
    uint32_t n_in_skin;               /* listed triangles that the skin in place lists too */
    uint32_t poses, active_targets;   /* successful ptmi_pose_morph calls since the morph was set; non-zero weights of the last one */
    uint32_t first_bad, skin_stale, reserved;   /* the last call's check pass (0xFFFFFFFF: none); a pose waits for ptmi_pose_skin */
    double   pose_ms;                 /* wall time of the last successful ptmi_pose_morph, its refit (if any) included */
};
int ptmi_set_morph(ptmi_ctx *ctx, const uint32_t *triangle, const uint32_t *row_start, const ptmi_morph_delta *deltas,
                   uint32_t n_morphed, uint32_t n_targets);
int ptmi_pose_morph(ptmi_ctx *ctx, const float *weights, uint32_t n_targets);
int ptmi_morph_status(ptmi_ctx *ctx, struct ptmi_morph_status *out);
/* on every device, checked once before any device changes; the status of device 0 */
int ptmi_multi_set_morph(ptmi_multi *m, const uint32_t *triangle, const uint32_t *row_start, const ptmi_morph_delta *deltas,
                         uint32_t n_morphed, uint32_t n_targets);
int ptmi_multi_pose_morph(ptmi_multi *m, const float *weights, uint32_t n_targets);
int ptmi_multi_morph_status(ptmi_multi *m, struct ptmi_morph_status *out);

/* ---- alpha cutouts ---------------------------------------------------------------------------
 * A per-material cutoff table for the loaded scene, one float per uploaded material. cutoff = 0: the material is opaque (the state of
 * every material without a table). cutoff > 0: a hit on the material is NOT THERE where the alpha of its albedo map's texel at the hit
 * is below the cutoff (alpha < cutoff, glTF's alphaMode MASK; a material without an albedo map has alpha 1). A ray that meets such a
 * hole goes on in the same direction past it with nothing else changed: no bounce counted, no RNG draw, no throughput change, no
 * roulette step. This holds for path segments and for the shadow rays of next-event estimation; `shade` sees the first hit that is
 * there, at its true distance along the ray, and the first-hit planes and ptmi_reproject see that surface too. The alpha is the atlas
 * texel's fourth channel, which nothing else reads.
 * Inactive (no table, or a table without a positive entry): every call issues the launches and gives the bits it gives without this
 * feature. Active: each bounce runs a resolve loop after `extend` and traces its shadow rays as closest-hit rays through a second loop
 * (the reference's own rule for shadow rays), on the one-stream schedule whatever ptmi_options.overlap says (the stored option is left
 * alone); a table whose holes no ray meets gives the bits of a render without it. max_layers bounds the holes one ray may pass per
 * segment: a path ray still on a hole after that many takes the hit as opaque, a shadow ray is occluded, and both are counted.
 * LIMITS: alphaMode BLEND stays opaque without ptmi_set_alpha_blend; a light sample aimed at an emissive triangle ignores that triangle's own cutout; the medium's
 * box is not cut by holes; no overlap while active.
 * cutoff NULL or n_materials 0 removes the table. PTMI_E_INVALID: no scene, n_materials different from the uploaded count, an entry
 * that is negative or not finite, max_layers > 32, a non-zero reserved word; a failed call leaves the previous table in place. The call
 * waits for the work in flight, as ptmi_set_medium does, and leaves the output and the planes alone. ptmi_upload_scene removes the
 * table (it belongs to that scene's materials); ptmi_upload_atlas and the ptmi_update_* calls leave it alone. */
typedef struct ptmi_alpha_params {
    uint32_t max_layers;      /* holes one ray may pass per segment, 1..32; 0 = default (4) */
    uint32_t reserved[3];     /* must be 0 */
} ptmi_alpha_params;          /* 16 bytes */
/* passes: holes passed; exhausted: rays still on a hole after max_layers — all four since ptmi_reset_stats. A struct tag only. */
struct ptmi_alpha_status {
    uint32_t present, n_materials, n_cutout, max_layers;      /* a table is in place; its length, positive entries and limit */
    uint64_t path_passes, path_exhausted, shadow_passes, shadow_exhausted;
};                            /* 48 bytes */
int ptmi_set_alpha_cutoff(ptmi_ctx *ctx, const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params /* NULL: defaults */);
int ptmi_alpha_status(ptmi_ctx *ctx, struct ptmi_alpha_status *out);      /* synchronises */
/* the table on every device, checked once before any device changes; the counters summed over the devices, the rest device 0's */
int ptmi_multi_set_alpha_cutoff(ptmi_multi *m, const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params);
int ptmi_multi_alpha_status(ptmi_multi *m, struct ptmi_alpha_status *out);

/* ---- alpha blending: hashed stochastic transparency -----------------------------------------
 * A per-material blend table for the loaded scene, one float per uploaded material. An entry < 0: the material is not blended (the
 * state of every material without a table; hosts write -1). An entry f in [0, 1]: the material is blended with factor f (glTF's
 * alphaMode BLEND; f is baseColorFactor[3]). A hit on a blended material examines alpha = f * a_texel, one float32 multiply, where
 * a_texel is the fourth channel of the albedo map's texel at the hit, fetched as for the cutoff rule (no albedo map: 1). The hit is
 * NOT THERE iff alpha <= xi, with xi = float(h >> 8) * 2^-24 in [0, 1) and h a hash of the ray itself (Wyman and McGuire's hashed
 * alpha testing), in wrapping uint32 arithmetic:
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     h = 0x9E3779B9;  for w in bits(o.x), bits(o.y), bits(o.z), bits(d.x), bits(d.y), bits(d.z), tri, seed:  h = mix(h ^ w)
 * (o, d) is the ray of the leg as the resolve loop holds it: the path's own origin and direction (the shadow record's, for a shadow
 * ray) on the first leg, the stepped origin and the same direction after each hole passed; bits() is the float's IEEE word (so -0.0
 * and 0.0 differ); tri is the hit triangle's index and seed the table's. So: alpha = 1 is always there, alpha = 0 is never there, and
 * in between the hit is there with probability alpha. The threshold is no draw from the path's RNG stream: a ray that passes a blended
 * hit goes on with exactly the bits it would have in a scene without that triangle, as a ray on a cutout hole does (no bounce
 * counted, no RNG draw, no throughput change), past it by the same step, reporting the distance along its original ray, under the
 * max_layers bound: a path ray still on an absent hit after that many takes it as opaque, a shadow ray is occluded, both counted
 * (ptmi_alpha_status). A camera ray's direction changes with every frame's jitter, so frames are decorrelated and the accumulated
 * image converges to the blend. Shadow rays take the same rule: a light sample's expected visibility through blended layers is the
 * product of (1 - alpha). Where a cutoff table is in place too, a hit is absent if either rule says so; the cutoff rule is asked
 * first, and a MASK hole computes no hash and counts no test.
 * Inactive (no table, or no entry >= 0): every call issues the launches and gives the bits it gives without this feature. Active: the
 * schedule of an active cutoff table (ptmi_set_alpha_cutoff above: the two resolve loops, one stream), with either table or both;
 * ptmi_debug_alpha_intersect / _occluded work with either. Each table keeps its own max_layers; the loops run to the larger of those
 * in place. ptmi_alpha_status's passes and exhausted counts count every hole passed, blended ones included.
 * LIMITS: coverage only: order-dependent compositing, coloured transmission and refraction are not modelled. A light sample aimed at
 * an emissive triangle ignores that triangle's own blend; the medium's box is not cut; ptmi_reproject's centre rays and the
 * first-hit planes take the same rule, so a blended surface appears in about alpha of its pixels or frames and the planes hold the
 * mixture.
 * factor NULL or n_materials 0 removes the table. PTMI_E_INVALID: no scene, n_materials different from the uploaded count, an entry
 * that is not finite or above 1, max_layers > 32, a non-zero reserved word; a failed call leaves the previous table in place. The call
 * waits for the work in flight and leaves the output and the planes alone. ptmi_upload_scene removes the table; ptmi_upload_atlas and
 * the ptmi_update_* calls leave it alone. */
typedef struct ptmi_alpha_blend_params {
    uint32_t max_layers;      /* absent hits one ray may pass per segment, 1..32; 0 = default (4) */
    uint32_t seed;            /* the last word of the hash */
    uint32_t reserved[2];     /* must be 0 */
} ptmi_alpha_blend_params;    /* 16 bytes */
/* tests: hits on blended materials that were examined; passes: those found absent (whether or not the ray could still go on) — all
 * four since ptmi_reset_stats. A struct tag only. */
struct ptmi_alpha_blend_status {
    uint32_t present, n_materials, n_blend, max_layers, seed, reserved;   /* a table is in place; its length, entries >= 0, limit, seed */
    uint64_t path_tests, path_passes, shadow_tests, shadow_passes;
};                            /* 56 bytes */
int ptmi_set_alpha_blend(ptmi_ctx *ctx, const float *factor, uint32_t n_materials, const ptmi_alpha_blend_params *params /* NULL: defaults */);
int ptmi_alpha_blend_status(ptmi_ctx *ctx, struct ptmi_alpha_blend_status *out);      /* synchronises */
/* the table on every device, checked once before any device changes; the counters summed over the devices, the rest device 0's */
int ptmi_multi_set_alpha_blend(ptmi_multi *m, const float *factor, uint32_t n_materials, const ptmi_alpha_blend_params *params);
int ptmi_multi_alpha_blend_status(ptmi_multi *m, struct ptmi_alpha_blend_status *out);

/* ---- the frame scissor -------------------------------------- */
/* A plain ptmi_dispatch traces no camera path of a pixel none of whose camera rays can meet the scene's root box: such a path ends at
 * bounce 0 with radiance 0 whatever its random numbers, so the output, the planes and every field of ptmi_stats are what they are
 * without the scissor, bit for bit (the paths not traced are added to segments and segments_by_bounce[0]). The rectangle is worked out
 * per dispatch, on the host, from the camera and the root box, for every jitter and every lens sample, with margins for rounding. It
 * is not applied (reason says why) to anything a miss can still contribute to, or whose pixels are not the whole band.
 * PTMI_SCISSOR=0 in the environment when the context is created switches it off.
 * ptmi_scissor_status: the last dispatch of any kind that had something to enqueue (zeros before the first; a dispatch of 0 frames,
 * of a context that owns no row of the frame, or of an empty texel list returns before the scissor is looked at and leaves the
 * previous status in place); skipped counts since ptmi_reset_stats. Does not
 * synchronise: everything it reports is known on the host when the dispatch returns. */
enum {
    PTMI_SCISSOR_APPLIED = 0,
    PTMI_SCISSOR_OFF = 1,            /* PTMI_SCISSOR=0 */
    PTMI_SCISSOR_NOT_PLAIN = 2,      /* ptmi_dispatch_adaptive, ptmi_dispatch_bake, ptmi_dispatch_probes */
    PTMI_SCISSOR_ENVIRONMENT = 3,    /* an environment map is in place (sampled or looked up): a miss adds its radiance */
    PTMI_SCISSOR_MEDIUM = 4,         /* a medium is in place: a ray may scatter before it leaves */
    PTMI_SCISSOR_AOV = 5,            /* a first-hit plane is on: a miss writes its record */
    PTMI_SCISSOR_MOMENTS = 6,        /* the moments plane is on */
    PTMI_SCISSOR_ALPHA = 7,          /* an active cutoff or blend table */
    PTMI_SCISSOR_PROJECTION = 8,     /* the camera is not a perspective camera */
    PTMI_SCISSOR_NO_PROMISE = 9,     /* the camera is inside the (inflated) box, a corner of it is not in front of the camera, a field
                                        is not finite or out of the range the argument covers, or the scene is empty */
    PTMI_SCISSOR_NOTHING = 10        /* the rectangle holds every pixel of the context's rows: nothing to skip */
};
struct ptmi_scissor_status {
    uint32_t x0, x1, y0, y1;  /* the rectangle [x0, x1) x [y0, y1) in frame pixels; the whole frame where none was worked out */
    uint32_t applied;         /* 1: the last dispatch traced the pixels inside only */
    uint32_t reason;          /* PTMI_SCISSOR_* */
    uint64_t skipped;         /* paths not traced since ptmi_reset_stats */
};                            /* 32 bytes */
int ptmi_scissor_status(ptmi_ctx *ctx, struct ptmi_scissor_status *out);

/* ---- statistics ----------------------------------------------------------- */
int ptmi_get_stats(ptmi_ctx *ctx, ptmi_stats *out);           /* synchronises */
int ptmi_reset_stats(ptmi_ctx *ctx);

/* ---- per-stage entry points (parity tests of single kernels) -------------- */
/* raygen kernel (pt.wgsl:714-750) for explicit (x, y, frame) triples. o3/d3: n*3 floats. */
int ptmi_debug_raygen(ptmi_ctx *ctx, const ptmi_camera *camera, uint32_t n, const uint32_t *xs,
                      const uint32_t *ys, const uint32_t *frames, float *o3, float *d3, uint32_t *rng);
/* the centre rays ptmi_reproject traces for `camera` (step 2 there), for the n = width*height pixels of the context's size, index
 * y*width+x. o3/d3: n*3 floats each, n_floats_each must be n*3 (else, or with a camera of another size: PTMI_E_INVALID). The origin
 * is per pixel: camera->position for the pinhole and the equirectangular projection, the pixel's point of the camera plane for an
 * orthographic camera (ptmi_set_projections). */
int ptmi_debug_center_rays(ptmi_ctx *ctx, const ptmi_camera *camera, float *o3, float *d3, size_t n_floats_each);
/* extend kernel (pt.wgsl:248-296) on caller rays: t = -1 / tri = 0xFFFFFFFF on miss. Raw: an alpha cutoff table is not consulted. */
int ptmi_debug_intersect(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3,
                         float *t, uint32_t *tri, float *u, float *v);
/* shadow kernel predicate (pt.wgsl:394/423/465); dist[i] < 0 = directional light (any hit occludes). Every negative value
 * means that: the library normalises them to -1 before the kernel sees them (inside a dispatch, -2 marks the record of an
 * emissive hit, which is added without a traversal — never a value a caller can inject here). Raw: an alpha cutoff table is not
 * consulted. */
int ptmi_debug_occluded(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3,
                        const float *dist, uint8_t *occluded);
/* The two loops of an active alpha cutoff or blend table on caller rays, the very loops the renders run (PTMI_E_STATE without a
 * cutoff table that has a positive entry or a blend table that has an entry >= 0). intersect: `extend`, then the path loop -> the first hit that is there, t measured along the caller's ray (-1 /
 * 0xFFFFFFFF: a miss). occluded: the shadow stage of a bounce with the verdict written out instead of added; dist as for
 * ptmi_debug_occluded. layers[i]: the holes ray i passed, or max_layers + 1 for a ray still on a hole after max_layers (its hit is
 * reported as it stands / it is occluded). */
int ptmi_debug_alpha_intersect(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3, float *t, uint32_t *tri, uint32_t *layers);
int ptmi_debug_alpha_occluded(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3, const float *dist, uint8_t *occluded,
                              uint32_t *layers);
/* Host-only (no context, no device): builds the traversal image ptmi_upload_scene would build and reports on it.
 * out[0] wide nodes of the rebuilt hierarchy (0: the tree is walked as uploaded), [1] leaves, [2] its depth,
 * [3] quantised nodes (0: none), [4] dwords of the leaf stream, [5] quantised child boxes that do NOT contain the exact
 * box they stand for (must be 0), [6] mean relative growth of box surface area by the quantisation, [7] structural
 * mismatches (must be 0): leaf headers or triangle records of the stream that differ from the uploaded leaf box / triangles,
 * inner boxes of the rebuilt hierarchy that are not the exact union of their children's boxes, nodes not reached once. */
int ptmi_debug_image_stats(const ptmi_triangle *triangles, uint32_t n_triangles,
                           const ptmi_bvh_node *bvh_nodes, uint32_t n_nodes, double out[8]);
/* Host-only (no context, no device): builds the traversal image ptmi_upload_scene would build under opt's `leaves`, `leaf_tris` and
 * `keep_reference_tree` (NULL: the defaults) and copies it out, for tests and tools that walk it on the CPU. Every buffer may be NULL
 * (call once for the sizes). wnodes16: n_wnodes x 16 floats (csrc/pt_device.h: two child boxes, two references); qnodes8: n_wnodes x 8
 * words (only when info->quantised; numbered top-of-tree first, not like wnodes16); tripos12: n_tris x 12 floats — (v0, w), e1, e2 with
 * w = bits(original triangle index) and the triangles in LEAF order when leaves_used = 2; leafbox8: n_triangles x 8 floats, the box of
 * the reference leaf that lists each (original) triangle (leaves_used = 2 only). */
typedef struct ptmi_image_info {
    uint32_t leaves_used, n_wnodes, n_tris, root_ref, depth, n_leaves, max_leaf_tris, quantised;
    float root_min[3], root_max[3];   /* the box tested first (leaves_used = 2: padded) */
    float pad, safe_origin;           /* leaves_used = 2: what every box was padded by; the origin distance the padding is good for */
    float q_origin[3], q_scale[3];
    uint32_t ref_depth;               /* levels of the uploaded tree */
} ptmi_image_info;
int ptmi_debug_build_image(const ptmi_triangle *triangles, uint32_t n_triangles, const ptmi_bvh_node *bvh_nodes, uint32_t n_nodes,
                           const ptmi_options *opt, ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12,
                           float *leafbox8);
/* The traversal image the context's last ptmi_upload_scene put on its device, read back with the conventions of ptmi_debug_build_image
 * (NULL buffers: only *info, for the sizes; leafbox8 has the uploaded scene's n_triangles rows). Before any upload *info is all zero.
 * Synchronises. */
int ptmi_debug_read_image(ptmi_ctx *ctx, ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12, float *leafbox8);
/* arithmetic-contract probe: out[i] = op(a[i], b[i], c[i]) evaluated on the device.
 * ops: 0 a/b, 1 sqrt(a), 2 fma(a,b,c), 3 min(a,b), 4 max(a,b), 5 sin(a), 6 cos(a),
 *      7 pow5(a), 8 f32(u32 bits of a), 9 u32(a) as bits, 10 a - trunc(a), 11 tan(a), 12 1/a (the kernels' short form) */
int ptmi_debug_math(ptmi_ctx *ctx, int op, uint32_t n, const float *a, const float *b,
                    const float *c, float *out);
/* The environment map (ptmi_upload_environment), probed with the functions the renders run. Both synchronise; PTMI_E_STATE: no map.
 * lookup: n unit directions d3 (n*3 floats) -> out4[4i .. 4i+3] = (Le.rgb, pdf) of direction i.
 * sample: the sampling routine on caller-supplied uniforms r4[4i .. 4i+3] = r1 .. r4 in place of RNG draws (PTMI_E_STATE also when
 * the map is not sampled) -> d3 the direction, out4 = (Le.rgb, density), texel[i] the texel picked. d3 / out4 / texel may be NULL. */
int ptmi_debug_env_lookup(ptmi_ctx *ctx, uint32_t n, const float *d3, float *out4);
int ptmi_debug_env_sample(ptmi_ctx *ctx, uint32_t n, const float *r4, float *d3, float *out4, uint32_t *texel);
/* The medium (ptmi_set_medium), probed with the functions the renders run. Both synchronise; PTMI_E_STATE: no medium in place.
 * step: one path segment on caller-supplied uniforms r3[3i .. 3i+2] = (r, xi1, xi2) in place of RNG draws, for the ray (o3, d3) and
 * the hit distance t_hit[i] (+inf: a miss) -> scattered[i] 0 / 1, x3 the scatter point, dir3 the sampled direction,
 * out4 = (a, b, s, phase density of dir). Without an interval s, x3, dir3 and the density are 0; without a scatter x3, dir3 and the
 * density are 0. tr: tr[i] = Tr(o3, wi3, dist[i]) (dist < 0: directional). Output pointers may be NULL. */
int ptmi_debug_medium_step(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3, const float *t_hit, const float *r3,
                           uint32_t *scattered, float *x3, float *dir3, float *out4);
int ptmi_debug_medium_tr(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *wi3, const float *dist, float *tr);
/* The density grid (ptmi_upload_medium_density), probed with the functions the renders run. Both synchronise; PTMI_E_STATE: no grid.
 * density: rho_out[i] = the lookup at point p3[3i .. 3i+2].
 * track: ray i is (o3, d3) and draws from the kernel RNG state rng_in[i] (the number of draws is open, so no list of uniforms serves).
 * mode 0: delta tracking of the segment ending at t_end[i] (+inf: a miss), on its interval as ptmi_debug_medium_step computes it
 * (without one: nothing is drawn) -> scattered[i] 0 / 1, t_out the scatter distance, value_out rho at the scatter point (both 0
 * without a scatter). mode 1: ratio tracking towards dist = t_end[i] (< 0: directional) -> scattered 0, t_out the segment's `end`,
 * value_out = T. Both: steps_out the tentative collisions, rng_out the RNG state afterwards. Output pointers may be NULL. */
int ptmi_debug_medium_density(ptmi_ctx *ctx, uint32_t n, const float *p3, float *rho_out);
int ptmi_debug_medium_track(ptmi_ctx *ctx, uint32_t n, const float *o3, const float *d3, const float *t_end, const uint32_t *rng_in,
                            uint32_t mode, uint32_t *scattered, float *t_out, float *value_out, uint32_t *steps_out, uint32_t *rng_out);
/* Host-only (no context, no device): the checks ptmi_upload_medium_density would run for this grid on this medium, with its error
 * codes (PTMI_E_INVALID also for rho NULL, a zero dimension or a medium that ptmi_set_medium would refuse) and the message under
 * ptmi_last_error(NULL). medium NULL: the grid's own checks alone, without the optical-depth limit. *out (may be NULL) = what
 * ptmi_medium_grid_status would report after the upload. */
int ptmi_debug_medium_grid_check(const ptmi_medium *medium, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz,
                                 const ptmi_medium_grid *params, struct ptmi_medium_grid_status *out);
/* Host-only (no context, no device): the tables ptmi_upload_environment would build for these texels. c_out: width*height floats
 * (c_t); prob_out / alias_out: width*height entries of the alias table; *weight_sum = sum(w). Each may be NULL. An all-black map gives
 * weight_sum 0, every c_t and prob 0 and alias[k] = k: such a map is never sampled. Errors as ptmi_upload_environment's, with the
 * message under ptmi_last_error(NULL). */
int ptmi_debug_env_table(const void *texels, uint32_t width, uint32_t height, int format, float *c_out, float *prob_out,
                         uint32_t *alias_out, double *weight_sum);
/* The kernels compute 1/x and sqrt(x) with short instruction sequences where the operand's magnitude is within
 * [2^-100, 2^100] and with the compiler's IEEE expansions elsewhere (csrc/pt_math.h). This runs both over ALL 2^32 float bit
 * patterns on the device and reports how many inputs give different bits (two NaNs count as equal) and the smallest such
 * pattern: which = 0: 1/x; 1: sqrt(x); 2: the 1/x of the triangle test, whose result is only used for |x| >= 1e-6.
 * The arithmetic contract (correctly rounded results, as the CPU oracle's '/' and sqrtf) holds iff all three report 0. */
int ptmi_debug_exact_math(ptmi_ctx *ctx, int which, uint64_t *n_different, uint32_t *first_different);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
