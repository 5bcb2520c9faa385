/*
 * pt_oracle.h — CPU oracle for the path-tracing hot path (TEST INFRASTRUCTURE).
 *
 * A scalar f32 restatement of the reference's compute shader
 * (reference: src/shader/pt.wgsl + src/shader/random.wgsl), plus, as optional extras the reference does not have (pto_extras
 * below), the environment map and the participating medium of include/ptmi.h as the kernels implement them. It is the checker
 * the HIP path is compared against and the timed CPU baseline of bench.py.
 * It is NOT part of the product: nothing under wgpu-path-tracing_amd/ links,
 * loads or calls it. Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may use it.
 *
 * PARITY UNPINNED: the reference holds no golden vectors, known-answer tests or
 * fixtures for this path (its only test, src/spec/arr.test.ts, pins the partial
 * quicksort used by the BVH builder), and its WGSL cannot be executed in this
 * environment (no WebGPU implementation). This restatement is pinned only by
 * its own KATs: the integer RNG vectors of SURVEY.md Appendix B (derived with
 * Python integers, independent of this code), analytic intersection cases,
 * closed-form BSDF identities and energy tests (tests/test_oracle_*.py).
 */
#ifndef PT_ORACLE_H
#define PT_ORACLE_H

#include <stdint.h>
#include "../include/ptmi_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PTO_ATLAS_NONE = 0, PTO_ATLAS_RGBA16F = 1, PTO_ATLAS_RGBA32F = 2 };

typedef struct pto_scene {
    const ptmi_triangle *tris;   uint32_t n_tris;
    const ptmi_material *mats;   uint32_t n_mats;
    const ptmi_bvh_node *nodes;  uint32_t n_nodes;
    const ptmi_light    *lights; uint32_t n_lights;
    const void *atlas; uint32_t atlas_w, atlas_h; int32_t atlas_fmt;
} pto_scene;

typedef struct pto_options {
    uint32_t max_bounces;   /* pt.wgsl:5 MAX_BOUNCES (8) */
    uint32_t do_mis;        /* pt.wgsl:636 DO_MIS (1) */
    uint32_t y0, y1;        /* rows [y0,y1) rendered; y1 = 0 means height */
    uint32_t threads;       /* 0 = omp default */
} pto_options;

typedef struct pto_stats {
    uint64_t paths;         /* (pixel, frame) samples started */
    uint64_t segments;      /* bounce-loop iterations reaching sceneIntersect (pt.wgsl:643-644) */
    uint64_t shadow_rays;   /* shadow traversals (pt.wgsl:392/421/463) */
    uint64_t nodes_visited; /* BVH nodes popped, closest-hit + shadow */
    uint64_t tris_tested;   /* ray/triangle tests */
    uint64_t closest_hits;  /* segments that hit something */
    uint32_t max_stack;     /* peak traversal-stack occupancy */
    uint32_t threads;       /* threads used */
    double   seconds;       /* wall time of the frame loop */
} pto_stats;

/* 1 = built with PT_STRICT (literal transcription: IEEE divisions everywhere,
 * no fused multiply-add, libm sin/cos/tan/pow); 0 = the arithmetic contract
 * of DESIGN.md that the HIP kernels implement bit-for-bit. */
int pto_is_strict(void);

/* random.wgsl:3-12. state_io is advanced n times; outputs (each may be NULL):
 * states[i] = rngState after draw i, words[i] = the hashed u32, vals[i] = rand(). */
void pto_rand(uint32_t *state_io, uint32_t n, uint32_t *states, uint32_t *words, float *vals);
/* random.wgsl:3-5 */
uint32_t pto_seed(uint32_t x, uint32_t y, uint32_t frame);
/* random.wgsl:14-16 with the N-1 clamp of DESIGN.md (rand()==1.0 case) */
uint32_t pto_rand_int(uint32_t *state_io, uint32_t lo, uint32_t hi);

/* contract sin/cos (x >= 0); in strict builds this is sinf/cosf */
void pto_sincos(float x, float *s, float *c);

/* pt.wgsl:714-750: camera ray for pixels (xs[i], ys[i]) at frames[i].
 * o3/d3: n*3 floats; rng_out[i] = rngState after the 2 or 4 raygen draws. */
int pto_raygen(const ptmi_camera *cam, uint32_t n, const uint32_t *xs, const uint32_t *ys,
               const uint32_t *frames, float *o3, float *d3, uint32_t *rng_out);

/* pt.wgsl:248-296 closest hit with the reference's rules (DFS, no t cull, first
 * strictly smaller t wins). t[i] = -1 on miss, tri[i] = 0xFFFFFFFF. */
int pto_intersect(const pto_scene *s, uint32_t n, const float *o3, const float *d3,
                  float *t, uint32_t *tri, float *u, float *v, pto_stats *st);

/* Shadow predicate of pt.wgsl:394 (dist[i] < 0: directional, occluded iff t>0)
 * and pt.wgsl:423/465 (occluded iff t>0 && t < dist - 2e-6). */
int pto_occluded(const pto_scene *s, uint32_t n, const float *o3, const float *d3,
                 const float *dist, uint8_t *occluded, pto_stats *st);

/* pt.wgsl:712-762 for frames cam->frame_index .. +n_frames-1 in order.
 * out_rgba: W*H*4 floats (xyz = running mean, w = 0), read when frame > 0. */
int pto_render(const pto_scene *s, const ptmi_camera *cam, uint32_t n_frames,
               const pto_options *opt, float *out_rgba, pto_stats *st);

/* The branch census: pto_render with a table census[event * PTO_CENSUS_BOUNCES + bounce] of how often each event of the bounce
 * loop happened at each bounce (bounces from 63 on share the last column, like ptmi_stats.segments_by_bounce). Same trace(),
 * same image bits, same pto_stats as pto_render.
 *
 * "would_leave_record", "contribution_zero", "contribution_nonfinite" and "sample_pdf_not_positive" describe a next-event
 * sample as the `shade` kernel sees it, before the shadow ray is traced: its pdf and contribution as if unoccluded. For that the
 * census evaluates an occluded sample too, beside the result (it is never added). From the table follow three figures the
 * GPU reports: segments_by_bounce[b] = segment[b]; shadow_rays = sum of nee_* minus point_light_beyond_100;
 * shadow_traced = sum of would_leave_record.
 *
 * The cs_* events are the call sites in `shade` of the short reciprocal / square root / normalize (csrc/pt_math.h rcp1, sqrt1,
 * normalize3): counted when the operand is outside [2^-100, 2^100] or NaN, where the kernel takes the IEEE expansion. Sites
 * whose operand cannot leave the range are not listed: normalize of the ray direction (unit length, or the ray has missed),
 * 1 / n_lights, / pi, / max(4 NdotV NdotL, 1e-6), / max(pdf, 1e-6) of the BSDF sample, and the square roots of uniform draws
 * (zero for one RNG word in 2^32). */
#define PTO_CENSUS_BOUNCES 64
#define PTO_CENSUS_EVENTS(X) \
    X(PTO_EV_SEGMENT, "segment") \
    X(PTO_EV_MISS_FINITE, "miss_finite") \
    X(PTO_EV_MISS_NONFINITE, "miss_nonfinite") \
    X(PTO_EV_EMISSIVE_FINITE, "emissive_finite") \
    X(PTO_EV_EMISSIVE_NONFINITE, "emissive_nonfinite") \
    X(PTO_EV_NEE_DIRECTIONAL, "nee_directional") \
    X(PTO_EV_NEE_POINT, "nee_point") \
    X(PTO_EV_NEE_EMISSIVE, "nee_emissive") \
    X(PTO_EV_POINT_LIGHT_BEYOND_100, "point_light_beyond_100") \
    X(PTO_EV_WOULD_LEAVE_RECORD, "would_leave_record") \
    X(PTO_EV_CONTRIBUTION_ZERO, "contribution_zero") \
    X(PTO_EV_SAMPLE_PDF_NOT_POSITIVE, "sample_pdf_not_positive") \
    X(PTO_EV_CONTRIBUTION_NONFINITE, "contribution_nonfinite") \
    X(PTO_EV_NEE_SKIPPED_BACK_FACE, "nee_skipped_back_face") \
    X(PTO_EV_NEE_SKIPPED_TRANSMISSION, "nee_skipped_transmission") \
    X(PTO_EV_LOBE_DIFFUSE, "lobe_diffuse") \
    X(PTO_EV_LOBE_SPECULAR, "lobe_specular") \
    X(PTO_EV_LOBE_TRANSMIT_FRONT, "lobe_transmit_front") \
    X(PTO_EV_LOBE_TRANSMIT_BACK, "lobe_transmit_back") \
    X(PTO_EV_TOTAL_INTERNAL_REFLECTION, "total_internal_reflection") \
    X(PTO_EV_FRESNEL_REFLECTION, "fresnel_reflection") \
    X(PTO_EV_REFRACTION, "refraction") \
    X(PTO_EV_REFRACT_K_NEGATIVE, "refract_k_negative") \
    X(PTO_EV_NORMAL_MAP, "normal_map") \
    X(PTO_EV_NORMAL_MAP_ZERO_DET, "normal_map_zero_det") \
    X(PTO_EV_TBN_NX_ABOVE_0P9, "tbn_nx_above_0p9") \
    X(PTO_EV_NAN_NORMAL, "nan_normal") \
    X(PTO_EV_MATERIAL_OUT_OF_RANGE, "material_out_of_range") \
    X(PTO_EV_TRANSMISSION_FRACTIONAL, "transmission_fractional") \
    X(PTO_EV_ROUGHNESS_CLAMPED, "roughness_clamped") \
    X(PTO_EV_ROULETTE_KILL, "roulette_kill") \
    X(PTO_EV_ROULETTE_SURVIVAL, "roulette_survival") \
    X(PTO_EV_BOUNCE_LIMIT_END, "bounce_limit_end") \
    X(PTO_EV_MED_NO_INTERVAL, "med_no_interval") \
    X(PTO_EV_MED_INTERVAL_NO_SCATTER, "med_interval_no_scatter") \
    X(PTO_EV_MED_SCATTER_BEFORE_HIT, "med_scatter_before_hit") \
    X(PTO_EV_MED_SCATTER_ON_MISS, "med_scatter_on_miss") \
    X(PTO_EV_MED_SCATTER_THROUGHPUT_ZERO, "med_scatter_throughput_zero") \
    X(PTO_EV_MED_NEE_DIRECTIONAL, "med_nee_directional") \
    X(PTO_EV_MED_NEE_POINT, "med_nee_point") \
    X(PTO_EV_MED_NEE_EMISSIVE, "med_nee_emissive") \
    X(PTO_EV_MED_NEE_ENV, "med_nee_env") \
    X(PTO_EV_MED_CONTRIBUTION_ZERO, "med_contribution_zero") \
    X(PTO_EV_MED_SAMPLE_PDF_NOT_POSITIVE, "med_sample_pdf_not_positive") \
    X(PTO_EV_MED_WOULD_LEAVE_RECORD, "med_would_leave_record") \
    X(PTO_EV_MED_ROULETTE_KILL, "med_roulette_kill") \
    X(PTO_EV_MED_ROULETTE_SURVIVAL, "med_roulette_survival") \
    X(PTO_EV_MED_BOUNCE_LIMIT_END, "med_bounce_limit_end") \
    X(PTO_EV_SURFACE_NEE_TR_BELOW_ONE, "surface_nee_tr_below_one") \
    X(PTO_EV_SURFACE_NEE_TR_ONE, "surface_nee_tr_one") \
    X(PTO_EV_NEE_ENV, "nee_env") \
    X(PTO_EV_MISS_SKY_WEIGHTED, "miss_sky_weighted") \
    X(PTO_EV_MISS_SKY_UNWEIGHTED, "miss_sky_unweighted") \
    X(PTO_EV_MISS_SKY_ZERO, "miss_sky_zero") \
    X(PTO_EV_ENV_WEIGHT_AT_SURFACE, "env_weight_at_surface") \
    X(PTO_EV_ENV_WEIGHT_AT_SCATTER, "env_weight_at_scatter") \
    X(PTO_CS_GEO_NORMAL, "cs_geo_normal") \
    X(PTO_CS_VERTEX_NORMAL, "cs_vertex_normal") \
    X(PTO_CS_UV_DET, "cs_uv_det") \
    X(PTO_CS_TANGENT, "cs_tangent") \
    X(PTO_CS_TANGENT_ORTHO, "cs_tangent_ortho") \
    X(PTO_CS_BITANGENT, "cs_bitangent") \
    X(PTO_CS_MAPPED_NORMAL, "cs_mapped_normal") \
    X(PTO_CS_EMISSIVE_ATTENUATION, "cs_emissive_attenuation") \
    X(PTO_CS_LIGHT_DIRECTION, "cs_light_direction") \
    X(PTO_CS_POINT_DISTANCE, "cs_point_distance") \
    X(PTO_CS_POINT_RCP_DISTANCE, "cs_point_rcp_distance") \
    X(PTO_CS_POINT_ATTENUATION, "cs_point_attenuation") \
    X(PTO_CS_LIGHT_NORMAL, "cs_light_normal") \
    X(PTO_CS_EMISSIVE_DISTANCE, "cs_emissive_distance") \
    X(PTO_CS_EMISSIVE_RCP_DISTANCE, "cs_emissive_rcp_distance") \
    X(PTO_CS_LIGHT_AREA, "cs_light_area") \
    X(PTO_CS_LIGHT_RCP_AREA, "cs_light_rcp_area") \
    X(PTO_CS_EVAL_HALF, "cs_eval_half") \
    X(PTO_CS_EVAL_IOR, "cs_eval_ior") \
    X(PTO_CS_DIRECT_PDF, "cs_direct_pdf") \
    X(PTO_CS_TBN_B, "cs_tbn_b") \
    X(PTO_CS_TBN_T, "cs_tbn_t") \
    X(PTO_CS_GGX_SIN, "cs_ggx_sin") \
    X(PTO_CS_GGX_NORMAL, "cs_ggx_normal") \
    X(PTO_CS_SAMPLE_IOR, "cs_sample_ior") \
    X(PTO_CS_SAMPLE_SIN, "cs_sample_sin") \
    X(PTO_CS_REFRACT_K, "cs_refract_k") \
    X(PTO_CS_NEXT_DIRECTION, "cs_next_direction") \
    X(PTO_CS_ROULETTE, "cs_roulette")
typedef enum pto_census_event {
#define PTO_X_(id, name) id,
    PTO_CENSUS_EVENTS(PTO_X_)
#undef PTO_X_
    PTO_EV_COUNT
} pto_census_event;
int pto_render_census(const pto_scene *s, const ptmi_camera *cam, uint32_t n_frames,
                      const pto_options *opt, float *out_rgba, pto_stats *st, uint64_t *census);
int pto_census_event_count(void);
const char *pto_census_event_name(int ev);

/* ---- extras: the environment map and the participating medium ------------------------------------------------------------------
 * NOT a restatement of the reference, which has no sky and no fog: they restate include/ptmi.h §environment and §medium as the
 * `shade` kernel implements them (csrc/shade.hip k_shade<.., ENV, MED>, csrc/pt_env.h, csrc/pt_medium.h), statement by statement,
 * inside the same trace() as everything above. With ex = NULL, or neither part present, every *_ext entry point is its plain
 * namesake bit for bit, census included. Inside the arithmetic contract: everything but logf, expf (free flight, transmittance)
 * and atan2f, acosf (the sky lookup), which are libm's here and the device library's there, 1 - 2 ulp apart.
 *
 * Environment (env_texels != NULL): texels (r, g, b, c) per texel, row 0 at the +Y pole, c the texel's density over (u, v); the
 * alias table (prob, alias) per entry. The tables are inputs (ptmi_debug_env_table builds them; intensity and rotation as
 * ptmi_upload_environment resolves them: intensity not 0, |rotation| <= pi). env_sampled: 1 = it is light number n_lights for
 * next-event estimation and bounce rays carry an MIS weight; 0 = looked up only.
 * Medium (med_on != 0): ptmi_medium's fields.
 * ulp_nudge: every result of logf, expf, atan2f and acosf inside the extras is moved by this many float32 steps (0: the reference);
 * for measuring what a 1 - 2 ulp library may change, nothing else.
 *
 * border (may be NULL), per pixel (renders, the smallest over the pixel's frames) or per path: the smallest distance of any sky
 * lookup of the path, at a miss or for a bounce ray's weight, from a texel border, in texels (of u w and v h); +inf without a
 * lookup. Which texel a direction that close to a border reads is the device's atan2f / acosf's to decide.
 *
 * branches (may be NULL), per pixel (over its frames) or per path: one word hashed from every decision of the path that is not
 * arithmetic: the triangle each segment hit, interval and scatter, the light picked, whether its sample was occluded, dropped or
 * left a record, the lobe, reflection or refraction, roulette, the sky texel read. Two runs (two values of ulp_nudge) with equal
 * words took the same branches and differ by rounding alone; with different words some path went another way.
 *
 * Census: the med_*, surface_nee_tr_*, nee_env, miss_sky_* and env_weight_* events are counted only with extras present. A scatter
 * counts `segment` and the med_* events and none of the surface's; under a map a miss counts miss_sky_* instead of miss_*finite;
 * would_leave_record / contribution_zero at a surface are taken after the transmittance, as `shade` takes them. The GPU's figures:
 * shadow_rays = sum of nee_* and med_nee_* minus point_light_beyond_100; shadow_traced = would_leave_record + med_would_leave_record. */
typedef struct pto_extras {
    const float *env_texels; const float *env_prob; const uint32_t *env_alias;
    uint32_t env_w, env_h, env_sampled;
    float env_intensity, env_rotation;
    uint32_t med_on;
    float sigma_t, albedo[3], g, box_min[3], box_max[3];
    int32_t ulp_nudge;
} pto_extras;
int pto_render_ext(const pto_scene *s, const ptmi_camera *cam, uint32_t n_frames, const pto_options *opt, const pto_extras *ex,
                   float *out_rgba, float *border, uint32_t *branches, pto_stats *st);
int pto_render_census_ext(const pto_scene *s, const ptmi_camera *cam, uint32_t n_frames, const pto_options *opt, const pto_extras *ex,
                          float *out_rgba, float *border, uint32_t *branches, pto_stats *st, uint64_t *census);
/* pto_trace_path / pto_trace_paths with extras. A scatter's log record is a segment's like any other: its hit t and triangle are
 * what the traversal found behind the scatter point. */
int pto_trace_path_ext(const pto_scene *s, const ptmi_camera *cam, uint32_t x, uint32_t y, uint32_t frame, const pto_options *opt,
                       const pto_extras *ex, float *radiance3, float *log16);
int pto_trace_paths_ext(const pto_scene *s, const ptmi_camera *cam, uint64_t n, const uint32_t *xs, const uint32_t *ys,
                        const uint32_t *frames, const pto_options *opt, const pto_extras *ex, float *radiance3, uint32_t *segments,
                        float *border, uint32_t *branches);
/* The extras' functions on n inputs of 8 floats each, 8 floats out each (unused ones zero):
 *   MED_STEP   in o.xyz, d.xyz, t_hit, r     out a, b, s (free flight; 0 without an interval), scattered (0 / 1), scatter point.xyz
 *   MED_TR     in o.xyz, wi.xyz, dist        out Tr
 *   MED_PHASE  in d.xyz, xi1, xi2            out direction.xyz, sampled cosine, its phase value
 *   ENV_SAMPLE in r1, r2, r3, r4             out direction.xyz, radiance.rgb, density, texel (bits)
 *   ENV_LOOKUP in d.xyz                      out radiance.rgb, density, texel (bits), distance from a texel border */
enum { PTO_PROBE_MED_STEP = 0, PTO_PROBE_MED_TR = 1, PTO_PROBE_MED_PHASE = 2, PTO_PROBE_ENV_SAMPLE = 3, PTO_PROBE_ENV_LOOKUP = 4 };
int pto_ext_probe(const pto_extras *ex, int op, uint32_t n, const float *in, float *out);

/* Every ray a render traces, with the traversal's result (for tools that replay real rays through another traversal):
 * rec9[9 i ..] = o.xyz, d.xyz, dist (0: closest-hit ray; < 0: shadow ray to a directional light; > 0: shadow ray, the light's
 * distance), t (-1: miss), tri (bits). Rows [opt->y0, opt->y1) x n_frames; at most max_rays are stored, in no particular order;
 * returns how many were traced. No image is written. */
uint64_t pto_render_tap(const pto_scene *s, const ptmi_camera *cam, uint32_t n_frames, const pto_options *opt,
                        float *rec9, uint64_t max_rays);

/* One path, with a per-bounce log for debugging parity failures.
 * log: max_bounces+1 records of 16 floats:
 *   [0..2] ray origin, [3..5] ray dir, [6..8] throughput, [9..11] radiance,
 *   [12] rng state (bits), [13] hit t, [14] hit tri (bits), [15] alive flag
 * taken at the top of each bounce; the last written record has alive = 0.
 * radiance3 = the unclamped result of trace(). Returns the number of records. */
int pto_trace_path(const pto_scene *s, const ptmi_camera *cam, uint32_t x, uint32_t y,
                   uint32_t frame, const pto_options *opt, float *radiance3, float *log16);

/* pto_trace_path for n (x, y, frame) triples at once, threaded like pto_render (opt->threads; 0: all): radiance3[3 i ..] = the
 * unclamped result of path i, segments[i] (may be NULL) = the segments it traced = its log records with alive = 1. Both entry
 * points trace through one function. */
int pto_trace_paths(const pto_scene *s, const ptmi_camera *cam, uint64_t n, const uint32_t *xs, const uint32_t *ys,
                    const uint32_t *frames, const pto_options *opt, float *radiance3, uint32_t *segments);

/* blit.wgsl:43-155 (presentation pass; tolerance-compared). rgba/out: W*H*4 floats, out row 0 = canvas top. */
void pto_blit(const float *rgba, uint32_t W, uint32_t H, float *out_rgba);

/* out[i] = op(a[i], b[i], c[i]) with the contract's scalar helpers; op codes as
 * ptmi_debug_math in include/ptmi.h */
void pto_math(int op, uint32_t n, const float *a, const float *b, const float *c, float *out);

/* per-function probes used by the analytic KAT tests */
void pto_eval_bsdf(const float albedo[3], float roughness, float metallic, float transmission,
                   float ior, const float n[3], const float v[3], const float l[3], int front,
                   float out4[4]);
float pto_distribution_ggx(const float n[3], const float h[3], float roughness);
float pto_power_heuristic(float nf, float fpdf, float ng, float gpdf);
void pto_cosine_direction(uint32_t *state_io, float out3[3]);
void pto_sample_ggx_normal(uint32_t *state_io, const float n[3], float roughness, float out3[3]);

#ifdef __cplusplus
}
#endif
#endif
