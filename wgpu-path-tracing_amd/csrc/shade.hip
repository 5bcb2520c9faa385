// shade.hip — the shade / next-event kernel of the wavefront path tracer.
//
// One lane per queued path segment. From the hit record (t, u, v, triangle) written by
// `extend` it rebuilds the shading state of the closest hit, applies emission, emits the
// next-event (shadow) record, samples and evaluates the BSDF, advances the ray and
// throughput, and plays Russian roulette — one iteration of the bounce loop of the
// reference (src/shader/pt.wgsl:638-709) minus its two traversals. All RNG draws of the
// bounce happen here, in the reference's order; the u32 RNG state
// travels in O.w. Survivors and emitted shadow records are flagged with one wave ballot
// each (64 paths -> one u64 word) for the ordered compaction kernel.
#include "pt_device.h"
#include "pt_math.h"
#include "pt_hit.h"
#include "pt_texel.h"
#include "pt_env.h"
#include "pt_medium.h"

namespace {

struct HitInfo {                       // pt.wgsl:86-101 (fields the bounce loop reads)
    v3 position; float t;
    v3 normal;
    v3 albedo;
    float roughness, metallic, transmission, ior;
    v3 emission; float emissive_strength;
    bool is_front;
};

// Where a bounce gets its material, its light and the light's triangle (pt_device.h, shade tables). STAGE names the tables k_shade
// copied into LDS (PT_STAGE_*): those are read from there through address-space-qualified pointers, as the
// traversal kernels read theirs (a generic pointer would make them FLAT loads, which take the texture-address path the copy exists to
// avoid); the others come from memory as they always did. Either way the same bytes arrive, the zeros of the out-of-range rules included.
typedef float f4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(3))) f4v *lds_f4p;
// a record of Q quads: copied as a whole, so that the compiler reads the fields the bounce uses in the widths that suit them (whole
// quads held in registers would keep the records' padding words live)
template <class R, int Q> PT_DEV R lds_record(lds_f4p p) {
    static_assert(sizeof(R) == Q * 16, "a record of Q quads");
    R r;
    __builtin_memcpy(&r, p, sizeof r);
    return r;
}
template <int STAGE> struct ShadeTabs {
    lds_f4p mats, lights, ltris;                // the staged tables (a table that is not staged: never read)
    PT_DEV ptmi_material material(const DevScene &sc, uint32_t mi) const {
        if (STAGE & PT_STAGE_MATS) return lds_record<ptmi_material, 8>(mats + 8u * min(mi, sc.n_mats));   // record n_mats is the zeros
        ptmi_material m;
        if (mi < sc.n_mats) m = sc.mats[mi];
        else __builtin_memset(&m, 0, sizeof m);
        return m;
    }
    PT_DEV ptmi_light light(const DevScene &sc, uint32_t li) const {
        if (STAGE & PT_STAGE_LIGHTS) return lds_record<ptmi_light, 3>(lights + 3u * li);
        return sc.lights[li];
    }
    PT_DEV ptmi_triangle light_triangle(const DevScene &sc, uint32_t li, uint32_t triangle_index) const {
        if (STAGE & PT_STAGE_LIGHTS) return lds_record<ptmi_triangle, 8>(ltris + 8u * li);
        ptmi_triangle T;
        if (triangle_index < sc.n_tris) T = sc.tris[triangle_index];
        else __builtin_memset(&T, 0, sizeof T);
        return T;
    }
};

// rayTriangleIntersect, pt.wgsl:159-226, for the closest hit only. The hit record carries (t, triangle); the barycentric
// (u, v) are the ones `extend` computed when it accepted the hit (pt_hit.h).
template <int STAGE>
PT_DEV HitInfo make_hitinfo(const DevScene &sc, const ShadeTabs<STAGE> &tabs, v3 ro, v3 rd, float t, uint32_t tri) {
    HitInfo hi;
    const ptmi_triangle &T = sc.tris[tri];
    // the whole triangle record is requested before the first use: the range tests of the short reciprocal / square root below
    // are branches, and a load placed after one is not issued before it
    const v3 tv0 = ld3(T.v0), tv1 = ld3(T.v1), tv2 = ld3(T.v2);
    const v3 tn0 = ld3(T.n0), tn1 = ld3(T.n1), tn2 = ld3(T.n2);
    const float u0x = T.uv0[0], u0y = T.uv0[1], u1x = T.uv1[0], u1y = T.uv1[1], u2x = T.uv2[0], u2y = T.uv2[1];
    const uint32_t mi = T.material_index;
    v3 e1, e2;
    float u, v;
    (void)tri_hit(tv0, tv1, tv2, ro, rd, u, v, e1, e2);
    hi.t = t;
    hi.position = madd3(rd, t, ro);
    float w = 1.0f - u - v;
    v3 geo_n = normalize3(cross3(e1, e2));
    v3 n_i = normalize3(lincomb3(tn0, w, tn1, u, tn2, v));
    const float uvx = hit_texcoord(u0x, u1x, u2x, u, v), uvy = hit_texcoord(u0y, u1y, u2y, u, v);
    hi.is_front = dot3(geo_n, rd) < 0.0f;
    const ptmi_material m = tabs.material(sc, mi);
    v4 one; one.x = one.y = one.z = one.w = 1.0f;
    v4 alb = texture_color(sc, m.albedo_map, uvx, uvy, one);
    hi.albedo = mk3(alb.x * m.base_color[0], alb.y * m.base_color[1], alb.z * m.base_color[2]);
    v4 pbr = texture_color(sc, m.pbr_map, uvx, uvy, one);
    hi.metallic = pbr.z * m.metallic;
    hi.roughness = max1(pbr.y * m.roughness, 0.04f);
    hi.transmission = m.transmission;
    hi.ior = m.ior;
    v4 em = texture_color(sc, m.emissive_map, uvx, uvy, one);
    hi.emission = mk3(em.x * m.emission[0], em.y * m.emission[1], em.z * m.emission[2]);
    hi.emissive_strength = m.emissive_strength;
    v4 flat; flat.x = 0.5f; flat.y = 0.5f; flat.z = 1.0f; flat.w = 1.0f;
    v4 nm = texture_color(sc, m.normal_map, uvx, uvy, flat);
    if (nm.x != 0.5f || nm.y != 0.5f || nm.z != 1.0f) {
        float du1x = u1x - u0x, du1y = u1y - u0y;
        float du2x = u2x - u0x, du2y = u2y - u0y;
        float rr = rcp1(fma1(du1x, du2y, -(du1y * du2x)));
        v3 tg = mk3(fma1(e1.x, du2y, -(e2.x * du1y)) * rr, fma1(e1.y, du2y, -(e2.y * du1y)) * rr,
                    fma1(e1.z, du2y, -(e2.z * du1y)) * rr);
        tg = normalize3(tg);
        v3 N = n_i;
        v3 Tn = normalize3(madd3(N, -dot3(N, tg), tg));
        v3 Bn = normalize3(cross3(N, Tn));
        float tx = nm.x * 2.0f - 1.0f, ty = nm.y * 2.0f - 1.0f, tz = nm.z * 2.0f - 1.0f;
        hi.normal = normalize3(lincomb3(Tn, tx, Bn, ty, N, tz));
    } else {
        hi.normal = n_i;
    }
    return hi;
}

PT_DEV float distribution_ggx(v3 N, v3 H, float roughness) {   // pt.wgsl:316-325
    float a = roughness * roughness;
    float a2 = a * a;
    float ndh = max1(dot3(N, H), 0.0f);
    float ndh2 = ndh * ndh;
    float denom = ndh2 * (a2 - 1.0f) + 1.0f;
    return max1(a2 / (PT_PI * denom * denom), 0.0f);
}
PT_DEV float geometry_schlick_ggx(float ndv, float roughness) { // pt.wgsl:328-332
    float r = roughness + 1.0f;
    float k = (r * r) / 8.0f;
    return ndv / (ndv * (1.0f - k) + k);
}
PT_DEV float geometry_smith(v3 N, v3 V, v3 L, float roughness) { // pt.wgsl:334-340
    float ndv = max1(dot3(N, V), 0.0f);
    float ndl = max1(dot3(N, L), 0.0f);
    float g2 = geometry_schlick_ggx(ndv, roughness);
    float g1 = geometry_schlick_ggx(ndl, roughness);
    return g1 * g2;
}
PT_DEV v3 fresnel_schlick(float cos_theta, v3 F0) {             // pt.wgsl:343-345
    float p = pow5(1.0f - cos_theta);
    return mk3(fma1(1.0f - F0.x, p, F0.x), fma1(1.0f - F0.y, p, F0.y), fma1(1.0f - F0.z, p, F0.z));
}
PT_DEV float reflectance(float cos_theta, float eta) {          // pt.wgsl:616-620
    float r0 = (1.0f - eta) / (1.0f + eta);
    r0 = r0 * r0;
    return r0 + (1.0f - r0) * pow5(1.0f - cos_theta);
}
PT_DEV void construct_tbn(v3 N, v3 &T, v3 &B) {                 // pt.wgsl:624-634
    T = mk3(1.0f, 0.0f, 0.0f);
    if (__builtin_fabsf(N.x) > 0.9f) T = mk3(0.0f, 1.0f, 0.0f);
    B = normalize3(cross3(N, T));
    T = normalize3(cross3(B, N));
}
// sampleGGXNormal, pt.wgsl:348-364, from its two draws' products: (sin, cos) of 2 pi r1, r2, and the frame constructTBN gives for `normal`
PT_DEV v3 ggx_normal_from(float sp, float cp, float r2, v3 normal, v3 T, v3 B, float roughness) {
    float a = roughness * roughness;
    float cos_t = sqrt1((1.0f - r2) / (1.0f + (a * a - 1.0f) * r2));
    float sin_t = sqrt1(1.0f - cos_t * cos_t);
    return normalize3(lincomb3(T, sin_t * cp, B, sin_t * sp, normal, cos_t));
}
PT_DEV float power_heuristic(float nf, float fpdf, float ng, float gpdf) { // pt.wgsl:492-496
    float f = nf * fpdf, g = ng * gpdf;
    return (f * f) / (f * f + g * g);
}
// sampleBSDF, pt.wgsl:498-546. The three lobes of the reference each start the same way — two draws, (sin, cos) of 2 pi r1, the frame
// constructTBN builds around the shading normal (randomCosineDirection + constructTBN :299-307 / :624-634 for the diffuse lobe,
// sampleGGXNormal :348-364 for the other two) — and a wave of bounce rays holds lanes of all three: written lobe by lobe it would
// execute that prefix three times and the GGX half-vector twice, each time for a part of its lanes. Here the common part runs once for
// the whole wave and the GGX half-vector once for the specular and the transmissive lanes together: the same operations on the same
// operands in the same order for every lane (bit-identical results, same RNG draws), a fifth fewer instructions for a mixed wave.
PT_DEV v3 sample_bsdf(uint32_t &rng, const HitInfo &h, v3 rd, bool front) {
    v3 V = neg3(normalize3(rd));
    float diffuse_p = (1.0f - h.metallic) * (1.0f - h.transmission);
    float specular_p = h.metallic;
    float r = rng_f(rng);
    const float r1 = rng_f(rng), r2 = rng_f(rng);
    const float phi = (2.0f * PT_PI) * r1;
    float sp, cp; sincos1(phi, sp, cp);
    v3 T, B; construct_tbn(h.normal, T, B);
    if (r < diffuse_p) {                                            // randomCosineDirection in the frame of the normal
        const float z = sqrt1(1.0f - r2), sr = sqrt1(r2);
        return lincomb3(T, cp * sr, B, sp * sr, h.normal, z);
    }
    float rough = max1(h.roughness, 0.04f);
    v3 N = ggx_normal_from(sp, cp, r2, h.normal, T, B, rough);
    if (r < diffuse_p + specular_p) return reflect3(neg3(V), N);
    float eta = front ? rcp1(h.ior) : h.ior;
    if (!front) N = neg3(N);
    float cos_t = dot3(N, V);
    float sin_t = sqrt1(1.0f - cos_t * cos_t);
    bool cannot_refract = eta * sin_t > 1.0f;
    float F = reflectance(__builtin_fabsf(cos_t), eta);
    if (cannot_refract || (rng_f(rng) < F)) return reflect3(neg3(V), N);   // short-circuit: draw only if needed
    return refract3(neg3(V), N, eta);
}
// evalBSDF, pt.wgsl:548-614: (f*cos, pdf)
PT_DEV v4 eval_bsdf(const HitInfo &h, v3 normal, v3 V, v3 L, bool front) {
    v3 H = normalize3(add3(V, L));
    float ndl = max1(dot3(normal, L), 0.0f);
    float ndv = max1(dot3(normal, V), 0.0f);
    float ndh = max1(dot3(normal, H), 0.0f);
    float vdh = max1(dot3(V, H), 0.0f);
    v3 F0 = mk3(mix1(0.04f, h.albedo.x, h.metallic), mix1(0.04f, h.albedo.y, h.metallic),
                mix1(0.04f, h.albedo.z, h.metallic));
    v3 F = fresnel_schlick(vdh, F0);
    float G = geometry_smith(normal, V, L, h.roughness);
    float D = distribution_ggx(normal, H, h.roughness);
    float one_m_tr = 1.0f - h.transmission;
    v3 kD = mk3((1.0f - F.x) * one_m_tr, (1.0f - F.y) * one_m_tr, (1.0f - F.z) * one_m_tr);
    v3 diffuse = vdiv3(mul3(kD, h.albedo), PT_PI);
    v3 specular = vdiv3(scale3(scale3(F, G), D), max1(4.0f * ndv * ndl, PT_EPS));
    v3 bsdf = mk3(0.0f, 0.0f, 0.0f);
    float pdf = 0.0f;
    if (h.transmission > 0.0f) {
        float eta = front ? rcp1(h.ior) : h.ior;
        float cos_t = dot3(normal, V);
        float Ft = reflectance(__builtin_fabsf(cos_t), eta);
        bsdf = scale3(h.albedo, 1.0f - Ft);
        pdf = (1.0f - h.metallic) * h.transmission;
    } else {
        bsdf = scale3(add3(diffuse, specular), ndl);
        float diffuse_p = (1.0f - h.metallic) * (1.0f - h.transmission);
        float specular_p = h.metallic;
        float diffuse_pdf = ndl / PT_PI;
        float specular_pdf = D * ndh / (4.0f * vdh);
        pdf = diffuse_p * diffuse_pdf + specular_p * specular_pdf;
    }
    v4 r; r.x = bsdf.x; r.y = bsdf.y; r.z = bsdf.z; r.w = max1(pdf, PT_EPS);
    return r;
}

struct LightSample { v3 intensity; v3 wi; float pdf; float dist; bool traced; };   // dist < 0: directional; traced: the
                                                                                  // reference shoots its shadow ray for this sample

// sampleLight, pt.wgsl:374-489, without its traversal: the occlusion test is the
// `shadow` kernel's; pdf = 0 means "no record" (the :413-415 early-out).
// ENV: a sampled environment is light number n_lights — one more light to pick from, for every light's 1 / n. Picked, it takes four
// draws (pt_env.h env_sample) and leaves a directional sample: any hit occludes. inv_n goes back to the caller for the MIS weight of
// the bounce ray (k_shade).
template <int STAGE, bool ENV>
PT_DEV LightSample sample_light(const DevScene &sc, const ShadeTabs<STAGE> &tabs, uint32_t &rng, v3 hit_pos, float &inv_n_out) {
    LightSample ls;
    ls.intensity = mk3(0.0f, 0.0f, 0.0f); ls.wi = mk3(0.0f, 0.0f, 0.0f); ls.pdf = 0.0f; ls.dist = -1.0f; ls.traced = false;
    const uint32_t nl = ENV ? sc.n_lights + sc.env.sampled : sc.n_lights;
    const uint32_t li = rng_int(rng, 0u, nl - 1u);
    if (ENV && li == sc.n_lights) {
        const float inv_n = rcp1((float)nl);
        inv_n_out = inv_n;
        const float r1 = rng_f(rng), r2 = rng_f(rng), r3 = rng_f(rng), r4 = rng_f(rng);
        uint32_t texel;
        const EnvSample es = env_sample(sc.env, r1, r2, r3, r4, ls.wi, texel);
        ls.intensity = es.le;
        ls.pdf = es.pdf * inv_n;
        ls.traced = true;
        return ls;
    }
    const ptmi_light lt = tabs.light(sc, li);
    const float inv_n = rcp1((float)nl);
    if (ENV) inv_n_out = inv_n;
    if (lt.light_type == PTMI_LIGHT_DIRECTIONAL) {
        ls.wi = normalize3(neg3(ld3(lt.position)));
        ls.intensity = scale3(ld3(lt.color), lt.intensity);
        ls.pdf = inv_n * 1000.0f;
        ls.dist = -1.0f;
        ls.traced = true;
    } else if (lt.light_type == PTMI_LIGHT_POINT) {
        v3 to_l = sub3(ld3(lt.position), hit_pos);
        float dist = length3(to_l);
        if (dist > 100.0f) return ls;
        ls.wi = vdiv3(to_l, dist);
        float att = rcp1(dist * dist);
        ls.intensity = scale3(scale3(ld3(lt.color), lt.intensity), att);
        ls.pdf = inv_n * 10000.0f;
        ls.dist = dist;
        ls.traced = true;
    } else if (lt.light_type == PTMI_LIGHT_EMISSIVE) {
        const ptmi_triangle T = tabs.light_triangle(sc, li, lt.triangle_index);
        float r1 = rng_f(rng), r2 = rng_f(rng);
        float sq = sqrt1(r1);
        float u = 1.0f - sq;
        float v = r2 * sq;
        float w = 1.0f - u - v;
        v3 lp = lincomb3(ld3(T.v0), w, ld3(T.v1), u, ld3(T.v2), v);
        v3 n = normalize3(lincomb3(ld3(T.n0), w, ld3(T.n1), u, ld3(T.n2), v));
        v3 to_l = sub3(lp, hit_pos);
        float dist = length3(to_l);
        v3 wi = vdiv3(to_l, dist);
        v3 e1 = sub3(ld3(T.v1), ld3(T.v0)), e2 = sub3(ld3(T.v2), ld3(T.v0));
        float area = length3(cross3(e1, e2)) * 0.5f;
        float cos_t = __builtin_fabsf(dot3(n, neg3(wi)));
        ls.pdf = (inv_n * rcp1(area)) * (dist * dist / max1(cos_t, PT_EPS));
        ls.intensity = scale3(ld3(lt.color), lt.intensity);
        ls.wi = wi;
        ls.dist = dist;
        ls.traced = true;
    }
    return ls;
}

constexpr int SBLOCK = 256;

#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 0           /* > 0: waves per SIMD asked of the register allocator (94 VGPRs = 5 waves by itself) */
#endif
#if PT_SHADE_WAVES > 0
#define PT_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(PT_SHADE_WAVES)))
#else
#define PT_SHADE_ATTR
#endif

// ---- the steps both kinds of vertex take (the surface hit, the medium's scatter vertex) and both kinds of miss, each said once ----
// A step reports a lane's votes as its return value, never through a reference: a bool behind a reference stays a byte through
// the ballots.

// A path's last addition to L: an emissive hit, a miss under an environment, a miss with a throughput that is not finite. With
// emit_records the lane leaves a record with nothing to trace (rec_o stays (0, 0, 0, -2)) that `shadow` adds in bounce order, and the
// caller votes `shadow` and `emitted`; else the addition is made here.
PT_DEV bool terminal_add(const DevPaths &P, uint32_t emit_records, uint32_t p, v3 e, float4 &rec_d, rgb_sc &rec_c) {
    if (emit_records) {
        rec_d.w = __uint_as_float(p);
        rec_c = rgb_sc{e.x, e.y, e.z};
        return true;
    }
    const rgb_sc l = P.ldL(p);
    P.stL(p, l.x + e.x, l.y + e.y, l.z + e.z);
    return false;
}
// The first-hit record of camera ray i (AOV), 32 B at slot i (the bounce-0 queue is the identity: slot i is path i), from the
// HitInfo the bounce builds anyway: aov[2i] = (albedo.rgb, t), aov[2i + 1] = (normal.xyz, bits(triangle)) ...
PT_DEV void aov_hit(float4 *__restrict__ aov, uint32_t i, const HitInfo &hit, float tri_bits) {
    st_stream(&aov[2 * (size_t)i], make_float4(hit.albedo.x, hit.albedo.y, hit.albedo.z, hit.t));
    st_stream(&aov[2 * (size_t)i + 1], make_float4(hit.normal.x, hit.normal.y, hit.normal.z, tri_bits));
}
// ... and of a camera ray that misses: zeros and triangle 0xFFFFFFFF
PT_DEV void aov_miss(float4 *__restrict__ aov, uint32_t i) {
    st_stream(&aov[2 * (size_t)i], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    st_stream(&aov[2 * (size_t)i + 1], make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu)));
}
// What the segment in state slot q starts with: its path id (where its radiance is; pid NULL: the slot is the path id) ...
// (path_id and throughput_in take their word of ShadeParams by value: called with the struct by reference from the scatter vertex,
// the kernels with a medium came out with other registers. continue_path takes the struct and does not have that effect.)
PT_DEV uint32_t path_id(const uint32_t *pid, uint32_t q) { return pid ? pid[q] : q; }
// ... and its throughput (pt.wgsl:639): (D.w, C.xy) of the slot for a bounce > 0, D being loaded already; raygen stores none, a
// camera ray's is 1. (The environment miss calls stored_throughput itself: the weight in P.W is read under the same test, and with
// the test in here that load leaves its branch and the kernels with an environment map take other registers.)
PT_DEV v3 stored_throughput(const DevPaths &P, uint32_t q, float4 d4) {
    const float2 c2 = ld_stream(&P.C[q]);
    return mk3(d4.w, c2.x, c2.y);
}
PT_DEV v3 throughput_in(const DevPaths &P, uint32_t bounce, uint32_t q, float4 d4) {
    v3 thr = mk3(1.0f, 1.0f, 1.0f);
    if (bounce != 0u) thr = stored_throughput(P, q, d4);
    return thr;
}

// How a vertex hands its path on: Russian roulette (pt.wgsl:699-705), then, unless this was the last bounce, the surviving path's
// state into slot q: the ray (o, nd), the RNG state in O.w, the throughput in (D.w, C.xy). Returns whether the path survived.
// ENV, while the map is sampled: the bounce ray carries in P.W what the environment's radiance weighs if this ray misses: where this
// vertex's next-event sample could have picked the same direction (inv_n != 0: it ran, sample_light), the power heuristic of the
// path's own density against the environment's at nd; else 1. own_pdf() is that density, asked for only there: the BSDF's pdf at a
// surface, the phase value at a scatter vertex.
// (Three things here are shaped by what the compiler in use makes of them, to keep the kernels without an environment map the code
// they were before this was a function: alive is a flag and not an early return, rng is a reference though no caller reads it
// afterwards, own_pdf is a callable and not a float. None of them is needed for correctness; with another compiler, or once those
// kernels may change, a plain `float own_pdf`, `uint32_t rng` and early returns are the simpler form.)
template <bool ENV, class OwnPdf>
PT_DEV bool continue_path(const DevScene &sc, const DevPaths &P, const ShadeParams &sp, uint32_t q, uint32_t &rng, v3 o, v3 nd, v3 thr,
                          OwnPdf own_pdf, float inv_n) {
    bool alive = true;
    if (pt_plays_roulette(sp.bounce)) {
        float pr = max1(max1(thr.x, thr.y), thr.z);
        if (rng_f(rng) > pr) alive = false;
        else thr = vdiv3(thr, pr);
    }
    if (alive && sp.bounce + 1u < sp.max_bounces) {
        st_stream(&P.O[q], make_float4(o.x, o.y, o.z, __uint_as_float(rng)));
        st_stream(&P.D[q], make_float4(nd.x, nd.y, nd.z, thr.x));
        st_stream(&P.C[q], make_float2(thr.y, thr.z));
        if (ENV && P.W) {
            float w = 1.0f;
            if (inv_n != 0.0f) w = power_heuristic(1.0f, own_pdf(), 1.0f, env_lookup(sc.env, nd).pdf * inv_n);
            P.W[q] = w;
        }
    }
    return alive;
}

// AOV: the instantiation launched for bounce 0 while first-hit planes are enabled (ptmi_set_aovs). It also writes the path's first-hit
// record (aov_hit, aov_miss). The other instantiation never reads `aov` and is the bounce kernel as it was.
//
// Shadow records (next-event samples, and with emit_records the records of emissive hits and non-finite misses) are held in
// registers until the wave's ballot and then packed at the front of the wave's 64 slots: the lane with `rank` records below it
// writes record 64 * (i / 64) + rank. Slot order is kept (the compaction lists positions in that order, pipeline.hip), and the
// lines `shadow` reads are the filled ones: where 59 % of the slots leave a record (Cornell, MIS), the records left at their own
// slots put a record in nearly every line of all three streams.
//
// STAGE (PT_STAGE_*, chosen per launch by pt_shade_stage): the shade tables the workgroup copies into LDS before its first segment. On
// the scenes measured every lane of every bounce fetched its material, its light and the light's triangle from a handful of records
// through its own vector loads, three dependent rounds behind the hit's triangle; from LDS they cost ds_reads on another unit.
//
// ENV: the instantiations launched while an environment map is in place (DevScene::env). A ray that misses — a camera
// ray too — adds throughput * (W * Le(direction)) where an emissive hit's addition goes; while the map is sampled it is one more light
// for next-event estimation (sample_light), and the bounce ray carries W in P.W for the bounce that may miss (continue_path).
// Without ENV the kernel is the one it was: no branch of it reads the map.
//
// MED: the instantiations launched while a participating medium is in place (DevScene::med; DESIGN.md §11, pt_medium.h), with or
// without ENV. A segment that crosses the box takes one draw for its free flight before any other; a collision in front of the hit (or
// anywhere along a miss) makes the segment a SCATTER, decided before the hit's triangle and material are fetched and before the sky is
// looked up: albedo, next-event estimation with the phase value where the BSDF's value and pdf stand, a direction sampled from the
// phase function, roulette. Otherwise the segment is shaded as without a medium, except that every next-event sample's contribution
// takes the transmittance towards its light. Without MED the kernel is the one it was: no branch of it reads the medium.
// MED is PT_MED_HOMOGENEOUS for that medium and PT_MED_GRID while a density grid is in place (ptmi_upload_medium_density; DESIGN.md
// §12): the one free-flight draw becomes delta tracking against the majorant sigma_t and the transmittance becomes ratio tracking,
// both with draws from the path's RNG (pt_medium.h); everything around them is the same code. The instantiations without a grid
// contain none of it.
template <bool AOV, int STAGE, bool ENV, int MED>
__global__ __launch_bounds__(SBLOCK) PT_SHADE_ATTR void k_shade(DevScene sc, DevPaths P, const uint32_t *__restrict__ queue,
                                                  const uint32_t *__restrict__ count_ptr,
                                                  const float2 *__restrict__ hits, DevShadow S,
                                                  uint64_t *__restrict__ alive_mask,
                                                  uint64_t *__restrict__ shadow_mask, ShadeParams sp,
                                                  float4 *__restrict__ aov) {
    extern __shared__ float4 smem[];
    const uint32_t count = *count_ptr;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t mats_q = (STAGE & PT_STAGE_MATS) ? (uint32_t)pt_tab_mats_q(sc.n_mats) : 0u;          // staged quads of each table
    const uint32_t lights_q = (STAGE & PT_STAGE_LIGHTS) ? (uint32_t)pt_tab_lights_q(sc.n_lights) : 0u;
    if (STAGE) {
        const float4 *src = sc.shade_tab + ((STAGE & PT_STAGE_MATS) ? 0u : pt_tab_mats_q(sc.n_mats));
        for (uint32_t k = threadIdx.x; k < mats_q + lights_q; k += SBLOCK) smem[k] = src[k];
        __syncthreads();
    }
    const lds_f4p lds_lights = (lds_f4p)smem + mats_q;
    const ShadeTabs<STAGE> tabs{(lds_f4p)smem, lds_lights, lds_lights + 3u * sc.n_lights};
    uint32_t *__restrict__ const count_words = sp.counts;
    for (uint32_t base = blockIdx.x * SBLOCK; base < count; base += gridDim.x * SBLOCK) {
        const uint32_t i = base + threadIdx.x;
        bool alive = false, shadow = false, skipped = false, emitted = false;
        float4 rec_o = make_float4(0.0f, 0.0f, 0.0f, -2.0f), rec_d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // the record (SO, SD, SC)
        rgb_sc rec_c{0.0f, 0.0f, 0.0f};
        if (i < count) {
            const uint32_t q = queue ? queue[i] : i;                         // where this ray's state is
            const float2 h2 = ld_stream(&hits[i]);
            bool scattered = false;
            uint32_t med_rng = 0u;                                           // MED: the RNG state behind the free-flight draw, if one was taken
            float4 med_o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), med_d4 = med_o4;   // MED: the segment's O and D, loaded once for every branch
            if (MED) {
                med_o4 = ld_stream(&P.O[q]); med_d4 = ld_stream(&P.D[q]);
                const float4 o4 = med_o4, d4 = med_d4;
                const v3 ro = xyz(o4), rd = xyz(d4);
                const bool is_hit = !(h2.x < 0.0f);
                const MedInterval iv = med_interval(sc.med, ro, rd, is_hit ? h2.x : __builtin_inff());
                med_rng = __float_as_uint(o4.w);
                if (iv.b > iv.a) {
                    float t_sc;
                    bool capped = false;                                     // GRID: the tracking loop reached its cap, the path ends
                    if (MED == PT_MED_GRID) {
                        uint32_t steps;
                        const int how = med_delta_track(sc.med, ro, rd, iv.a, iv.b, med_rng, t_sc, steps);
                        scattered = how != PT_TRACK_PASSED;
                        capped = how == PT_TRACK_CAPPED;
                    } else {
                        t_sc = iv.a + med_free_flight(sc.med, rng_f(med_rng));
                        scattered = t_sc < iv.b;
                    }
                    if (scattered) {
                        if (AOV) {                                           // the planes record the camera ray's surface hit all the same
                            if (is_hit) {
                                const HitInfo hit = make_hitinfo(sc, tabs, ro, rd, h2.x, __float_as_uint(h2.y));
                                aov_hit(aov, i, hit, h2.y);
                            } else {
                                aov_miss(aov, i);
                            }
                        }
                        const uint32_t p = path_id(sp.pid, q);
                        v3 thr = mul3(throughput_in(P, sp.bounce, q, d4), ld3(sc.med.albedo));
                        if (!(MED == PT_MED_GRID && capped) &&
                            ((thr.x != 0.0f) | (thr.y != 0.0f) | (thr.z != 0.0f))) {     // all zero: the path ends here
                            const v3 x = madd3(rd, t_sc, ro);
                            const float g = sc.med.g;
                            // Next-event estimation as at the surface hit below: the phase value where the BSDF's (f * cos, pdf) stand,
                            // the record's origin x itself. (Still written out at both vertices: change one copy, change the other. A function
                            // for it waits until the kernels that run without an environment map may change; profiles/README.md.)
                            float inv_n = 0.0f;
                            const bool have_light = ENV ? sc.n_lights + sc.env.sampled > 0u : sc.n_lights > 0u;
                            if (sp.do_mis && have_light) {
                                LightSample ls = sample_light<STAGE, ENV>(sc, tabs, med_rng, x, inv_n);
                                if (ls.pdf > 0.0f) {
                                    const float ph = med_phase(g, dot3(rd, ls.wi));
                                    float wmis = power_heuristic(1.0f, ls.pdf, 1.0f, ph);
                                    v3 direct = vdiv3(scale3(scale3(ls.intensity, ph), wmis), max1(ls.pdf, PT_EPS));
                                    v3 contrib = MED == PT_MED_GRID ? scale3(mul3(thr, direct), med_ratio_track(sc.med, x, ls.wi, ls.dist, med_rng))
                                                                    : scale3(mul3(thr, direct), med_tr(sc.med, x, ls.wi, ls.dist));
                                    if ((contrib.x != 0.0f) | (contrib.y != 0.0f) | (contrib.z != 0.0f)) {
                                        rec_o = make_float4(x.x, x.y, x.z, ls.dist);
                                        rec_d = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, __uint_as_float(p));
                                        rec_c = rgb_sc{contrib.x, contrib.y, contrib.z};
                                        shadow = true;
                                    } else {
                                        skipped = true;
                                    }
                                } else if (ls.traced) {
                                    skipped = true;
                                }
                            }
                            const float xi1 = rng_f(med_rng), xi2 = rng_f(med_rng);
                            float ct;
                            const v3 nd = med_sample_phase(g, rd, xi1, xi2, ct);      // its density is its phase value: no factor
                            alive = continue_path<ENV>(sc, P, sp, q, med_rng, x, nd, thr, [=] { return med_phase(g, ct); }, inv_n);
                        }
                    }
                }
            }
            if (MED && scattered) {
                // handled above
            } else if (!(h2.x < 0.0f)) {                                     // pt.wgsl:646: miss adds zero
                const float4 o4 = MED ? med_o4 : ld_stream(&P.O[q]), d4 = MED ? med_d4 : ld_stream(&P.D[q]);
                const uint32_t p = path_id(sp.pid, q);
                uint32_t rng = MED ? med_rng : __float_as_uint(o4.w);
                const v3 ro = xyz(o4), rd = xyz(d4);
                v3 thr = throughput_in(P, sp.bounce, q, d4);
                const HitInfo hit = make_hitinfo(sc, tabs, ro, rd, h2.x, __float_as_uint(h2.y));
                if (AOV) aov_hit(aov, i, hit, h2.y);
                if (hit.emission.x > 0.0f || hit.emission.y > 0.0f || hit.emission.z > 0.0f) {   // pt.wgsl:652-658
                    float att = rcp1(1.0f + hit.t * hit.t);
                    float k = hit.emissive_strength;
                    const v3 e = mk3(thr.x * hit.emission.x * k * att, thr.y * hit.emission.y * k * att, thr.z * hit.emission.z * k * att);
                    if (terminal_add(P, sp.emit_records, p, e, rec_d, rec_c)) { shadow = true; emitted = true; }   // the path ends here
                } else {
                    float inv_n = 0.0f;                                       // ENV: set where next-event estimation ran
                    const bool have_light = ENV ? sc.n_lights + sc.env.sampled > 0u : sc.n_lights > 0u;
                    if (sp.do_mis && have_light && hit.transmission == 0.0f && hit.is_front) {   // pt.wgsl:661
                        LightSample ls = sample_light<STAGE, ENV>(sc, tabs, rng, hit.position, inv_n);
                        if (ls.pdf > 0.0f) {
                            v3 V = neg3(normalize3(rd));
                            v4 ev = eval_bsdf(hit, hit.normal, V, ls.wi, hit.is_front);
                            float wmis = power_heuristic(1.0f, ls.pdf, 1.0f, ev.w);
                            v3 direct = vdiv3(scale3(mul3(ls.intensity, mk3(ev.x, ev.y, ev.z)), wmis),
                                              max1(ls.pdf, PT_EPS));          // pt.wgsl:674
                            v3 contrib = mul3(thr, direct);                   // pt.wgsl:675, added by `shadow`
                            if (MED == PT_MED_GRID) contrib = scale3(contrib, med_ratio_track(sc.med, hit.position, ls.wi, ls.dist, rng));
                            else if (MED) contrib = scale3(contrib, med_tr(sc.med, hit.position, ls.wi, ls.dist));
                            // A contribution of exactly zero (the light is behind the surface: NdotL = 0) leaves the
                            // radiance unchanged whatever the shadow ray finds (x + 0 = x), so that ray is counted
                            // in the statistics like the reference's traversal but neither recorded nor traced.
                            if ((contrib.x != 0.0f) | (contrib.y != 0.0f) | (contrib.z != 0.0f)) {
                                v3 so = madd3(ls.wi, PT_EPS, hit.position);
                                rec_o = make_float4(so.x, so.y, so.z, ls.dist);
                                rec_d = make_float4(ls.wi.x, ls.wi.y, ls.wi.z, __uint_as_float(p));
                                rec_c = rgb_sc{contrib.x, contrib.y, contrib.z};
                                shadow = true;
                            } else {
                                skipped = true;
                            }
                        } else if (ls.traced) {
                            skipped = true;         // the reference traces this sample (pt.wgsl:392/421/463) and then drops it:
                        }                           // its pdf is not > 0 (underflow, 0 * inf); counted, nothing to add
                    }
                    v3 dir = sample_bsdf(rng, hit, rd, hit.is_front);         // pt.wgsl:680
                    v4 ev = eval_bsdf(hit, hit.normal, neg3(normalize3(rd)), dir, hit.is_front);
                    if (!(ev.w <= 0.0f)) {                                    // pt.wgsl:685
                        v3 no = madd3(dir, PT_EPS, hit.position);             // pt.wgsl:691
                        v3 nd = normalize3(dir);
                        thr = mul3(thr, vdiv3(mk3(ev.x, ev.y, ev.z), max1(ev.w, PT_EPS)));   // pt.wgsl:696
                        alive = continue_path<ENV>(sc, P, sp, q, rng, no, nd, thr, [=] { return ev.w; }, inv_n);
                    }
                }
            } else if (ENV) {                                                 // a miss sees the environment, the camera ray too
                if (AOV) {
                    aov_miss(aov, i);
                }
                const float4 d4 = MED ? med_d4 : ld_stream(&P.D[q]);
                v3 thr = mk3(1.0f, 1.0f, 1.0f);
                float w = 1.0f;
                if (sp.bounce != 0u) {
                    thr = stored_throughput(P, q, d4);
                    if (P.W) w = P.W[q];
                }
                const v3 le = env_lookup(sc.env, xyz(d4)).le;
                const v3 e = mk3(thr.x * (w * le.x), thr.y * (w * le.y), thr.z * (w * le.z));
                // a zero leaves the radiance as it is (x + 0 = x): nothing to add, as without a map; a throughput that is not finite
                // gives NaN or infinity and is added, as without a map
                if ((e.x != 0.0f) | (e.y != 0.0f) | (e.z != 0.0f)) {
                    const uint32_t p = path_id(sp.pid, q);
                    if (terminal_add(P, sp.emit_records, p, e, rec_d, rec_c)) { shadow = true; emitted = true; }
                }
            } else if (AOV) {                                                 // bounce 0 only: a camera ray that misses
                aov_miss(aov, i);
            } else if (sp.bounce != 0u) {
                // pt.wgsl:646-648: a miss adds `throughput * vec3f(0.0)` — nothing while the throughput is finite (x + +-0 = x, and
                // the radiance is never -0), NaN in every component whose throughput is infinite or NaN (degenerate materials
                // only; the camera ray's throughput is 1). Such a path leaves a record like an emissive hit's.
                const float tx = reinterpret_cast<const float *>(&P.D[q])[3];
                const float2 c2 = ld_stream(&P.C[q]);
                if (!(__builtin_isfinite(tx) & __builtin_isfinite(c2.x) & __builtin_isfinite(c2.y))) {
                    const uint32_t p = path_id(sp.pid, q);
                    const v3 e = mk3(tx * 0.0f, c2.x * 0.0f, c2.y * 0.0f);
                    if (terminal_add(P, sp.emit_records, p, e, rec_d, rec_c)) { shadow = true; emitted = true; }
                }
            }
        }
        const uint64_t am = __ballot(alive), sm = __ballot(shadow), zm = __ballot(skipped), em = __ballot(emitted);
        if (shadow) {
            const uint32_t r = (i & ~63u) + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
            st_stream(&S.SO[r], rec_o);
            st_stream(&S.SD[r], rec_d);
            S.SC[r] = rec_c;
        }
        if (lane == 0u && i < count) {
            alive_mask[i >> 6] = am;
            shadow_mask[i >> 6] = sm;
            count_words[i >> 6] = (uint32_t)__popcll(zm) | (uint32_t)__popcll(em) << 16;   // summed by the compaction (pipeline.hip)
        }
    }
}

}  // namespace

// This file is built twice (Makefile): once under the arithmetic contract (pt_launch_shade, the default and the only
// build the parity tests compare with the oracle), once with PT_SHADE_FAST and the compiler's fast division / square root /
// contraction for ptmi_options.perf_mode = 1 (pt_launch_shade_fast): same source, same RNG draws, same control flow.
#ifdef PT_SHADE_FAST
#define PT_LAUNCH_SHADE pt_launch_shade_fast
#else
#define PT_LAUNCH_SHADE pt_launch_shade
#endif
namespace {
template <bool AOV, int STAGE, bool ENV, int MED>
void launch_shade(hipStream_t s, int blocks, const DevScene &sc, DevPaths p, const uint32_t *queue, const uint32_t *count,
                  const float2 *hits, DevShadow sh, uint64_t *alive_mask, uint64_t *shadow_mask, ShadeParams sp, float4 *aov) {
    const size_t lds = (((STAGE & PT_STAGE_MATS) ? pt_tab_mats_q(sc.n_mats) : 0) + ((STAGE & PT_STAGE_LIGHTS) ? pt_tab_lights_q(sc.n_lights) : 0)) * 16;
    hipLaunchKernelGGL((k_shade<AOV, STAGE, ENV, MED>), dim3(blocks), dim3(SBLOCK), lds, s, sc, p, queue, count, hits, sh, alive_mask,
                       shadow_mask, sp, aov);
}
}  // namespace
// the tables each launch stages: pt_shade_stage of the scene's counts (what fits PT_SHADE_LDS_BUDGET), for every instantiation; ENV
// while an environment map is in place, MED by the medium in place and its grid
void PT_LAUNCH_SHADE(hipStream_t s, int blocks, const DevScene &sc, DevPaths p, const uint32_t *queue,
                     const uint32_t *count, const float2 *hits, DevShadow sh, uint64_t *alive_mask,
                     uint64_t *shadow_mask, ShadeParams sp, float4 *aov) {
#define PT_SHADE_PICK(STAGE, MED)                                                                                         \
    (sc.env.tab ? (aov ? launch_shade<true, STAGE, true, MED> : launch_shade<false, STAGE, true, MED>)                    \
                : (aov ? launch_shade<true, STAGE, false, MED> : launch_shade<false, STAGE, false, MED>))
#define PT_SHADE_CASE(STAGE)                                                                                              \
    case STAGE:                                                                                                           \
        (!sc.med.on ? PT_SHADE_PICK(STAGE, PT_MED_NONE)                                                                   \
                    : sc.med.grid ? PT_SHADE_PICK(STAGE, PT_MED_GRID) : PT_SHADE_PICK(STAGE, PT_MED_HOMOGENEOUS))(        \
            s, blocks, sc, p, queue, count, hits, sh, alive_mask, shadow_mask, sp, aov);                                  \
        break;
    switch (pt_shade_stage(sc.n_mats, sc.n_lights)) {
        PT_SHADE_CASE(0) PT_SHADE_CASE(PT_STAGE_MATS) PT_SHADE_CASE(PT_STAGE_LIGHTS) PT_SHADE_CASE(PT_STAGE_MATS | PT_STAGE_LIGHTS)
    }
#undef PT_SHADE_CASE
#undef PT_SHADE_PICK
}
