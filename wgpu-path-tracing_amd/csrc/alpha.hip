// alpha.hip — alpha cutouts and alpha blending (include/ptmi.h ptmi_set_alpha_cutoff, ptmi_set_alpha_blend): the
// per-material cutoff and blend tables, the two resolve loops that run between the existing kernels while a cutoff table with a
// positive entry or a blend table with an entry >= 0 is in place, and their debug entry points.
//
// A hit on a material with cutoff > 0 is not there where the albedo map's alpha at the hit is below the cutoff (glTF's MASK rule).
// Neither a traversal kernel nor `shade` knows about it: after `extend`, k_alpha_resolve looks at every hit record, and a ray on a
// hole continues from beyond it as a scratch ray that `extend` traces again, until the hit that is there (or the miss) stands in
// the hit record with the distance along the ORIGINAL ray. The shadow rays of next-event estimation are traced by `extend` too, as
// closest-hit rays (the reference's own rule: pt.wgsl:392/421/463 call sceneIntersect and compare t with the limit), and
// k_alpha_shadow_resolve decides each record the way ShadowIO does.
//
// A blended material (blend factor f >= 0) asks the same question with a threshold of the ray's own: the hit is not there where
// f * alpha <= xi, xi a hash of the leg's origin and direction, the triangle and the table's seed (blend_xi). The BLEND = true
// instantiations of the two kernels are launched while a blend table is active; the BLEND = false ones are the cutout code alone.
#include "ptmi_ctx.h"
#include "pt_math.h"
#include "pt_hit.h"
#include "pt_texel.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int ABLOCK = 256;
constexpr uint32_t kDefaultLayers = 4u, kMaxLayers = 32u;

// Whether the hit of the ray (ro, rd) on triangle `tri` is a hole: the texture coordinates at the hit's (u, v) (pt_hit.h: the ones
// `shade` looks its maps up with), alpha = .w of the albedo map's texel (no map: 1).
PT_DEV bool alpha_hole(const DevScene &sc, const float *__restrict__ cutoff, uint32_t tri, v3 ro, v3 rd) {
    const ptmi_triangle &T = sc.tris[tri];
    const uint32_t mi = T.material_index;
    if (mi >= sc.n_mats) return false;                      // `shade` reads a material of zeros there: no map, alpha 1
    const float cut = cutoff[mi];
    if (!(cut > 0.0f)) return false;
    float u, v;
    (void)tri_hit(T, ro, rd, u, v);
    const float uvx = hit_texcoord(T.uv0[0], T.uv1[0], T.uv2[0], u, v), uvy = hit_texcoord(T.uv0[1], T.uv1[1], T.uv2[1], u, v);
    v4 one; one.x = one.y = one.z = one.w = 1.0f;
    return texture_color(sc, sc.mats[mi].albedo_map, uvx, uvy, one).w < cut;
}

// One round of the hash: the 32-bit finaliser with the constants 0x7feb352d / 0x846ca68b
PT_DEV uint32_t blend_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// The threshold of a blended hit (include/ptmi.h): the words of the leg's ray, the triangle and the seed, mixed in that order; the
// top 24 bits as a float in [0, 1)
PT_DEV float blend_xi(v3 o, v3 d, uint32_t tri, uint32_t seed) {
    uint32_t h = 0x9E3779B9u;
    h = blend_mix(h ^ __float_as_uint(o.x)); h = blend_mix(h ^ __float_as_uint(o.y)); h = blend_mix(h ^ __float_as_uint(o.z));
    h = blend_mix(h ^ __float_as_uint(d.x)); h = blend_mix(h ^ __float_as_uint(d.y)); h = blend_mix(h ^ __float_as_uint(d.z));
    h = blend_mix(h ^ tri); h = blend_mix(h ^ seed);
    return (float)(h >> 8) * 0x1p-24f;
}

// alpha_hole under both tables: the cutoff rule first (a MASK hole computes no hash and is no test), then the blend rule on the same
// texel. `tested`: the material is blended and the blend rule was asked. The ends need no hash: alpha <= 0 is never there, alpha >= 1
// (and a NaN) always is, as alpha <= xi says for every xi in [0, 1).
PT_DEV bool alpha_blend_hole(const DevScene &sc, const DevAlpha &a, uint32_t tri, v3 ro, v3 rd, bool &tested) {
    tested = false;
    const ptmi_triangle &T = sc.tris[tri];
    const uint32_t mi = T.material_index;
    if (mi >= sc.n_mats) return false;
    const float cut = a.cutoff ? a.cutoff[mi] : 0.0f, f = a.blend[mi];
    const bool cutout = cut > 0.0f, blended = !(f < 0.0f);
    if (!cutout && !blended) return false;
    float u, v;
    (void)tri_hit(T, ro, rd, u, v);
    const float uvx = hit_texcoord(T.uv0[0], T.uv1[0], T.uv2[0], u, v), uvy = hit_texcoord(T.uv0[1], T.uv1[1], T.uv2[1], u, v);
    v4 one; one.x = one.y = one.z = one.w = 1.0f;
    const float texel = texture_color(sc, sc.mats[mi].albedo_map, uvx, uvy, one).w;
    if (cutout && texel < cut) return true;
    if (!blended) return false;
    tested = true;
    const float alpha = f * texel;
    if (alpha <= 0.0f) return true;
    if (!(alpha < 1.0f)) return false;
    return alpha <= blend_xi(ro, rd, tri, a.blend_seed);
}

// The distance of the hit on `tri` along the ray (ro, rd) its segment STARTED with, for a ray that reached it past holes: the triangle
// test `extend` would have run for it from there (pt_hit.h), so the ray reports the bits an unobstructed ray reports. The
// distance travelled plus the last leg carries the rounding of every scratch origin (an ulp of the coordinates: 15 PT_EPS at 200
// units, enough to put a hit point under the floor it lies on); it stands in only where the test from the start rejects the hit, a
// rounding apart at an edge.
PT_DEV float alpha_hit_t(const DevScene &sc, uint32_t tri, v3 ro, v3 rd, float fallback) {
    float u, v;
    const float t = tri_hit(sc.tris[tri], ro, rd, u, v);
    return t > 0.0f ? t : fallback;
}

// The step past a hole at distance t of the ray (o, d): the next origin, and `step`, the distance from o to it. PT_EPS alone is
// below one ulp of a coordinate beyond about 8 units (the ray would meet the triangle it just left again), so the offset grows with
// the hit point: eps = max(PT_EPS, 2^-18 max|p|).
PT_DEV v3 alpha_step(v3 o, v3 d, float t, float &step) {
    const v3 p = madd3(d, t, o);
    const float m = max1(max1(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z));
    const float eps = max1(PT_EPS, 0x1p-18f * m);
    step = t + eps;
    return madd3(d, eps, p);
}

// one ballot and one atomic addition per wave: the lanes with `want` get consecutive positions of `list`, in lane order
PT_DEV void wave_append(bool want, uint32_t value, uint32_t lane, uint32_t *__restrict__ list, uint32_t *length) {
    const uint64_t m = __ballot(want);
    if (m == 0ull) return;
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(length, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0);
    if (want) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = value;
}

struct RoundIO {
    const uint32_t *in; uint32_t *out, *out_n;
};
// The lists and control words of round r (pt_device.h DevAlpha). Thread 0 of the grid zeroes the word the NEXT round appends under:
// this round neither reads nor adds to it, and the round before has finished with it.
PT_DEV RoundIO round_io(const DevAlpha &a, uint32_t round) {
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.control[(round + 1u) % 3u] = 0u;
    return RoundIO{a.list[(round & 1u) ^ 1u], a.list[round & 1u], &a.control[round % 3u]};
}

// FIRST: round 0, over the queue's slots; otherwise over the list of the round before (count_ptr is then its control word).
// Whole waves run every iteration (the ballots need all lanes), so the loop's bound is the wave's first index.
template <bool FIRST, bool BLEND>
__global__ __launch_bounds__(ABLOCK) void k_alpha_resolve(DevScene sc, DevAlpha a, uint32_t round, const float4 *__restrict__ O,
                                                          const float4 *__restrict__ D, const uint32_t *__restrict__ queue,
                                                          const uint32_t *__restrict__ count_ptr, float2 *__restrict__ hits,
                                                          uint32_t *__restrict__ layers_out) {
    const uint32_t count = *count_ptr;
    const uint32_t lane = threadIdx.x & 63u;
    const RoundIO io = round_io(a, round);
    uint32_t n_pass = 0u, n_exhausted = 0u;                 // lane 0 of each wave: one atomic per wave at the end
    uint32_t n_tested = 0u, n_absent = 0u;                  // BLEND: hits on blended materials examined, and those found absent
    for (uint64_t w0 = (uint64_t)blockIdx.x * ABLOCK + (threadIdx.x & ~63u); w0 < count; w0 += (uint64_t)gridDim.x * ABLOCK) {
        const uint32_t i = (uint32_t)w0 + lane;
        bool pass = false, exhausted = false, tested = false, absent = false;
        uint32_t slot = 0u;
        if (i < count) {
            float4 ro, rd; float2 h; float travelled = 0.0f;
            if (FIRST) {
                slot = i;
                const uint32_t p = queue ? queue[i] : i;
                ro = O[p]; rd = D[p]; h = hits[i];
            } else {
                slot = io.in[i];
                ro = a.RO[slot]; rd = a.RD[slot]; h = a.hits[i];
                travelled = ro.w;
            }
            const bool hit = !(h.x < 0.0f);
            bool hole;
            if (BLEND) { hole = hit && alpha_blend_hole(sc, a, __float_as_uint(h.y), xyz(ro), xyz(rd), tested); absent = tested & hole; }
            else hole = hit && alpha_hole(sc, a.cutoff, __float_as_uint(h.y), xyz(ro), xyz(rd));
            exhausted = hole & (round >= a.max_layers);     // still on a hole after the last trace: the hit stands as opaque
            pass = hole & !exhausted;
            if (pass) {
                float step;
                const v3 o2 = alpha_step(xyz(ro), xyz(rd), h.x, step);
                a.RO[slot] = make_float4(o2.x, o2.y, o2.z, travelled + step);
                if (FIRST) a.RD[slot] = rd;
            } else {
                // the distance is the one along the path's own ray, whose O and D were never touched
                if (!FIRST) {
                    if (hit) {
                        const uint32_t p = queue ? queue[slot] : slot;
                        h.x = alpha_hit_t(sc, __float_as_uint(h.y), xyz(O[p]), xyz(D[p]), travelled + h.x);
                    }
                    hits[slot] = h;                         // (a miss: as `extend` writes it)
                }
                if (layers_out) layers_out[slot] = exhausted ? a.max_layers + 1u : round;
            }
        }
        wave_append(pass, slot, lane, io.out, io.out_n);
        const uint64_t pm = __ballot(pass), em = __ballot(exhausted);
        if (lane == 0u) { n_pass += (uint32_t)__popcll(pm); n_exhausted += (uint32_t)__popcll(em); }
        if (BLEND) {
            const uint64_t tm = __ballot(tested), am = __ballot(absent);
            if (lane == 0u) { n_tested += (uint32_t)__popcll(tm); n_absent += (uint32_t)__popcll(am); }
        }
    }
    if (n_pass) atomicAdd(&a.stats[kCtAlphaPathPasses], (unsigned long long)n_pass);
    if (n_exhausted) atomicAdd(&a.stats[kCtAlphaPathExhausted], (unsigned long long)n_exhausted);
    if (BLEND && n_tested) atomicAdd(&a.stats[kCtBlendPathTests], (unsigned long long)n_tested);
    if (BLEND && n_absent) atomicAdd(&a.stats[kCtBlendPathPasses], (unsigned long long)n_absent);
}

template <bool FIRST, bool BLEND>
__global__ __launch_bounds__(ABLOCK) void k_alpha_shadow_resolve(DevScene sc, DevAlpha a, uint32_t round, DevPaths P, DevShadow S,
                                                                 const uint32_t *__restrict__ sq, const uint32_t *__restrict__ count_ptr,
                                                                 const float2 *__restrict__ hits0, uint8_t *__restrict__ occ_out,
                                                                 uint32_t *__restrict__ layers_out) {
    const uint32_t count = *count_ptr;
    const uint32_t lane = threadIdx.x & 63u;
    const RoundIO io = round_io(a, round);
    uint32_t n_pass = 0u, n_exhausted = 0u, n_tested = 0u, n_absent = 0u;
    for (uint64_t w0 = (uint64_t)blockIdx.x * ABLOCK + (threadIdx.x & ~63u); w0 < count; w0 += (uint64_t)gridDim.x * ABLOCK) {
        const uint32_t i = (uint32_t)w0 + lane;
        bool pass = false, exhausted = false, tested = false, absent = false;
        uint32_t rec = 0u;
        if (i < count) {
            float4 so, sd; float2 h; float travelled = 0.0f;
            if (FIRST) {
                rec = sq ? sq[i] : i;
                so = S.SO[rec]; sd = S.SD[rec]; h = hits0[i];
            } else {
                rec = io.in[i];
                so = a.RO[rec]; sd = a.RD[rec]; h = a.hits[i];
                travelled = so.w;
            }
            const float4 so0 = FIRST ? so : S.SO[rec];      // the record as `shade` left it: its origin, and the distance to the light
            bool add;
            if (FIRST && so.w == -2.0f) add = true;         // the record of an emissive hit: nothing was to be traced
            else {
                // ShadowIO::fetch's limit and the any-hit kernel's test, NaN meaning "no limit": occluded iff a hit has !(t >= tlim),
                // t being the hit's distance along the record's own ray
                const float tlim = so0.w < 0.0f ? __builtin_nanf("") : so0.w - PT_EPS * 2.0f;
                const bool hit = !(h.x < 0.0f);
                float t = h.x;
                if (!FIRST && hit) t = alpha_hit_t(sc, __float_as_uint(h.y), xyz(so0), xyz(sd), travelled + h.x);
                const bool nearer = hit & !(t >= tlim);
                add = !nearer;
                bool hole;
                if (BLEND) { hole = nearer && alpha_blend_hole(sc, a, __float_as_uint(h.y), xyz(so), xyz(sd), tested); absent = tested & hole; }
                else hole = nearer && alpha_hole(sc, a.cutoff, __float_as_uint(h.y), xyz(so), xyz(sd));
                if (hole) {
                    exhausted = round >= a.max_layers;      // unresolved after the last trace: occluded
                    pass = !exhausted;
                }
            }
            if (pass) {
                float step;
                const v3 o2 = alpha_step(xyz(so), xyz(sd), h.x, step);
                a.RO[rec] = make_float4(o2.x, o2.y, o2.z, travelled + step);
                if (FIRST) a.RD[rec] = sd;
            } else {
                if (occ_out) occ_out[rec] = add ? 0 : 1;
                else if (add) {                             // ShadowIO::finish
                    const uint32_t p = __float_as_uint(sd.w);
                    const rgb_sc l = P.ldL(p), c = S.SC[rec];
                    P.stL(p, l.x + c.x, l.y + c.y, l.z + c.z);   // pt.wgsl:675
                }
                if (layers_out) layers_out[rec] = exhausted ? a.max_layers + 1u : round;
            }
        }
        wave_append(pass, rec, lane, io.out, io.out_n);
        const uint64_t pm = __ballot(pass), em = __ballot(exhausted);
        if (lane == 0u) { n_pass += (uint32_t)__popcll(pm); n_exhausted += (uint32_t)__popcll(em); }
        if (BLEND) {
            const uint64_t tm = __ballot(tested), am = __ballot(absent);
            if (lane == 0u) { n_tested += (uint32_t)__popcll(tm); n_absent += (uint32_t)__popcll(am); }
        }
    }
    if (n_pass) atomicAdd(&a.stats[kCtAlphaShadowPasses], (unsigned long long)n_pass);
    if (n_exhausted) atomicAdd(&a.stats[kCtAlphaShadowExhausted], (unsigned long long)n_exhausted);
    if (BLEND && n_tested) atomicAdd(&a.stats[kCtBlendShadowTests], (unsigned long long)n_tested);
    if (BLEND && n_absent) atomicAdd(&a.stats[kCtBlendShadowPasses], (unsigned long long)n_absent);
}

// the lane's arrays with the context's table, words and limit: what the kernels of either loop take
DevAlpha dev_alpha(const ptmi_ctx *c) {
    DevAlpha a = c->lane.alpha;
    a.cutoff = static_cast<const float *>(c->buf[kAlphaCutoff]);
    a.control = &c->d_control[kCwAlpha];
    a.stats = c->d_counters;
    a.max_layers = c->alpha_layers > c->blend_layers ? c->alpha_layers : c->blend_layers;      // each 0 without its table
    a.blend = c->blend_count ? static_cast<const float *>(c->buf[kAlphaBlend]) : nullptr;        // non-NULL: the BLEND = true kernels
    a.blend_seed = c->blend_seed;
    return a;
}

// what either table's params struct is checked for (NULL: defaults); *layers = max_layers with its default
template <class Params>
int check_params(const Params *params, const char *name, uint32_t *layers, std::string &err) {
    *layers = kDefaultLayers;
    if (!params) return PTMI_OK;
    if (params->max_layers > kMaxLayers) return fail(err, PTMI_E_INVALID, "max_layers %u above %u", params->max_layers, kMaxLayers);
    for (uint32_t r : params->reserved) if (r) return fail(err, PTMI_E_INVALID, "a reserved word of %s is not zero", name);
    if (params->max_layers) *layers = params->max_layers;
    return PTMI_OK;
}

// the argument checks of ptmi_set_alpha_cutoff that need no context
int check_alpha(const float *cutoff, uint32_t n, const ptmi_alpha_params *params, uint32_t *layers, std::string &err) {
    const int rc = check_params(params, "ptmi_alpha_params", layers, err);
    if (rc) return rc;
    for (uint32_t i = 0; cutoff && i < n; i++)
        if (!std::isfinite(cutoff[i]) || cutoff[i] < 0.0f)
            return fail(err, PTMI_E_INVALID, "cutoff[%u] = %g is negative or not finite", i, (double)cutoff[i]);
    return PTMI_OK;
}

// the argument checks of ptmi_set_alpha_blend that need no context
int check_blend(const float *factor, uint32_t n, const ptmi_alpha_blend_params *params, uint32_t *layers, std::string &err) {
    const int rc = check_params(params, "ptmi_alpha_blend_params", layers, err);
    if (rc) return rc;
    for (uint32_t i = 0; factor && i < n; i++)
        if (!std::isfinite(factor[i]) || factor[i] > 1.0f)
            return fail(err, PTMI_E_INVALID, "factor[%u] = %g is above 1 or not finite", i, (double)factor[i]);
    return PTMI_OK;
}

// the loops' arrays live only while a table is active (ensure_capacity makes them)
void drop_idle_arrays(ptmi_ctx *c) {
    if (alpha_active(c)) return;
    for (int k = kAlphaO; k <= kAlphaHits; k++) dfree(c->lane.buf[k]);
    lane_views(c->lane);
}

// Puts `table` (n floats; NULL: none) in the place of buf[which], for either setter: the new table is on the device before the old
// one goes, and the old one goes only when nothing in flight reads it any more. A failed call leaves the old table in place.
int swap_table(ptmi_ctx *c, SceneBuf which, const float *table, uint32_t n, const char *what) {
    HIP_TRY(c, hipSetDevice(c->device));
    void *fresh = nullptr;
    if (table) {
        HIP_TRY(c, hipMalloc(&fresh, (size_t)n * sizeof(float)));
        const hipError_t e = hipMemcpy(fresh, table, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            dfree(fresh);
            return fail(c, PTMI_E_HIP, "%s table upload failed: %s (the previous table, if any, is still in place)", what, hipGetErrorString(e));
        }
    }
    const hipError_t e = sync_all(c);
    if (e != hipSuccess) {
        dfree(fresh);
        return fail(c, PTMI_E_HIP, "sync_all failed: %s", hipGetErrorString(e));
    }
    dfree(c->buf[which]);
    c->buf[which] = fresh;
    return PTMI_OK;
}

// what both probes do first: a scene, an active table, nothing in flight, room for n rays
int probe_begin(ptmi_ctx *c, uint32_t n) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!alpha_active(c))
        return fail(c, PTMI_E_STATE, "no alpha cutoff table with a positive entry (ptmi_set_alpha_cutoff) and no blend table with an entry >= 0 "
                                     "(ptmi_set_alpha_blend) in place");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    return ensure_capacity(c, c->lane, n);
}

int upload_rays(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *w, float4 *dO, float4 *dD) {
    std::vector<float4> o(n), d(n);
    for (uint32_t i = 0; i < n; i++) {
        o[i] = make_float4(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2], w ? w[i] : 0.0f);
        d[i] = make_float4(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2], 0.0f);
    }
    HIP_TRY(c, hipMemcpyAsync(dO, o.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dD, d.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, sync_all(c));
    return PTMI_OK;
}

}  // namespace

void pt_launch_alpha_resolve(hipStream_t s, int blocks, const DevScene &sc, DevAlpha a, uint32_t round, DevPaths p, const uint32_t *queue,
                             const uint32_t *count, float2 *hits, uint32_t *layers_out) {
    const bool first = round == 0u;
    const auto k = a.blend ? (first ? k_alpha_resolve<true, true> : k_alpha_resolve<false, true>)
                           : (first ? k_alpha_resolve<true, false> : k_alpha_resolve<false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(ABLOCK), 0, s, sc, a, round, p.O, p.D, queue, first ? count : &a.control[(round + 2u) % 3u],
                       hits, layers_out);
}

void pt_launch_alpha_shadow_resolve(hipStream_t s, int blocks, const DevScene &sc, DevAlpha a, uint32_t round, DevPaths p, DevShadow sh,
                                    const uint32_t *sq, const uint32_t *count, const float2 *hits0, uint8_t *occ_out, uint32_t *layers_out) {
    const bool first = round == 0u;
    const auto k = a.blend ? (first ? k_alpha_shadow_resolve<true, true> : k_alpha_shadow_resolve<false, true>)
                           : (first ? k_alpha_shadow_resolve<true, false> : k_alpha_shadow_resolve<false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(ABLOCK), 0, s, sc, a, round, p, sh, first ? sq : nullptr,
                       first ? count : &a.control[(round + 2u) % 3u], hits0, occ_out, layers_out);
}

PT_HOST {

// Rounds 0 .. max_layers of the resolve kernel with max_layers launches of `extend` between them: round r appends the rays that go on
// to list r & 1 under control word r % 3, `extend` traces exactly that list (queue = the list, count = the word, on the device) into the
// scratch hits, round r + 1 decides them. An empty list costs the launches and nothing else; no length ever comes back to the host.
void alpha_resolve_paths(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, const uint32_t *queue, const uint32_t *count,
                         float2 *hits, uint32_t *layers_out) {
    const DevAlpha a = dev_alpha(c);
    const int blocks = c->n_cu * 8;
    const DevPaths scratch{a.RO, a.RD, nullptr, nullptr};
    (void)hipMemsetAsync(a.control, 0, 3 * sizeof(uint32_t), s);
    for (uint32_t r = 0; r <= a.max_layers; r++) {
        pt_launch_alpha_resolve(s, blocks, c->sc, a, r, p, queue, count, hits, layers_out);
        if (r < a.max_layers) launch_extend(c, s, cfg, scratch, a.list[r & 1u], &a.control[r % 3u], a.hits);
    }
}

void alpha_shadow_stage(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, DevShadow sh, const uint32_t *sq,
                        const uint32_t *count, float2 *hits0, uint8_t *occ_out, uint32_t *layers_out) {
    const DevAlpha a = dev_alpha(c);
    const int blocks = c->n_cu * 8;
    const DevPaths records{sh.SO, sh.SD, nullptr, nullptr}, scratch{a.RO, a.RD, nullptr, nullptr};
    (void)hipMemsetAsync(a.control, 0, 3 * sizeof(uint32_t), s);
    launch_extend(c, s, cfg, records, sq, count, hits0);
    for (uint32_t r = 0; r <= a.max_layers; r++) {
        pt_launch_alpha_shadow_resolve(s, blocks, c->sc, a, r, p, sh, sq, count, hits0, occ_out, layers_out);
        if (r < a.max_layers) launch_extend(c, s, cfg, scratch, a.list[r & 1u], &a.control[r % 3u], a.hits);
    }
}

}  // namespace pt_host

int pt_check_alpha_cutoff(const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params, std::string &err) {
    uint32_t layers;
    return check_alpha(cutoff, n_materials, params, &layers, err);
}
int pt_check_alpha_blend(const float *factor, uint32_t n_materials, const ptmi_alpha_blend_params *params, std::string &err) {
    uint32_t layers;
    return check_blend(factor, n_materials, params, &layers, err);
}
uint32_t pt_ctx_materials(const ptmi_ctx *c) { return c->have_scene ? c->sc.n_mats : 0u; }
bool pt_ctx_has_scene(const ptmi_ctx *c) { return c->have_scene; }

extern "C" {

// Checked before anything changes, and the new table is on the device before the old one goes: a failed call leaves the table in place.
int ptmi_set_alpha_cutoff(ptmi_ctx *c, const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params) {
    if (!c) return PTMI_E_INVALID;
    if (!c->have_scene) return fail(c, PTMI_E_INVALID, "no scene uploaded: the table belongs to a scene's materials (ptmi_upload_scene)");
    const bool remove = !cutoff || n_materials == 0u;
    uint32_t layers = kDefaultLayers;
    int rc = check_alpha(remove ? nullptr : cutoff, n_materials, params, &layers, c->err);
    if (rc) return rc;
    if (!remove && n_materials != c->sc.n_mats)
        return fail(c, PTMI_E_INVALID, "n_materials %u is not the loaded scene's %u", n_materials, c->sc.n_mats);
    uint32_t n_cutout = 0u;
    for (uint32_t i = 0; !remove && i < n_materials; i++) n_cutout += cutoff[i] > 0.0f ? 1u : 0u;
    if ((rc = swap_table(c, kAlphaCutoff, remove ? nullptr : cutoff, n_materials, "cutoff"))) return rc;
    c->alpha_present = !remove;
    c->alpha_cutout = n_cutout;
    c->alpha_layers = remove ? 0u : layers;
    drop_idle_arrays(c);
    return PTMI_OK;
}

int ptmi_alpha_status(ptmi_ctx *c, struct ptmi_alpha_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    unsigned long long h[4];
    HIP_TRY(c, hipMemcpy(h, &c->d_counters[kCtAlphaPathPasses], sizeof h, hipMemcpyDeviceToHost));
    out->present = c->alpha_present ? 1u : 0u;
    out->n_materials = c->alpha_present ? c->sc.n_mats : 0u;
    out->n_cutout = c->alpha_cutout;
    out->max_layers = c->alpha_layers;
    out->path_passes = h[kCtAlphaPathPasses - kCtAlphaPathPasses]; out->path_exhausted = h[kCtAlphaPathExhausted - kCtAlphaPathPasses];
    out->shadow_passes = h[kCtAlphaShadowPasses - kCtAlphaPathPasses]; out->shadow_exhausted = h[kCtAlphaShadowExhausted - kCtAlphaPathPasses];
    return PTMI_OK;
}

// ptmi_set_alpha_cutoff's life cycle, clause by clause, for the blend table
int ptmi_set_alpha_blend(ptmi_ctx *c, const float *factor, uint32_t n_materials, const ptmi_alpha_blend_params *params) {
    if (!c) return PTMI_E_INVALID;
    if (!c->have_scene) return fail(c, PTMI_E_INVALID, "no scene uploaded: the table belongs to a scene's materials (ptmi_upload_scene)");
    const bool remove = !factor || n_materials == 0u;
    uint32_t layers = kDefaultLayers;
    int rc = check_blend(remove ? nullptr : factor, n_materials, params, &layers, c->err);
    if (rc) return rc;
    if (!remove && n_materials != c->sc.n_mats)
        return fail(c, PTMI_E_INVALID, "n_materials %u is not the loaded scene's %u", n_materials, c->sc.n_mats);
    uint32_t n_blend = 0u;
    for (uint32_t i = 0; !remove && i < n_materials; i++) n_blend += factor[i] >= 0.0f ? 1u : 0u;
    if ((rc = swap_table(c, kAlphaBlend, remove ? nullptr : factor, n_materials, "blend"))) return rc;
    c->blend_present = !remove;
    c->blend_count = n_blend;
    c->blend_layers = remove ? 0u : layers;
    c->blend_seed = !remove && params ? params->seed : 0u;
    drop_idle_arrays(c);
    return PTMI_OK;
}

int ptmi_alpha_blend_status(ptmi_ctx *c, struct ptmi_alpha_blend_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    unsigned long long h[4];
    HIP_TRY(c, hipMemcpy(h, &c->d_counters[kCtBlendPathTests], sizeof h, hipMemcpyDeviceToHost));
    out->present = c->blend_present ? 1u : 0u;
    out->n_materials = c->blend_present ? c->sc.n_mats : 0u;
    out->n_blend = c->blend_count;
    out->max_layers = c->blend_layers;
    out->seed = c->blend_seed;
    out->path_tests = h[0]; out->path_passes = h[kCtBlendPathPasses - kCtBlendPathTests];
    out->shadow_tests = h[kCtBlendShadowTests - kCtBlendPathTests]; out->shadow_passes = h[kCtBlendShadowPasses - kCtBlendPathTests];
    return PTMI_OK;
}

int ptmi_debug_alpha_intersect(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, float *t, uint32_t *tri, uint32_t *layers) {
    if (!c) return PTMI_E_INVALID;
    if (!o3 || !d3 || !t || !tri || !layers) return fail(c, PTMI_E_INVALID, "NULL argument");
    int rc = probe_begin(c, n);
    if (rc || n == 0) return rc;
    Lane &ln = c->lane;
    if ((rc = upload_rays(c, n, o3, d3, nullptr, ln.paths.O, ln.paths.D))) return rc;
    HIP_TRY(c, hipMemcpyAsync(&c->d_control[kCwQueue], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg;
    if ((rc = traverse_ready(c, true, cfg))) return rc;
    uint32_t *const d_layers = ln.queue[0];                 // (no queue is in use: slot i is ray i)
    launch_extend(c, c->stream, cfg, ln.paths, nullptr, &c->d_control[kCwQueue], ln.hits);
    alpha_resolve_paths(c, c->stream, cfg, ln.paths, nullptr, &c->d_control[kCwQueue], ln.hits, d_layers);
    std::vector<float2> h(n);
    HIP_TRY(c, hipMemcpyAsync(h.data(), ln.hits, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(layers, d_layers, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipGetLastError());
    for (uint32_t i = 0; i < n; i++) { t[i] = h[i].x; std::memcpy(&tri[i], &h[i].y, 4); }
    return PTMI_OK;
}

int ptmi_debug_alpha_occluded(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *dist, uint8_t *occ, uint32_t *layers) {
    if (!c) return PTMI_E_INVALID;
    if (!o3 || !d3 || !dist || !occ || !layers) return fail(c, PTMI_E_INVALID, "NULL argument");
    int rc = probe_begin(c, n);
    if (rc || n == 0) return rc;
    Lane &ln = c->lane;
    {   // every negative distance means "directional light" and travels as -1, as in ptmi_debug_occluded
        std::vector<float> dn(dist, dist + n);
        for (float &x : dn) if (x < 0.0f) x = -1.0f;
        rc = upload_rays(c, n, o3, d3, dn.data(), ln.sh[0].SO, ln.sh[0].SD);
    }
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(&c->d_control[kCwQueue], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg;
    if ((rc = traverse_ready(c, true, cfg))) return rc;
    uint32_t *const d_layers = ln.queue[0];
    alpha_shadow_stage(c, c->stream, cfg, ln.paths, ln.sh[0], nullptr, &c->d_control[kCwQueue], ln.hits, ln.d_occ, d_layers);
    HIP_TRY(c, hipMemcpyAsync(occ, ln.d_occ, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(layers, d_layers, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
