// pt_device.h — device-side data layout of the wavefront path tracer and the
// kernel launch interface shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include "ptmi_layout.h"
#include "ptmi.h"

#define PT_HD __host__ __device__ inline

// ---- traversal image of the scene (built at upload from the 48-B reference nodes) ----
// Wide node, 64 B = 4 x float4: both children's boxes live in the parent, so one
// fetch decides both subtrees.
//   q0 = (Lmin.x, Lmin.y, Lmin.z, Lmax.x)
//   q1 = (Lmax.y, Lmax.z, Rmin.x, Rmin.y)
//   q2 = (Rmin.z, Rmax.x, Rmax.y, Rmax.z)
//   q3 = bits(Lref, Rref, 0, 0)
// Child reference: internal -> index of its wide node; leaf -> PT_REF_LEAF |
// (count-1) << 26 | first triangle. Triangle image: 3 x float4 (v0, e1 = v1-v0,
// e2 = v2-v0), the only triangle data the intersection test reads (pt.wgsl:128-156).
#define PT_REF_LEAF      0x80000000u
#define PT_REF_NONE      0xFFFFFFFFu
#define PT_LEAF_MAX_TRIS 32u
#define PT_LEAF_OFF_BITS 26u
#define PT_LEAF_OFF_MASK ((1u << PT_LEAF_OFF_BITS) - 1u)

// The environment map (ptmi_upload_environment; pt_env.h has the functions that read it). tab NULL: none uploaded.
struct DevEnv {
    const float4 *tab;          // per texel (r, g, b, c): the radiance and c = P_t N / (2 pi^2), the texel's density over (u, v)
    const uint2 *alias;         // per entry (bits(prob), alias): the alias table over the w * h texels (NULL: never sampled)
    uint32_t w, h;
    uint32_t sampled;           // 1: next-event estimation picks it as light number n_lights, and bounce rays carry an MIS weight
    float intensity, rotation;  // radiance scale; radians about +Y added to the azimuth
};

// The participating medium (ptmi_set_medium; pt_medium.h has the functions that read it). on 0: none in place.
struct DevMedium {
    float sigma_t, g;           // extinction per unit length; Henyey-Greenstein asymmetry
    float albedo[3];            // single-scattering albedo per channel
    float box_min[3], box_max[3];
    uint32_t on;
    // the density grid (ptmi_upload_medium_density; grid NULL: none, the medium is homogeneous): nx * ny * nz multipliers in [0, 1] of
    // sigma_t stretched over the box, x fastest; filter 0 nearest, 1 trilinear over cell centres
    uint32_t filter;
    const float *grid;
    uint32_t nx, ny, nz;
};

struct DevScene;
struct DevScene {
    const ptmi_triangle *tris;  uint32_t n_tris;
    const ptmi_material *mats;  uint32_t n_mats;
    const ptmi_light *lights;   uint32_t n_lights;
    const void *atlas;          uint32_t atlas_w, atlas_h, atlas_fmt;   // 0 none, 1 rgba16f, 2 rgba32f
    const float4 *wnodes;       uint32_t n_wnodes;     // the hierarchy the kernels walk
    const float4 *tripos;
    float root_min[3], root_max[3];
    uint32_t root_ref;          // PT_REF_NONE: empty scene
    // When the reference tree is nested (every node box contains its children) the walked hierarchy is a
    // SAH tree rebuilt over the reference's leaves (fast_tree.hip, has_fast = 1) and the reference-shaped
    // image is kept for irregular rays; otherwise wnodes IS the reference-shaped image.
    const float4 *ref_wnodes;   uint32_t ref_root_ref, has_fast;
    // Quantised image of the rebuilt hierarchy for the global traversal variant (traverse.hip QuantMem; NULL: none):
    // 32-B nodes whose child boxes are 16-bit plane numbers on the grid origin + k * scale per axis, and the leaf stream
    // (per leaf: exact box + first triangle + count, then 9 dwords per triangle).
    const uint4 *qnodes;        const uint32_t *leaf_stream;
    float q_origin[3], q_scale[3];
    // |dx| + |dy| + |dz| of a ray up to which |e1 . (d x e2)| <= 2^100 for every triangle (2^98 / longest edge squared; 0 when an
    // edge is not finite): such rays take the triangle test whose short reciprocal has no range test (pt_math.h)
    float tri_safe_dsum;
    uint32_t q_cached;          // the first q_cached quantised nodes are the top levels in breadth-first order (kept in LDS)
    // OWN LEAVES (ptmi_options.leaves = 2, traverse_own.hip; own = 0: none of this is set). wnodes / tripos / qnodes / root_min / root_max
    // then describe the library's own hierarchy over the triangles: padded boxes, tripos in LEAF order with the original triangle
    // index in v0.w, n_own_tris entries; qnodes without a leaf stream. The tree as uploaded stays in ref_wnodes (its exact root box
    // in ref_root_min / _max) with the triangle images in ORIGINAL order in ref_tripos: what `slow` rays walk.
    uint32_t own, n_own_tris;
    const float4 *ref_tripos;
    const float4 *tri_leafbox;  // per ORIGINAL triangle index: (min.xyz, 0), (max.xyz, 0) of the reference leaf that lists it
    float ref_root_min[3], ref_root_max[3];
    float safe_origin;          // |o|_inf up to which the boxes' padding covers the rounding of the fused slab test
    // compact references (scenes of up to 4 096 triangles, NULL otherwise): copies of wnodes / ref_wnodes whose child references are 16 bits —
    // an internal node's index, or 0x8000 | (count - 1) << 12 | first triangle — for the kernels with 16-bit stack entries
    const float4 *wnodes16, *ref_wnodes16;
    uint32_t root_ref16, ref_root_ref16;
    const uint4 *qnodes16;      // qnodes with the same 16-bit references (NULL: none)
    unsigned long long *verify_stat;    // the word kCtVerifyFailed: += rays whose winner failed its reference leaf's box and were traced again
    const DevScene *self;       // this description in device memory (the own-leaf kernels read it from there, not from kernel arguments)
    const float4 *shade_tab;    // the shade tables (below): what `shade` stages into LDS
    DevEnv env;                 // the environment map behind every miss (tab NULL: none, a miss adds throughput * 0)
    DevMedium med;              // the medium inside a box (on 0: none, every segment travels through vacuum), with or without a density grid
};

// ---- shade tables: the records `shade` reads per hit that are the same for the whole scene, in one blob built at upload ----
// In float4 (16 B) units, all raw copies of the uploaded bytes:
//   [0, 8 (n_mats + 1))         the materials, 8 each, then one material of zeros: what a material index >= n_mats reads
//   [.., + 3 n_lights)          the lights, 3 each
//   [.., + 8 n_lights)          per light, at the light's own index, the triangle an emissive light names (zeros for the other types
//                               and for a triangle index >= n_tris), so that it is found without reading triangle_index first
// k_shade copies the materials, the lights (with their triangles) or both into LDS when they fit PT_SHADE_LDS_BUDGET and reads them
// from there; a table that does not fit is read from DevScene::mats / lights / tris as before (pt_shade_stage: chosen per launch).
#define PT_SHADE_LDS_BUDGET 16384u      /* bytes of LDS per 256-thread workgroup of k_shade */
enum { PT_STAGE_MATS = 1, PT_STAGE_LIGHTS = 2 };
PT_HD size_t pt_tab_mats_q(uint32_t n_mats) { return ((size_t)n_mats + 1u) * 8u; }
PT_HD size_t pt_tab_lights_q(uint32_t n_lights) { return (size_t)n_lights * 11u; }
// which tables a launch stages: both if they fit together, else the materials (every hit reads one) if they fit, else the lights
PT_HD int pt_shade_stage(uint32_t n_mats, uint32_t n_lights) {
    const size_t m = pt_tab_mats_q(n_mats) * 16u, l = pt_tab_lights_q(n_lights) * 16u;
    if (m + l <= PT_SHADE_LDS_BUDGET) return PT_STAGE_MATS | (n_lights ? PT_STAGE_LIGHTS : 0);
    if (m <= PT_SHADE_LDS_BUDGET) return PT_STAGE_MATS;
    return l <= PT_SHADE_LDS_BUDGET && n_lights ? PT_STAGE_LIGHTS : 0;
}

// ---- path state: 56 B per path, four streams indexed by path id (O / D / C: by queue slot after the repack, ShadeParams) ----
//   O = (origin.xyz, bits(rng state))   D = (direction.xyz, throughput.x)      the two float4 `extend` reads
//   C = (throughput.y, throughput.z)    L = (radiance.xyz, 0)
// and, only while a sampled environment is in place, W: the MIS weight of the environment's radiance should this ray miss (4 B).
// Radiance L and the contribution SC of a shadow record have three lanes and are stored as three floats.
// SC (read and written in queue-slot order) sits at 12-byte stride. L is read-modify-written by path id, scattered, and its
// stride is chosen per dispatch (DevPaths::l_stride, in floats): 3 where the scene lives in LDS, 4 where the traversal
// kernels walk it from memory and every extra line the RMW straddles competes with node fetches. Measured, interleaved runs,
// Msamples/s (both 16 B / both 12 B / L 16 + SC 12 / L 12 + SC 16): config 1 8 907 / 9 172 / 9 031 / 9 133; config 3
// 4 742 / 4 524 / 4 734 / 4 482.
struct rgb_sc { float x, y, z; };
struct DevPaths {
    float4 *O, *D; float2 *C; float *L; uint32_t l_stride = 3;
    float *W = nullptr;         // NULL while no environment is sampled (a miss then takes the weight 1)
    // stride 4 means whole 16-byte accesses (a 12-byte access is issued as two requests: with stride 4 and 12-byte accesses
    // raygen's store of L takes 1.9 instead of 1.1 ms per 64 spp, and config 3 loses the same 5 % as with stride 3)
    __device__ __forceinline__ rgb_sc ldL(uint32_t p) const {
        if (l_stride == 4u) { const float4 v = reinterpret_cast<const float4 *>(L)[p]; return rgb_sc{v.x, v.y, v.z}; }
        return reinterpret_cast<const rgb_sc *>(L)[p];
    }
    __device__ __forceinline__ void stL(uint32_t p, float x, float y, float z) const {
        if (l_stride == 4u) reinterpret_cast<float4 *>(L)[p] = make_float4(x, y, z, 0.0f);
        else reinterpret_cast<rgb_sc *>(L)[p] = rgb_sc{x, y, z};
    }
};
// hit record, 8 B per queue slot: (t, bits(triangle index)); t = -1 on a miss. `shade` rebuilds (u, v) from the triangle.
// shadow record, 44 B per queue slot (`shade` packs a wave's records at the front of its 64 slots):
//   SO = (origin.xyz, dist or -1 for directional)  SD = (wi.xyz, bits(path id))
//   SC = throughput * directLight .xyz (12-byte stride)   added to L[path] when unoccluded
// One allocation per bounce parity: SO at the base, SD `cap` float4 further, SC after both (the shadow kernel carries only the
// base and cap: two pointers fewer in scalar registers, see traverse.hip ShadowIO)
struct DevShadow { float4 *SO, *SD; rgb_sc *SC; uint32_t cap; };   // 44 B per queue slot

// The rows one context renders: [y0, y1) of a width x height frame, or — when parts > 1 — every parts-th strip
// of `strip` rows inside that range, starting with strip number `part` (row bands interleaved across GPUs so each
// sees a sample of the whole picture). rows = how many rows that is; local row l is frame row row_of(l).
struct DevBand {
    uint32_t width, height, y0, y1, strip, parts, part, rows;
    PT_HD uint32_t row_of(uint32_t l) const {
        if (parts <= 1u) return y0 + l;
        return y0 + ((l / strip) * parts + part) * strip + l % strip;
    }
    // whether frame row y is one of the band's
    PT_HD bool has_row(uint32_t y) const {
        if (y < y0 || y >= y1) return false;
        return parts <= 1u || ((y - y0) / strip) % parts == part;
    }
    // band-local pixel (local row * width + x) -> its index in the width x height frame
    PT_HD size_t frame_pixel(uint32_t pix) const { return (size_t)row_of(pix / width) * width + pix % width; }
};

// Russian roulette (pt.wgsl:699-705) from this bounce on. The first such bounce is also where the batch's path state is repacked:
// after its compaction, O / D / C of the survivors are gathered into tail arrays at their queue positions (pt_launch_repack), and
// from the next bounce on the state stays at the slot the queue names, its path id beside it (ShadeParams::pid).
PT_HD bool pt_plays_roulette(uint32_t bounce) { return bounce > 2u; }
inline uint32_t pt_repack_bounce() { uint32_t b = 0; while (!pt_plays_roulette(b)) b++; return b; }

// ---- counter and control words: the two small blocks of a context that kernels and host code share by word ----
// Both are made and zeroed by ptmi_create and live as long as the context. Kernels get the block's base (ShadeParams::stats,
// DevAdaptive::counters / control, ReprojectArgs::status) or the address of one word (DevScene::verify_stat, queue lengths).
constexpr int kMaxBounces = 64;         // ptmi_options.max_bounces' upper limit (ptmi_set_options)
// u64 counters, added to with atomics. [kCtSegments, kCtDispatchEnd) is what ptmi_reset_stats zeroes.
enum CounterWord {
    kCtSegments,                        // path segments (k_tile_sums: the queue length of every bounce)
    kCtShadowRays,                      // records `shade` left (k_tile_sums) + next-event samples counted but not traced (k_shade)
    kCtShadowTraced,                    // records `shade` left
    kCtEmitRecords,                     // ... of which records of emissive hits: no shadow rays, ptmi_get_stats takes them off both
    kCtVerifyFailed,                    // own leaves: rays traced again (DevScene::verify_stat)
    kCtAdTraced,                        // paths of adaptive dispatches (ptmi_stats.paths)
    kCtByBounce,                        // kMaxBounces words: segments of bounce b
    kCtDispatchEnd = kCtByBounce + kMaxBounces,
    kCtAdSum = kCtDispatchEnd, kCtAdMin, kCtAdMax,                      // ptmi_adaptive_status: the band's counts (preset 0, ~0, 0 per call)
    kCtRpCarried, kCtRpDisoccluded, kCtRpMissed, kCtRpSamples,          // ptmi_reproject_status: the last ptmi_reproject
    kCounterWords
};
// u32 control words: lengths that one kernel writes and the next reads
enum ControlWord {
    kCwQueue,                           // kMaxBounces + 1 words: the queue length of bounce b (the last bounce writes that of the next)
    kCwShadow = kCwQueue + kMaxBounces + 1,     // 2 words: the shadow queue's length, by bounce parity (overlap)
    kCwAdPixels = kCwShadow + 2,        // adaptive round: the band's pixels
    kCwAdActive,                        // ... and how many of them the round lists
    kControlWords
};
// no two names share a word: every name or run of words starts where the one before it ends, and the last ends the block
constexpr bool pt_words_disjoint(std::initializer_list<int> first_then_length, int total) {
    int at = 0;
    for (const int *p = first_then_length.begin(); p != first_then_length.end(); p += 2) {
        if (p[0] != at) return false;
        at += p[1];
    }
    return at == total;
}
static_assert(pt_words_disjoint({kCtSegments, 1, kCtShadowRays, 1, kCtShadowTraced, 1, kCtEmitRecords, 1, kCtVerifyFailed, 1, kCtAdTraced, 1,
                                 kCtByBounce, kMaxBounces, kCtAdSum, 1, kCtAdMin, 1, kCtAdMax, 1,
                                 kCtRpCarried, 1, kCtRpDisoccluded, 1, kCtRpMissed, 1, kCtRpSamples, 1}, kCounterWords),
              "a counter word has two names, or none");
static_assert(pt_words_disjoint({kCwQueue, kMaxBounces + 1, kCwShadow, 2, kCwAdPixels, 1, kCwAdActive, 1}, kControlWords),
              "a control word has two names, or none");
static_assert(kCtDispatchEnd - kCtByBounce == 64 && sizeof(ptmi_stats::segments_by_bounce) == 64 * sizeof(uint64_t),
              "a word per bounce up to max_bounces' limit, as ptmi_stats reports them");
static_assert(kCwShadow - kCwQueue == 64 + 1, "bounce b reads queue length b and writes b + 1, for b < 64");
static_assert(kCtAdTraced < kCtDispatchEnd && kCtAdSum >= kCtDispatchEnd && kCtRpCarried >= kCtDispatchEnd,
              "ptmi_reset_stats zeroes the dispatch statistics and the adaptive traced count, nothing else");
static_assert(kCtAdMin == kCtAdSum + 1 && kCtAdMax == kCtAdSum + 2, "ptmi_adaptive_status presets and reads the three with one copy each");
static_assert(kCtRpDisoccluded == kCtRpCarried + 1 && kCtRpMissed == kCtRpCarried + 2 && kCtRpSamples == kCtRpCarried + 3,
              "ptmi_reproject zeroes the four with one memset, ptmi_reproject_status reads them with one copy");

struct ShadeParams {
    uint32_t bounce, max_bounces, do_mis;
    unsigned long long *stats;          // the counter block: [kCtShadowRays] += next-event samples counted but not traced (zero contribution)
    uint32_t emit_records;              // 1: an emissive hit does not add to L here; it leaves a record (SO.w = -2: nothing to trace)
                                        //    that `shadow` adds like an unoccluded light sample — all additions to L then happen in
                                        //    that one kernel, in bounce order, and `shadow` can run beside the next bounce's kernels.
                                        //    stats[kCtEmitRecords] += such records (they are not shadow rays)
    const uint32_t *pid;                // path id of a state slot after the repack (NULL: the slot is the path id)
};

enum { PT_VARIANT_GLOBAL = 1, PT_VARIANT_LDS = 2, PT_VARIANT_LDS_NODES = 3,
       // own leaves (traverse_own.hip): exact / quantised nodes in LDS, with (…_LDS) or without (…_NODES) the triangle images, or from memory
       PT_VARIANT_OWN_LDS = 4, PT_VARIANT_OWN_LDS_NODES = 5, PT_VARIANT_OWN_QLDS = 6, PT_VARIANT_OWN_QLDS_NODES = 7,
       PT_VARIANT_OWN_QGLOBAL = 8, PT_VARIANT_OWN_GLOBAL = 9,
       PT_VARIANT_OWN_LDS16_NODES = 10,         // exact nodes with 16-bit references and 16-bit stack entries (scenes up to 4 096 triangles)
       PT_VARIANT_OWN_QLDS16_NODES = 11,        // quantised nodes with 16-bit references: two workgroups per CU for trees of up to 2 046 nodes,
                                                // 8 - 15 16-bit entries per lane (what the nodes leave of 80 KB), the node stack spills
       PT_VARIANT_COUNT };

// What each traversal variant is: one row per PT_VARIANT_* (pt_variant), the one place selection (traverse_pick.hip traverse_config) and
// the launches read it from.
enum PtNodes {                  // node format
    PT_NODES_EXACT,             // 64-B wide nodes (PT_VARIANT_GLOBAL: or the quantised image, TraverseConfig::quantized)
    PT_NODES_QUANT,             // 32-B quantised nodes
    PT_NODES_EXACT16,           // exact nodes with 16-bit (compact) references
    PT_NODES_QUANT16 };         // quantised nodes with 16-bit references
enum PtWhere {                  // what is resident in LDS
    PT_LDS_ALL,                 // the nodes and the triangle images
    PT_LDS_NODES,               // the nodes; triangles through L1 / L2
    PT_FROM_MEMORY };           // nothing: walks the scene from memory (a quantised image keeps its top levels in LDS)
enum PtStack {                  // per-lane stack entries in LDS
    PT_STACK_DEPTH,             // 16 or 32 by tree depth, none spill; one workgroup per CU
    PT_STACK_NODES,             // two workgroups per CU: 15 (the tree's whole node stack); one: 16, the rest spills
    PT_STACK_SPILL,             // 16, the rest spills; the grid is as many workgroups as are resident
    PT_STACK_16BIT,             // 15 16-bit entries (the tree's whole node stack); two workgroups per CU
    PT_STACK_16BIT_SPILL };     // 8 - 15 16-bit entries, what the nodes leave; the rest spills; two workgroups per CU
struct PtVariant { PtNodes nodes; PtWhere where; PtStack stack; bool own; };
constexpr PtVariant kPtVariants[PT_VARIANT_COUNT] = {
    {},                                                                 // (0: none)
    {PT_NODES_EXACT,   PT_FROM_MEMORY, PT_STACK_SPILL,       false},    // PT_VARIANT_GLOBAL
    {PT_NODES_EXACT,   PT_LDS_ALL,     PT_STACK_DEPTH,       false},    // PT_VARIANT_LDS
    {PT_NODES_EXACT,   PT_LDS_NODES,   PT_STACK_NODES,       false},    // PT_VARIANT_LDS_NODES
    {PT_NODES_EXACT,   PT_LDS_ALL,     PT_STACK_DEPTH,       true},     // PT_VARIANT_OWN_LDS
    {PT_NODES_EXACT,   PT_LDS_NODES,   PT_STACK_NODES,       true},     // PT_VARIANT_OWN_LDS_NODES
    {PT_NODES_QUANT,   PT_LDS_ALL,     PT_STACK_DEPTH,       true},     // PT_VARIANT_OWN_QLDS
    {PT_NODES_QUANT,   PT_LDS_NODES,   PT_STACK_NODES,       true},     // PT_VARIANT_OWN_QLDS_NODES
    {PT_NODES_QUANT,   PT_FROM_MEMORY, PT_STACK_SPILL,       true},     // PT_VARIANT_OWN_QGLOBAL
    {PT_NODES_EXACT,   PT_FROM_MEMORY, PT_STACK_SPILL,       true},     // PT_VARIANT_OWN_GLOBAL
    {PT_NODES_EXACT16, PT_LDS_NODES,   PT_STACK_16BIT,       true},     // PT_VARIANT_OWN_LDS16_NODES
    {PT_NODES_QUANT16, PT_LDS_NODES,   PT_STACK_16BIT_SPILL, true},     // PT_VARIANT_OWN_QLDS16_NODES
};
inline const PtVariant &pt_variant(int v) { return kPtVariants[v > 0 && v < PT_VARIANT_COUNT ? v : 0]; }
inline bool pt_quantised(const PtVariant &r) { return r.nodes == PT_NODES_QUANT || r.nodes == PT_NODES_QUANT16; }
// the stack spills (the caller supplies TraverseConfig::spill) with `wgs` workgroups per CU
inline bool pt_spills(const PtVariant &r, int wgs) {
    return r.stack == PT_STACK_SPILL || r.stack == PT_STACK_16BIT_SPILL || (r.stack == PT_STACK_NODES && wgs == 1);
}
// dynamic LDS of one 1024-thread workgroup: [nodes][triangle images][stack: `entries` per lane]; none for the kernels that walk memory
inline size_t pt_lds_bytes(const PtVariant &r, uint32_t n_nodes, uint32_t n_tris, int entries) {
    if (r.where == PT_FROM_MEMORY) return 0;
    const bool narrow = r.nodes == PT_NODES_EXACT16 || r.nodes == PT_NODES_QUANT16;
    return (size_t)n_nodes * (pt_quantised(r) ? 32 : 64) + (r.where == PT_LDS_ALL ? (size_t)n_tris * 48 : 0) +
           (size_t)entries * 1024 * (narrow ? sizeof(uint16_t) : sizeof(uint32_t));
}

struct TraverseConfig {
    int variant;            // PT_VARIANT_*
    int stack_entries;      // per lane: 15, 16 or 32 (PtStack); PT_VARIANT_OWN_QLDS16_NODES: 8 ... 15
    int cull;               // 0/1
    int wgs_per_cu;         // workgroups per CU of the LDS variants (PtStack). ptmi_stats reports variant * 10 + wgs_per_cu
                            // (pt_variant_code), and leaves = 1 reports PT_VARIANT_GLOBAL and PT_VARIANT_LDS with 2 here
    size_t lds_bytes;       // dynamic LDS per workgroup (pt_lds_bytes), set where the variant is chosen
    uint32_t *spill;        // per-lane overflow of the node stack, pt_spill_bytes(blocks) bytes
    int wants_spill;        // the variant needs one (the caller supplies `spill`: each concurrently running kernel its own)
    int quantized;          // the variant walks quantised nodes (PT_VARIANT_GLOBAL: the quantised image, when the scene has one)
};
inline uint32_t pt_variant_code(const TraverseConfig &cfg) { return (uint32_t)cfg.variant * 10u + (uint32_t)cfg.wgs_per_cu; }
#ifndef PT_QCACHE_NODES
#define PT_QCACHE_NODES 256      /* quantised nodes of the top levels staged in LDS per workgroup (8 KB) */
#endif
#define PT_SPILL_ENTRIES 64     /* >= the deepest node stack: upload rejects trees deeper than 62 */
size_t pt_spill_bytes(int blocks);

// ---- launchers (each enqueues on `s`; grids are persistent, sized by the caller) ----
// The pixels a batch walks, in ray generation and the three folds: every pixel of the band from frame `frame0` on (list == NULL:
// plain dispatch), or the *n_active band-local pixels of `list`, each from its own frame index mom[pixel].z (adaptive dispatch).
// n_frames frames of each: path k * entries + j is frame k of entry j.
struct DevPixels {
    DevBand band; uint32_t frame0;
    const uint32_t *list, *n_active; const float4 *mom;
    unsigned long long *traced;         // listed: the word kCtAdTraced, += the batch's paths (a plain dispatch counts its paths on the host)
};
// *count_out = entries * n_frames
void pt_launch_raygen(hipStream_t s, int blocks, const ptmi_camera &cam, DevPixels px, uint32_t n_frames, DevPaths p,
                      uint32_t *count_out);
void pt_launch_raygen_list(hipStream_t s, const ptmi_camera &cam, uint32_t n, const uint32_t *xs,
                           const uint32_t *ys, const uint32_t *frames, DevPaths p);
void pt_launch_extend(hipStream_t s, int blocks, const TraverseConfig &cfg, const DevScene &sc, DevPaths p,
                      const uint32_t *queue, const uint32_t *count, float2 *hits);
void pt_launch_extend_own(hipStream_t s, int blocks, const TraverseConfig &cfg, const DevScene &sc, DevPaths p,
                          const uint32_t *queue, const uint32_t *count, float2 *hits);        // traverse_own.hip
// (u, v) of n hit records, rebuilt the way `shade` does it (debug entry point of the parity tests)
void pt_launch_hit_uv(hipStream_t s, uint32_t n, const DevScene &sc, DevPaths p, const float2 *hits, float2 *uv);
// shadow_queue: positions of the shadow records to trace (NULL = slots 0..count-1), count = their number
void pt_launch_shadow(hipStream_t s, int blocks, const TraverseConfig &cfg, const DevScene &sc, DevPaths p,
                      DevShadow sh, const uint32_t *shadow_queue, const uint32_t *count, uint8_t *occluded_out);
void pt_launch_shadow_own(hipStream_t s, int blocks, const TraverseConfig &cfg, const DevScene &sc, DevPaths p,
                          DevShadow sh, const uint32_t *shadow_queue, const uint32_t *count, uint8_t *occluded_out);
void pt_launch_shade(hipStream_t s, int blocks, const DevScene &sc, DevPaths p, const uint32_t *queue,
                     const uint32_t *count, const float2 *hits, DevShadow sh, uint64_t *alive_mask,
                     uint64_t *shadow_mask, ShadeParams sp, float4 *aov = nullptr);
void pt_launch_shade_fast(hipStream_t s, int blocks, const DevScene &sc, DevPaths p, const uint32_t *queue,
                          const uint32_t *count, const float2 *hits, DevShadow sh, uint64_t *alive_mask,
                          uint64_t *shadow_mask, ShadeParams sp, float4 *aov = nullptr);   // perf mode: shade.hip built with fast division / sqrt
// (aov, bounce 0 only: 2 float4 per path of first-hit record, see shade.hip k_shade; NULL: none written)
// ordered stream compaction of the survivors: masks -> next queue + its count, plus statistics
// (tiles = ceil(capacity / pt_compact_tile_slots()) + 1: one workgroup per tile of ballot words)
uint32_t pt_compact_tile_slots(void);
// the repack: queue entry j (path id q, j < *count) -> to.O / D / C[j] = from.O / D / C[q] (W too, where there is one), pid[j] = q
void pt_launch_repack(hipStream_t s, int blocks, const uint32_t *count, const uint32_t *queue, DevPaths from, DevPaths to,
                      uint32_t *pid);
void pt_launch_compact(hipStream_t s, int tiles, const uint32_t *queue, const uint32_t *count,
                       const uint64_t *alive_mask, const uint64_t *shadow_mask, uint32_t *tile_sums,
                       uint32_t *next_queue, uint32_t *next_count, uint32_t *shadow_queue, uint32_t *shadow_count,
                       unsigned long long *stats, uint32_t bounce, int do_scatter);
// the three folds of a batch over its pixels (DevPixels), each pixel's frames in ascending order. Listed pixels read their frame index
// from mom.z, which the moments fold moves on: it goes last.
void pt_launch_accumulate(hipStream_t s, int blocks, DevPixels px, uint32_t n_frames, const float *L, uint32_t l_stride, float4 *out);
// the first-hit planes (ptmi_set_aovs) from the batch's bounce-0 records; a NULL plane is not written
void pt_launch_accumulate_aov(hipStream_t s, int blocks, DevPixels px, uint32_t n_frames, const float4 *rec,
                              const ptmi_triangle *tris, uint32_t n_tris, float4 *albedo, float4 *normal, uint2 *ids);
// the sample-moments plane (ptmi_set_moments) from the batch's per-path radiance; listed pixels: mom is px.mom
void pt_launch_accumulate_moments(hipStream_t s, int blocks, DevPixels px, uint32_t n_frames, const float *L, uint32_t l_stride,
                                  float4 *mom);
// adaptive sampling (ptmi_dispatch_adaptive; kernels in pipeline.hip): the context's buffers of a round
struct DevAdaptive {
    uint64_t *ballot;             // one word per 64 band pixels: bit set = the pixel gets frames this round
    uint32_t *list;               // ... as the ascending list of band-local pixel indices
    uint32_t *tile_sums;          // pt_adaptive_tiles(band pixels) words
    uint32_t *control;            // the context's control block: kCwAdPixels, kCwAdActive (the length of the list)
    unsigned long long *counters; // the context's counter block: kCtAdTraced, and kCtAdSum / Min / Max of the counts (status)
};
uint32_t pt_adaptive_tiles(uint32_t npix);
void pt_launch_adaptive_restart(hipStream_t s, int blocks, DevBand band, float4 *mom);          // every count of the band back to 0
// select + list build: ad.ballot, ad.list and the two control words of this round from the moments plane
void pt_launch_adaptive_list(hipStream_t s, int blocks, DevBand band, const ptmi_adaptive_params &ap, const float4 *mom, DevAdaptive ad);
// (ray generation and the folds of a round: pt_launch_raygen / pt_launch_accumulate* with the list as their DevPixels)
void pt_launch_adaptive_status(hipStream_t s, int blocks, DevBand band, const float4 *mom, DevAdaptive ad);
// Adaptive rounds over several devices (ptmi_multi_dispatch_adaptive with neighbourhood = 1): the NOISY flag of every pixel of the frame,
// one byte each, as the devices' shares one after the other. Share r holds the rows of part r (DevBand::row_of) of a frame dealt out
// from row 0, local row l at share_px * r + l * width: a device writes its own share and receives the others'.
struct DevFlagMap {
    const uint8_t *map;
    uint32_t share_px, width, strip, parts;
    PT_HD uint8_t at(uint32_t x, uint32_t y) const {
        if (parts <= 1u) return map[(size_t)y * width + x];
        const uint32_t s = y / strip;
        return map[(size_t)(s % parts) * share_px + (size_t)((s / parts) * strip + y % strip) * width + x];
    }
};
// flags[band-local pixel] = the pixel is NOISY (the rule of k_ad_select, per pixel)
void pt_launch_adaptive_flags(hipStream_t s, int blocks, DevBand band, const ptmi_adaptive_params &ap, const float4 *mom, uint8_t *flags);
// pt_launch_adaptive_list with the neighbourhood looked up in the whole-frame map instead of the band's own moments
void pt_launch_adaptive_list_map(hipStream_t s, int blocks, DevBand band, const ptmi_adaptive_params &ap, const float4 *mom, DevFlagMap fm,
                                 DevAdaptive ad);
// the denoiser (denoise.hip, ptmi_denoise): a prepass into guide / grad / cv, then `iterations` a-trous passes ping-ponging between
// cv and tmp, the last remodulating into out. albedo NULL: no demodulation. cv is overwritten.
struct DenoiseArgs {
    uint32_t W, H, iterations;
    float phi_color, phi_normal, phi_depth;
};
void pt_launch_denoise(hipStream_t s, const DenoiseArgs &a, const float4 *radiance, const float4 *normal, const float4 *albedo,
                       const float4 *moments, float4 *guide, float *grad, float4 *cv, float4 *tmp, float4 *out);
// reprojection (reproject.hip, ptmi_reproject; the contract is stated in include/ptmi.h). The centre rays of the band's pixels under
// `cam` go to p.O / p.D at the band-local pixel index, *count_out = their number: what `extend` then traces with a null queue.
void pt_launch_center_rays(hipStream_t s, int blocks, const ptmi_camera &cam, DevBand band, DevPaths p, uint32_t *count_out);
struct ReprojectArgs {
    ptmi_camera from;
    DevBand band;
    uint32_t max_history, match_ids;    // match_ids: 0 / 1, resolved
    float depth_tolerance;
    const float4 *O, *D; const float2 *hits;            // the centre rays of `to` and their closest hits, by band-local pixel
    const ptmi_triangle *tris; uint32_t n_tris;
    const float4 *h_out, *h_mom, *h_normal, *h_albedo; const uint2 *h_ids;   // the snapshot (albedo / ids NULL: that plane is off)
    float4 *out, *mom, *normal, *albedo; uint2 *ids;    // the live planes, rewritten
    unsigned long long *status;                         // the counter block: kCtRpCarried, ...Disoccluded, ...Missed, ...Samples +=
};
void pt_launch_reproject(hipStream_t s, const ReprojectArgs &a);
void pt_launch_blit(hipStream_t s, int blocks, uint32_t W, uint32_t H, const float4 *color, float4 *out_f32,
                    uint32_t *out_rgba8);
// a device's rows of the frame <-> a contiguous buffer (ptmi_multi_gather)
void pt_launch_pack_rows(hipStream_t s, int blocks, DevBand band, const float4 *frame, float4 *packed);
void pt_launch_unpack_rows(hipStream_t s, int blocks, DevBand band, const float4 *packed, float4 *frame);
// Several planes of a device's rows <-> one contiguous share (ptmi_multi_gather_planes). A share is laid out plane after plane, each
// share_px = rows_max x width entries (the largest band's; a smaller band leaves padding that is never unpacked): first the n4 planes of
// 16-byte entries in the order of f4[], then the 8-byte ids. A frame plane that is absent from the set is NULL / not counted.
struct DevPlaneSet {
    float4 *f4[4];
    uint2 *ids;
    uint32_t n4, share_px;
    PT_HD size_t share_bytes() const { return ((size_t)share_px * (n4 * 16u + (ids ? 8u : 0u)) + 15u) & ~(size_t)15u; }
};
// band's rows of every plane of the set -> share
void pt_launch_pack_planes(hipStream_t s, int blocks, DevBand band, DevPlaneSet set, float4 *share);
// recv = `parts` shares, share_bytes apart, share r from the device of part r -> the frame planes of the set, every row of the frame
// except those of part `skip` (0xFFFFFFFF: none). band: any device's (its part is not read).
void pt_launch_unpack_planes(hipStream_t s, int blocks, DevBand band, DevPlaneSet set, const float4 *recv, uint32_t skip);
// the rows DevBand describes for a context with these options on a width x height frame (rows = 0: none)
struct ptmi_options;
DevBand pt_band_of(const ptmi_options &opt, uint32_t width, uint32_t height);
void pt_launch_exact_math(hipStream_t s, int which, unsigned long long *out);
void pt_launch_math(hipStream_t s, int op, uint32_t n, const float *a, const float *b, const float *c, float *out);

