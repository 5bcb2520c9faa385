// traverse_pick.hip — which memory variant a traversal kernel runs as on the uploaded scene (pt_device.h pt_variant), and what every
// caller does between that choice and the launch: the refusal of a scene that does not fit, the spill area, the statistic.
#include "ptmi_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <iterator>
#include <utility>

namespace {

constexpr size_t kLdsMax = 160 * 1024;

// bytes of the walked image in LDS (nodes and triangle images)
size_t lds_scene_bytes(const ptmi_ctx *c) { return (size_t)c->img.n_wnodes * 64 + (size_t)c->img.n_tris * 48; }

// Sizes `variant` (pt_variant) on the uploaded scene with `wgs` workgroups per CU: the per-lane stack, whether it spills, the LDS it
// launches with. False: it does not fit, or the scene has no image in its node format.
bool size_variant(const ptmi_ctx *c, int variant, int wgs, TraverseConfig &cfg) {
    const PtVariant &r = pt_variant(variant);
    const uint32_t depth = std::max(c->img.depth, c->img.ref_depth);    // slow rays walk the uploaded tree on the same stacks
    int entries = 0;
    bool ok = true;
    switch (r.stack) {
    case PT_STACK_DEPTH: entries = depth + 2 <= 16 ? 16 : depth + 2 <= 32 ? 32 : 0; ok = wgs == 1 && entries != 0; break;
    case PT_STACK_NODES: entries = wgs == 2 ? 15 : 16; ok = wgs == 1 || (wgs == 2 && depth + 1 <= 15); break;
    case PT_STACK_SPILL: entries = 16; ok = wgs == 1; break;
    case PT_STACK_16BIT: entries = 15; ok = wgs == 2 && depth + 1 <= 15; break;
    case PT_STACK_16BIT_SPILL: {
        // the 16-bit entries (2 KB each per workgroup) take what the quantised nodes leave of a CU's half
        const size_t nq = (size_t)c->sc.n_wnodes * 32;
        entries = (c->sc.qnodes16 && nq + 64 < kLdsMax / 2) ? std::min<int>(15, (int)((kLdsMax / 2 - 64 - nq) / 2048)) : 0;
        if (const char *e = std::getenv("PTMI_OWN_Q16_ENTRIES"))      // tests: a shorter stack than fits (more spills), never below 8
            entries = std::min(entries, std::max(8, std::atoi(e)));
        ok = wgs == 2 && entries >= 8;
        break;
    }
    }
    ok = ok && (!pt_quantised(r) || (c->sc.own && c->img.quantised)) && (r.nodes != PT_NODES_EXACT16 || c->sc.wnodes16 != nullptr);
    cfg.variant = variant; cfg.wgs_per_cu = wgs; cfg.stack_entries = entries;
    cfg.wants_spill = pt_spills(r, wgs) ? 1 : 0;
    cfg.quantized = pt_quantised(r) ? 1 : 0;
    cfg.lds_bytes = pt_lds_bytes(r, c->sc.n_wnodes, c->sc.own ? c->sc.n_own_tris : c->sc.n_tris, entries);
    return ok && cfg.lds_bytes <= kLdsMax / (size_t)wgs;
}

// Which memory variant a traversal kernel runs as (closest_hit: the extend kernel, else the any-hit kernel). PTMI_OWN_EXTEND /
// PTMI_OWN_SHADOW (a code as ptmi_stats reports it, pt_variant_code: 102 = PT_VARIANT_OWN_LDS16_NODES, two workgroups per CU) override
// the choice of the own-leaf variants where it fits — for same-box A/Bs, not for users.
TraverseConfig traverse_config(const ptmi_ctx *c, bool closest_hit) {
    const bool own = c->sc.own, big = lds_scene_bytes(c) > ((size_t)4 << 20);       // big: beyond an XCD's L2
    const int traversal = c->opt.traversal;
    TraverseConfig cfg{};
    cfg.cull = c->opt.cull ? 1 : 0;
    auto pick = [&](int variant, int wgs) { return size_variant(c, variant, wgs, cfg); };
    // The quantised image pays where node fetches leave the L2 (measured: the 1 M-triangle scene, 67 MB, extend -16 %); a scene
    // that an XCD's 4 MiB L2 holds is bound by the ALUs, and decoding costs more than the bytes save (cornell_spheres walked
    // from global memory: shadow +30 %). AUTO decides by size; GLOBAL asks for the quantised image, GLOBAL_EXACT for the exact one.
    const bool mem_quant = traversal == PTMI_TRAVERSAL_GLOBAL || (traversal == PTMI_TRAVERSAL_AUTO && big);
    auto from_memory = [&]() {
        if (!own) { pick(PT_VARIANT_GLOBAL, 1); cfg.quantized = mem_quant; cfg.wgs_per_cu = 2; }  // (2: the code leaves = 1 has always reported)
        else pick(c->img.quantised && mem_quant ? PT_VARIANT_OWN_QGLOBAL : PT_VARIANT_OWN_GLOBAL, 1);
        return cfg;
    };
    if (traversal == PTMI_TRAVERSAL_GLOBAL || traversal == PTMI_TRAVERSAL_GLOBAL_EXACT) return from_memory();
    if (own && traversal == PTMI_TRAVERSAL_AUTO)
        if (const char *e = std::getenv(closest_hit ? "PTMI_OWN_EXTEND" : "PTMI_OWN_SHADOW")) {
            int code = std::atoi(e);
            // (the earlier short form, below every own-leaf code: 1 - 9 a variant with one workgroup per CU, + 10 with two; 20 / 21
            // variants 10 / 11 with two)
            if (code < 40) code = code == 20 ? 102 : code == 21 ? 112 : (code % 10) * 10 + (code >= 10 ? 2 : 1);
            if (pt_variant(code / 10).own && pick(code / 10, code % 10)) return cfg;
        }
    struct Pick { int variant, wgs; };
    // Own leaves: both kernels are box-step heavy (7 - 8 dependent node fetches per ray against 3 - 4 triangle tests) and gain from the
    // second workgroup per CU — 8 waves per SIMD to cover them — more than from resident triangles (config 1, same box: any-hit kernel
    // from two workgroups with quantised nodes 17.1 ms beside the main stream against 21.1 from the full image, +2 % overall)
    static const Pick own_auto[] = {{PT_VARIANT_OWN_LDS_NODES, 2}, {PT_VARIANT_OWN_LDS16_NODES, 2}, {PT_VARIANT_OWN_QLDS_NODES, 2},
                                    {PT_VARIANT_OWN_QLDS16_NODES, 2}, {PT_VARIANT_OWN_LDS, 1}, {PT_VARIANT_OWN_QLDS, 1},
                                    {PT_VARIANT_OWN_QLDS_NODES, 1}, {PT_VARIANT_OWN_LDS_NODES, 1}};
    static const Pick own_lds[] = {{PT_VARIANT_OWN_LDS, 1}, {PT_VARIANT_OWN_QLDS, 1}};
    // The reference's leaves: the any-hit kernel keeps the full LDS image, one workgroup per CU. From the node cache with two
    // workgroups (80 scalar registers since round 2) it is as fast by itself (8.53 ms per 64 spp either way) but takes every wave slot
    // of its CUs: beside it `shade` stretches from 16.5 to 18.3 ms and config 1 loses 4 % (9 767 -> 9 344); with one workgroup it is
    // 40 % slower itself. Mid-size trees (up to 1536 wide nodes, the last pick): all nodes in LDS, one workgroup per CU, stacks
    // spill; measured on cornell_spheres against the global variant: extend -6 %, shadow +5 % (so closest hit only).
    static const Pick ref_closest[] = {{PT_VARIANT_LDS_NODES, 2}, {PT_VARIANT_LDS, 1}, {PT_VARIANT_LDS_NODES, 1}};
    static const Pick ref_lds[] = {{PT_VARIANT_LDS, 1}};
    auto all = [](const auto &l) { return std::make_pair(std::begin(l), std::end(l)); };
    const auto picks = traversal == PTMI_TRAVERSAL_LDS ? (own ? all(own_lds) : all(ref_lds))
                     : own ? (big ? std::make_pair(own_auto, own_auto) : all(own_auto)) : closest_hit ? all(ref_closest) : all(ref_lds);
    if (own || c->sc.root_ref != PT_REF_NONE)                       // (an empty scene with the reference's leaves: the global variant)
        for (const Pick *p = picks.first; p != picks.second; p++)
            if (pick(p->variant, p->wgs)) {
                if (p->variant == PT_VARIANT_LDS) cfg.wgs_per_cu = 2;  // (the code leaves = 1 has always reported)
                return cfg;
            }
    return from_memory();                   // PTMI_TRAVERSAL_LDS: the caller reports that the scene does not fit
}

}  // namespace

PT_HOST {

// the radiance sits at 16-byte stride beside kernels that wait on node fetches from memory (pt_device.h DevPaths)
bool walks_memory_quantised(const TraverseConfig &cfg) {
    return cfg.quantized && pt_variant(cfg.variant).where == PT_FROM_MEMORY;
}

int traverse_pick(const ptmi_ctx *c, bool closest_hit, TraverseConfig &cfg) {
    cfg = traverse_config(c, closest_hit);
    if (closest_hit && c->opt.traversal == PTMI_TRAVERSAL_LDS && pt_variant(cfg.variant).where != PT_LDS_ALL)
        return fail(c, PTMI_E_UNSUPPORTED, "scene needs %zu B of LDS plus the stack; it does not fit in %zu B", lds_scene_bytes(c), kLdsMax);
    return PTMI_OK;
}

int traverse_arm(ptmi_ctx *c, bool closest_hit, SpillArea area, TraverseConfig &cfg, bool record) {
    Lane &ln = c->lane;
    uint32_t *&own = area == kSpillMain ? ln.d_spill : ln.d_spill_side;
    if (cfg.wants_spill && !own) HIP_TRY(c, hipMalloc(&own, pt_spill_bytes(c->n_cu * 8)));          // 128 MiB on 256 CUs
    cfg.spill = area == kSpillAfterExtend && ln.d_spill ? ln.d_spill : own;
    if (record) (closest_hit ? c->st.extend_variant : c->st.shadow_variant) = pt_variant_code(cfg);
    return PTMI_OK;
}

int traverse_ready(ptmi_ctx *c, bool closest_hit, TraverseConfig &cfg) {
    const int rc = traverse_pick(c, closest_hit, cfg);
    return rc ? rc : traverse_arm(c, closest_hit, kSpillMain, cfg, true);
}

void launch_extend(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, const uint32_t *queue, const uint32_t *count,
                   float2 *hits) {
    (c->sc.own ? pt_launch_extend_own : pt_launch_extend)(s, c->n_cu * 8, cfg, c->sc, p, queue, count, hits);
}
void launch_shadow(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, DevShadow sh, const uint32_t *shadow_queue,
                   const uint32_t *count, uint8_t *occluded_out) {
    (c->sc.own ? pt_launch_shadow_own : pt_launch_shadow)(s, c->n_cu * 8, cfg, c->sc, p, sh, shadow_queue, count, occluded_out);
}

}  // namespace pt_host
