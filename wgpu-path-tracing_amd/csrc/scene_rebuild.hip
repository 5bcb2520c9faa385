// scene_rebuild.hip — the walked own-leaf hierarchy rebuilt in place (include/ptmi.h: ptmi_rebuild_tree).
//
// A refit keeps the topology, so the walked tree degrades as geometry moves. The own-leaf hierarchy (leaves = 2) is the one part of the
// traversal image with total freedom: any topology over conservative boxes gives the same hits. After an edit
// everything its builders read is on the device, refitted: the triangles, the per-triangle box of the reference leaf (kLeafbox, which
// the refit keeps current) and the uploaded tree. ptmi_rebuild_tree builds the image an upload of that state would build and swaps it in.
//
//   units     the builders' unit list: the triangles some reachable reference leaf lists, ascending. Every node of kRefWnodes is
//             reachable (an upload numbers only those), so: one ballot word per 64 triangles, a leaf child ORs the bits of its range
//             into at most two words (atomicOr: ranges of different leaves share words; the result does not depend on the order);
//             then the ordered list of the set bits (pt_ballot_list.h, the bodies the compaction of a bounce uses: per-tile popcount
//             totals, then scatter_tile). On the device path nothing per triangle crosses the bus.
//   build     scene_image.hip rebuild_own_image: the code an upload builds own leaves with (which builder, which limits, the 16-bit
//             copies), reading the context's buffers; new buffers, the context untouched
//   swap      every holder of the old pointers moves together: the SceneBuf table, DevScene and its device copy, the image header, the
//             statistics, and the update plan, which described the old topology and is re-made here. The old buffers and the old plan are
//             kept until the new plan stands, so a failure anywhere puts them back: the call is all-or-nothing.
// Every kernel of one launch reads only what earlier launches wrote (scene_update.hip's rule): no hand-off inside a launch.
#include "pt_ballot_list.h"
#include "ptmi_ctx.h"
#include "wide_node.h"

#include <chrono>
#include <utility>

namespace {

constexpr int TB = 256;

__device__ __forceinline__ void flag_range(uint32_t ref, uint32_t n_tris, unsigned long long *words) {
    const uint32_t first = ref & PT_LEAF_OFF_MASK, cnt = ((ref >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u;   // cnt <= 32
    if ((uint64_t)first + cnt > n_tris) return;
    const uint32_t lo = first & 63u;
    const unsigned long long m = (1ull << cnt) - 1ull;
    atomicOr(&words[first >> 6], m << lo);
    if (lo + cnt > 64u) atomicOr(&words[(first >> 6) + 1u], m >> (64u - lo));      // (lo > 32 here: the shift is 1 .. 31)
}

// one thread per node of the tree as uploaded: the triangles its leaf children list. words: (n_tris + 63) / 64 of them, zeroed.
__global__ void __launch_bounds__(TB) k_flag_leaves(uint32_t n_nodes, const float4 *__restrict__ w, uint32_t n_tris, unsigned long long *words) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_nodes) return;
    for (int side = 0; side < 2; side++) {
        const uint32_t ref = pt_wide_ref(w + 4 * (size_t)i, side);
        if (ref & PT_REF_LEAF) flag_range(ref, n_tris, words);
    }
}
// a tree that is one leaf
__global__ void k_flag_root(uint32_t ref, uint32_t n_tris, unsigned long long *words) {
    if (ref != PT_REF_NONE && (ref & PT_REF_LEAF)) flag_range(ref, n_tris, words);
}

__global__ void __launch_bounds__(TILE_WORDS) k_unit_tile_sums(uint32_t nwords, const uint64_t *__restrict__ words,
                                                               uint32_t *__restrict__ tile_sums) {
    tile_total(nwords, words, tile_sums);
}
// the set bits' positions, ascending, into which[] (`cap` entries of room); their number into *count (the last tile writes it)
__global__ void __launch_bounds__(TILE_WORDS) k_unit_scatter(uint32_t nwords, const uint64_t *__restrict__ words,
                                                             const uint32_t *__restrict__ tile_sums, uint32_t cap, uint32_t *__restrict__ which,
                                                             uint32_t *__restrict__ count) {
    scatter_tile<false, true>(blockIdx.x, nwords, nullptr, words, tile_sums, which, count, TileStats{}, cap);
}

// The unit list of the loaded scene in device memory: *d_which (n_tris entries of room, owned by the caller's Scratch) and its length.
int unit_list(ptmi_ctx *c, Scratch<uint32_t> &which, uint32_t &n_units) {
    const uint32_t nt = c->sc.n_tris, nwords = (nt + 63u) / 64u, tiles = pt_ballot_tiles(nt);
    hipStream_t st = c->stream;
    Scratch<unsigned long long> words;
    Scratch<uint32_t> sums;                                          // the tile totals, then the count
    HIP_TRY(c, hipMalloc(&words.p, (size_t)nwords * 8));
    HIP_TRY(c, hipMalloc(&sums.p, ((size_t)tiles + 1) * 4));
    HIP_TRY(c, hipMalloc(&which.p, (size_t)nt * 4));
    HIP_TRY(c, hipMemsetAsync(words.p, 0, (size_t)nwords * 8, st));
    if (c->n_ref_wnodes)
        k_flag_leaves<<<dim3((c->n_ref_wnodes + TB - 1) / TB), TB, 0, st>>>(c->n_ref_wnodes, c->sc.ref_wnodes, nt, words.p);
    else
        k_flag_root<<<1, 1, 0, st>>>(c->sc.ref_root_ref, nt, words.p);
    const uint64_t *const bits = reinterpret_cast<const uint64_t *>(words.p);      // (atomicOr has no uint64_t form)
    k_unit_tile_sums<<<tiles, TILE_WORDS, 0, st>>>(nwords, bits, sums.p);
    k_unit_scatter<<<tiles, TILE_WORDS, 0, st>>>(nwords, bits, sums.p, nt, which.p, sums.p + tiles);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&n_units, sums.p + tiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (n_units > nt) return fail(c, PTMI_E_STATE, "the unit list has %u entries for %u triangles", n_units, nt);
    return PTMI_OK;
}

// the entries of the SceneBuf table a rebuild replaces, and the plan's
constexpr SceneBuf kImage[] = {kWnodes, kTripos, kQnodes, kWnodes16, kRefWnodes16, kQnodes16};
constexpr SceneBuf kPlan[] = {kPlanRefOrder, kPlanOrder, kPlanQnum, kPlanUnits, kPlanExact, kPlanWords};

// What a swap moves, as it was before: put back when the new plan cannot be made.
struct Before {
    void *buf[kSceneBufs] = {};
    DevScene sc;
    ptmi_image_info img;
    bool planned;
    std::vector<uint32_t> ref_off, off;
    struct ptmi_scene_update_status upd;
};

// The new image in place of the old one, and the plan for it.
int swap_in(ptmi_ctx *c, OwnRebuilt &nw) {
    Before old;
    old.sc = c->sc; old.img = c->img; old.planned = c->upd_planned; old.upd = c->upd;
    old.ref_off = std::move(c->upd_ref_off); old.off = std::move(c->upd_off);
    for (SceneBuf k : kImage) { old.buf[k] = c->buf[k]; c->buf[k] = nw.buf[k]; nw.buf[k] = nullptr; }
    for (SceneBuf k : kPlan) { old.buf[k] = c->buf[k]; c->buf[k] = nullptr; }
    c->upd_planned = false; c->upd_ref_off.clear(); c->upd_off.clear();
    void *const *d = c->buf;
    const ptmi_image_info &h = nw.img;
    DevScene &s = c->sc;
    s.wnodes = static_cast<const float4 *>(d[kWnodes]); s.n_wnodes = h.n_wnodes; s.has_fast = 1u;
    s.tripos = static_cast<const float4 *>(d[kTripos]); s.n_own_tris = h.n_tris;
    s.qnodes = static_cast<const uint4 *>(d[kQnodes]); s.q_cached = nw.q_top;
    s.wnodes16 = static_cast<const float4 *>(d[kWnodes16]); s.ref_wnodes16 = static_cast<const float4 *>(d[kRefWnodes16]);
    s.qnodes16 = static_cast<const uint4 *>(d[kQnodes16]);
    s.root_ref = h.root_ref; s.root_ref16 = nw.root_ref16; s.ref_root_ref16 = nw.ref_root_ref16;
    s.safe_origin = h.safe_origin;
    for (int k = 0; k < 3; k++) {
        s.root_min[k] = h.root_min[k]; s.root_max[k] = h.root_max[k];
        s.q_origin[k] = h.q_origin[k]; s.q_scale[k] = h.q_scale[k];
    }
    c->img = h;
    int rc = PTMI_OK;
    const hipError_t e = hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(c, PTMI_E_HIP, "writing the scene header failed: %s", hipGetErrorString(e));
    if (!rc) rc = make_plan(c);                                      // (sets c->upd: cost_built = cost_now = the new tree's, plan_ms)
    if (rc) {                                                        // back to the old image and the old plan; the error message stays
        drop_plan(c);
        for (SceneBuf k : kImage) { dfree(c->buf[k]); c->buf[k] = old.buf[k]; }
        for (SceneBuf k : kPlan) c->buf[k] = old.buf[k];
        c->sc = old.sc; c->img = old.img; c->upd_planned = old.planned; c->upd = old.upd;
        c->upd_ref_off = std::move(old.ref_off); c->upd_off = std::move(old.off);
        (void)hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice);
        (void)hipGetLastError();
        return rc;
    }
    for (SceneBuf k : kImage) dfree(old.buf[k]);
    for (SceneBuf k : kPlan) dfree(old.buf[k]);
    // an update's own numbers stay: how many there were, the last one's time, the uploaded tree's root box
    c->upd.updates = old.upd.updates; c->upd.refit_ms = old.upd.refit_ms;
    for (int k = 0; k < 3; k++) { c->upd.root_min[k] = old.upd.root_min[k]; c->upd.root_max[k] = old.upd.root_max[k]; }
    c->st.leaf_tris_used = h.max_leaf_tris;
    c->st.tree_builder_used = nw.builder_used;
    return PTMI_OK;
}

}  // namespace

int pt_check_rebuild(const ptmi_ctx *c, const ptmi_rebuild_params *p, std::string &err) {
    if (p) {
        if (p->builder > 2u) return fail(err, PTMI_E_INVALID, "ptmi_rebuild_params.builder = %u: 0 (the default), 1 (host) or 2 (device)", p->builder);
        for (uint32_t r : p->reserved) if (r) return fail(err, PTMI_E_INVALID, "ptmi_rebuild_params.reserved must be 0");
    }
    if (!c->have_scene) return fail(err, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if (c->sc.own) return PTMI_OK;
    const char *why = c->sc.n_tris == 0 || c->sc.ref_root_ref == PT_REF_NONE ? "the scene is empty"
                    : c->n_ref_wnodes == 0                                      ? "the uploaded tree is a single leaf"
                    : !c->tree_nested                                           ? "the uploaded tree is not nested and finite, so it is walked as uploaded"
                    : c->sc.has_fast ? "it was uploaded with leaves = 1: the hierarchy over the reference's leaves is not rebuilt"
                                     : "it was uploaded with keep_reference_tree: the tree is walked as uploaded";
    return fail(err, PTMI_E_UNSUPPORTED, "the loaded image has no own leaves to rebuild: %s", why);
}

extern "C" {

int ptmi_rebuild_tree(ptmi_ctx *c, const ptmi_rebuild_params *params) {
    if (!c) return PTMI_E_INVALID;
    int rc = pt_check_rebuild(c, params, c->err);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                    // nothing in flight reads the old image any more
    struct ptmi_rebuild_status st = c->reb;
    if ((rc = walked_cost(c, st.cost_before))) return rc;
    ptmi_options opt = c->opt;
    opt.leaves = 2u; opt.keep_reference_tree = 0u;
    opt.tree_builder = params && params->builder ? params->builder : 2u;
    OwnRebuilt nw;
    {
        Scratch<uint32_t> which;
        uint32_t n_units = 0;
        if ((rc = unit_list(c, which, n_units))) return rc;
        if ((rc = rebuild_own_image(c, opt, which.p, n_units, nw))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if ((rc = swap_in(c, nw))) return rc;
    st.cost_after = c->upd.cost_now;
    st.rebuilds++;
    st.builder_used = nw.builder_used;
    st.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->reb = st;
    return PTMI_OK;
}

int ptmi_rebuild_status(ptmi_ctx *c, struct ptmi_rebuild_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->reb;
    return PTMI_OK;
}

}  // extern "C"
