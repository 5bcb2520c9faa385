// scene_update.hip — edits of a loaded scene in place (include/ptmi.h: ptmi_update_triangles, _materials, _lights).
//
// ptmi_update_triangles refits, on the device, everything an upload derives from vertex positions, to the values an upload of the edited
// triangles with the uploaded tree's boxes refitted would make. The topology stays: only boxes, triangle images and header values move.
//
//   plan      once per upload, at the first update: the topology of both hierarchies is read back and their nodes are listed by HEIGHT
//             above their deepest leaf (a node's children are inner nodes of a smaller height, or leaves), the number of every walked
//             node in the quantised image is taken from that image itself, and the scratch is made. Neither hierarchy is in preorder
//             (the host builder rotates subtrees), so no sweep over indices would do.
//   images    v0, e1, e2 of every triangle in original order; the longest edge squared in double, max-reduced (the order of a maximum
//             does not matter); the triangles of emissive lights in the shade tables
//   uploaded  per height, one launch: a leaf child's box = min / max over its triangles' vertices, an inner child's = the union of that
//             node's two stored boxes, written one launch earlier; a leaf child also writes its box to its triangles' rows of the leaf-box
//             table. The hierarchy over the reference's leaves (leaves = 1) is refitted by the same kernel: its leaves are the same ranges.
//   own       unit boxes as the builders compute them (pt_box.h pt_unit_box: slivers re-decided, grown by the NEW leaf box), the
//             triangle images in leaf order, |coordinate| max-reduced for the padding; then per height: exact child boxes (kept
//             unpadded in scratch for the parents), stored padded with the builders' pt_pad_box; the padded bounds min / max-reduced
//             for the 16-bit grid (quantise.hip pt_quant_grid), every child through wide_node.h pt_quantise_child, references kept
//   cost      the surface areas of all stored child boxes, summed in a fixed order (per-thread strided sums, a tree per block, the
//             blocks' partial sums added on the host in block order): the same update leaves the same number on every run
// Every kernel of one launch reads only what earlier launches wrote: no hand-off inside a launch, nothing depends on dispatch order.
// Minima and maxima are exact, so the results do not depend on the order of the unions either (which of -0 / +0 a tie returns is open).
#include "ptmi_ctx.h"
#include "pt_box.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace {

constexpr int TB = 256;
constexpr int kCostBlocks = 256;         // partial sums of the cost (one double each)

// The reduction words of one update, preset before it. Every thread of a wave takes part in the wave_* steps (no early return before them).
struct Words {
    unsigned long long emax2;         // bits of the longest edge squared (non-negative doubles order as integers)
    uint32_t edge_bad;                // an edge whose square is not finite
    uint32_t biggest;                 // bits of max |coordinate| over the unit boxes
    uint32_t umin[3], umax[3];        // ord() of the unit boxes' bounds: the own hierarchy's exact root box
    uint32_t qmin[3], qmax[3];        // ord() of the padded child boxes' bounds: the 16-bit grid
    uint32_t spare[2];
    Box6 leaf;                        // k_leaf_bounds: the box of a tree that is one leaf
    double cost[kCostBlocks];
};

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ bool wave_leader() { return (threadIdx.x & 63u) == 0u; }

// v0, e1, e2 of every triangle in original order (scene_image.hip build_image: one IEEE subtraction per component), and the longest
// edge squared as build_image takes it: over e1 and e2, products and sums in double
__global__ void __launch_bounds__(TB) k_tri_images(uint32_t n, const ptmi_triangle *__restrict__ tris, float4 *__restrict__ tp, Words *red) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    unsigned long long best = 0ull; uint32_t bad = 0u;
    if (i < n) {
        const ptmi_triangle &t = tris[i];
        const float4 e1 = make_float4(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2], 0.0f);
        const float4 e2 = make_float4(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2], 0.0f);
        tp[3 * (size_t)i + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], 0.0f);
        tp[3 * (size_t)i + 1] = e1;
        tp[3 * (size_t)i + 2] = e2;
        const float4 e[2] = {e1, e2};
        for (int j = 0; j < 2; j++) {
            const double l2 = (double)e[j].x * e[j].x + (double)e[j].y * e[j].y + (double)e[j].z * e[j].z;
            if (!(l2 <= 1.7e308)) bad = 1u;
            else best = max(best, (unsigned long long)__double_as_longlong(l2));
        }
    }
    best = wave_max64(best); bad = wave_max(bad);
    if (wave_leader()) {
        if (best) atomicMax(&red->emax2, best);
        if (bad) atomicOr(&red->edge_bad, 1u);
    }
}

// the shade tables' copy of the triangle each emissive light names, zeros for every other light (scene_image.hip shade_tables)
__global__ void k_light_tris(uint32_t nl, const ptmi_light *__restrict__ lights, const ptmi_triangle *__restrict__ tris, uint32_t nt,
                             float4 *__restrict__ tab_tris) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= nl) return;
    constexpr int Q = (int)(sizeof(ptmi_triangle) / sizeof(float4));
    const ptmi_light l = lights[i];
    const bool named = l.light_type == PTMI_LIGHT_EMISSIVE && l.triangle_index < nt;
    const float4 *src = named ? reinterpret_cast<const float4 *>(tris + l.triangle_index) : nullptr;
    for (int q = 0; q < Q; q++) tab_tris[(size_t)i * Q + q] = named ? src[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__device__ __forceinline__ Box6 range_box(const ptmi_triangle *__restrict__ tris, uint32_t first, uint32_t cnt) {
    Box6 b = pt_empty_box();
    for (uint32_t t = first; t < first + cnt; t++) {
        const ptmi_triangle &tr = tris[t];
        for (int k = 0; k < 3; k++) {
            b.mn[k] = pt_min(pt_min(pt_min(b.mn[k], tr.v0[k]), tr.v1[k]), tr.v2[k]);
            b.mx[k] = pt_max(pt_max(pt_max(b.mx[k], tr.v0[k]), tr.v1[k]), tr.v2[k]);
        }
    }
    return b;
}
__device__ __forceinline__ uint32_t leaf_first(uint32_t ref) { return ref & PT_LEAF_OFF_MASK; }
__device__ __forceinline__ uint32_t leaf_count(uint32_t ref) { return ((ref >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u; }

// One height of a hierarchy whose leaves are ranges of the ORIGINAL triangles (the tree as uploaded; the one over its leaves). w16: the
// copy with 16-bit references (NULL: none), leafbox: the per-triangle leaf-box table (NULL: none). n_nodes / n_tris bound every index.
__global__ void __launch_bounds__(TB) k_refit_ranges(uint32_t m, const uint32_t *__restrict__ order, uint32_t n_nodes, uint32_t n_tris,
                                                     const ptmi_triangle *__restrict__ tris, float4 *w, float4 *w16, float4 *leafbox) {
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    if (k >= m) return;
    const uint32_t i = order[k];
    if (i >= n_nodes) return;
    float4 *me = w + 4 * (size_t)i;
    for (int side = 0; side < 2; side++) {
        const uint32_t ref = pt_wide_ref(me, side);
        Box6 b;
        if (ref & PT_REF_LEAF) {
            const uint32_t first = leaf_first(ref), cnt = leaf_count(ref);
            if ((uint64_t)first + cnt > n_tris) continue;
            b = range_box(tris, first, cnt);
            if (leafbox)
                for (uint32_t t = first; t < first + cnt; t++) {
                    leafbox[2 * (size_t)t] = make_float4(b.mn[0], b.mn[1], b.mn[2], 0.0f);
                    leafbox[2 * (size_t)t + 1] = make_float4(b.mx[0], b.mx[1], b.mx[2], 0.0f);
                }
        } else {
            if (ref >= n_nodes) continue;
            const float4 *c = w + 4 * (size_t)ref;                  // (a lower height: written by an earlier launch)
            b = pt_unite(pt_child_box(c, 0), pt_child_box(c, 1));
        }
        pt_wide_set_box(me, side, b.mn, b.mx);
        if (w16) pt_wide_set_box(w16 + 4 * (size_t)i, side, b.mn, b.mx);
    }
}

// a tree that is one leaf: its box
__global__ void k_leaf_bounds(uint32_t ref, uint32_t n_tris, const ptmi_triangle *__restrict__ tris, float4 *leafbox, Words *red) {
    const uint32_t first = leaf_first(ref), cnt = leaf_count(ref);
    if ((uint64_t)first + cnt > n_tris) return;
    const Box6 b = range_box(tris, first, cnt);
    red->leaf = b;
    if (leafbox)
        for (uint32_t t = first; t < first + cnt; t++) {
            leafbox[2 * (size_t)t] = make_float4(b.mn[0], b.mn[1], b.mn[2], 0.0f);
            leafbox[2 * (size_t)t + 1] = make_float4(b.mx[0], b.mx[1], b.mx[2], 0.0f);
        }
}

// own leaves: the unit box and the triangle image of every listed triangle, at its place in leaf order (tp[3p].w keeps the original index)
__global__ void __launch_bounds__(TB) k_units(uint32_t n, uint32_t n_tris, const ptmi_triangle *__restrict__ tris,
                                              const float4 *__restrict__ leafbox, float4 *tp, Box6 *__restrict__ unit, Words *red) {
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    uint32_t big = 0u, lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    const uint32_t orig = p < n ? __float_as_uint(tp[3 * (size_t)p].w) : PT_REF_NONE;
    if (orig < n_tris) {
        const ptmi_triangle &t = tris[orig];
        const PtUnitBox ub = pt_unit_box(t.v0, t.v1, t.v2, [&] { return pt_leafbox_row(leafbox, orig); });   // (the NEW leaf box)
        const Box6 &u = ub.box;
        big = ub.biggest;
        for (int k = 0; k < 3; k++) { lo[k] = pt_ord(u.mn[k]); hi[k] = pt_ord(u.mx[k]); }
        unit[p] = u;
        tp[3 * (size_t)p + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], __uint_as_float(orig));
        tp[3 * (size_t)p + 1] = make_float4(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2], 0.0f);
        tp[3 * (size_t)p + 2] = make_float4(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2], 0.0f);
    }
    big = wave_max(big);
    for (int k = 0; k < 3; k++) { lo[k] = wave_min(lo[k]); hi[k] = wave_max(hi[k]); }
    if (wave_leader()) {
        atomicMax(&red->biggest, big);
        for (int k = 0; k < 3; k++) { atomicMin(&red->umin[k], lo[k]); atomicMax(&red->umax[k], hi[k]); }
    }
}

// One height of the own hierarchy: leaves are ranges of the unit boxes. exact: both unpadded child boxes per node.
__global__ void __launch_bounds__(TB) k_refit_own(uint32_t m, const uint32_t *__restrict__ order, uint32_t n_nodes, uint32_t n_units,
                                                  float pad, const Box6 *__restrict__ unit, Box6 *exact, float4 *w, float4 *w16, Words *red) {
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    const uint32_t i = k < m ? order[k] : PT_REF_NONE;
    if (i < n_nodes) {
        float4 *me = w + 4 * (size_t)i;
        for (int side = 0; side < 2; side++) {
            const uint32_t ref = pt_wide_ref(me, side);
            Box6 b;
            if (ref & PT_REF_LEAF) {
                const uint32_t first = leaf_first(ref), cnt = leaf_count(ref);
                if ((uint64_t)first + cnt > n_units) continue;
                b = unit[first];
                for (uint32_t t = first + 1; t < first + cnt; t++) b = pt_unite(b, unit[t]);
            } else {
                if (ref >= n_nodes) continue;
                b = pt_unite(exact[2 * (size_t)ref], exact[2 * (size_t)ref + 1]);     // (a lower height: an earlier launch)
            }
            exact[2 * (size_t)i + side] = b;
            Box6 p;
            for (int a = 0; a < 3; a++) {
                p.mn[a] = pt_pad_lower(b.mn[a], pad); p.mx[a] = pt_pad_upper(b.mx[a], pad);
                lo[a] = min(lo[a], pt_ord(p.mn[a])); hi[a] = max(hi[a], pt_ord(p.mx[a]));
            }
            pt_wide_set_box(me, side, p.mn, p.mx);
            if (w16) pt_wide_set_box(w16 + 4 * (size_t)i, side, p.mn, p.mx);
        }
    }
    for (int a = 0; a < 3; a++) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
    if (wave_leader())
        for (int a = 0; a < 3; a++) { atomicMin(&red->qmin[a], lo[a]); atomicMax(&red->qmax[a], hi[a]); }
}

// every child of every node onto the grid g (wide_node.h), at the node's number in the quantised image; the references stay
__global__ void __launch_bounds__(TB) k_requantise(uint32_t m, PtQuantGrid g, const float4 *__restrict__ w, const uint32_t *__restrict__ qnum,
                                                   uint4 *qn, uint4 *qn16) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= m) return;
    const uint32_t me = qnum[i];
    if (me >= m) return;
    for (int c = 0; c < 2; c++) {
        const PtWideChild ch = pt_wide_child(w + 4 * (size_t)i, c);
        const size_t at = (size_t)me * 2 + c;
        const uint4 q = pt_quantise_child(g, ch.lo, ch.hi, qn[at].w).q;
        qn[at] = q;
        if (qn16) qn16[at] = make_uint4(q.x, q.y, q.z, qn16[at].w);
    }
}

// the surface areas of all child boxes: block b's share, summed in a fixed order
__global__ void __launch_bounds__(TB) k_cost(uint32_t m, const float4 *__restrict__ w, Words *red) {
    __shared__ double s[TB];
    double a = 0.0;
    for (uint32_t i = blockIdx.x * TB + threadIdx.x; i < m; i += kCostBlocks * TB)
        for (int c = 0; c < 2; c++) {
            const PtWideChild ch = pt_wide_child(w + 4 * (size_t)i, c);
            a += pt_box_area(ch.lo, ch.hi);
        }
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = TB / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) red->cost[blockIdx.x] = s[0];
}

dim3 blocks(uint32_t k) { return dim3((k + TB - 1) / TB); }

// The nodes of a hierarchy by height above their deepest leaf (0: both children are leaves), lowest first, ascending index within a
// height. false: the image is not a tree of n nodes below `root` (cannot happen for an image the library made; nothing is touched then).
bool level_lists(const std::vector<float4> &w, uint32_t root, std::vector<uint32_t> &order, std::vector<uint32_t> &off) {
    const uint32_t n = (uint32_t)(w.size() / 4);
    order.clear(); off.assign(1, 0u);
    if (n == 0 || (root & PT_REF_LEAF)) return n == 0;
    if (root >= n) return false;
    std::vector<uint32_t> height(n, PT_REF_NONE), stack{root};
    std::vector<uint8_t> open(n, 0);
    uint32_t seen = 0, top = 0;
    while (!stack.empty()) {                                    // post-order without recursion: a node is closed after its children
        const uint32_t i = stack.back();
        const uint32_t ch[2] = {pt_wide_ref(&w[(size_t)i * 4], 0), pt_wide_ref(&w[(size_t)i * 4], 1)};
        if (!open[i]) {
            open[i] = 1;
            if (++seen > n) return false;
            for (uint32_t c : ch)
                if (!(c & PT_REF_LEAF)) {
                    if (c >= n || open[c]) return false;
                    stack.push_back(c);
                }
            continue;
        }
        stack.pop_back();
        uint32_t h = 0;
        for (uint32_t c : ch) if (!(c & PT_REF_LEAF)) h = std::max(h, height[c] + 1u);
        height[i] = h; top = std::max(top, h);
    }
    if (seen != n) return false;
    off.assign((size_t)top + 2, 0u);
    for (uint32_t i = 0; i < n; i++) off[height[i] + 1]++;
    for (size_t l = 1; l < off.size(); l++) off[l] += off[l - 1];
    order.resize(n);
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    for (uint32_t i = 0; i < n; i++) order[at[height[i]]++] = i;
    return true;
}

template <class T> int to_device(ptmi_ctx *c, SceneBuf k, const std::vector<T> &v) {
    dfree(c->buf[k]);
    HIP_TRY(c, hipMalloc(&c->buf[k], v.empty() ? 16 : v.size() * sizeof(T)));
    if (!v.empty()) HIP_TRY(c, hipMemcpy(c->buf[k], v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PTMI_OK;
}
template <class T> T *buf_as(const ptmi_ctx *c, SceneBuf k) { return static_cast<T *>(c->buf[k]); }

// The reduction words, made on first use. Zeroed on the context's stream and waited for: that stream does not wait for the null stream,
// so a plain hipMemset could land after the first k_cost had written its partial sums.
int ensure_words(ptmi_ctx *c) {
    if (c->buf[kPlanWords]) return PTMI_OK;
    HIP_TRY(c, hipMalloc(&c->buf[kPlanWords], sizeof(Words)));
    HIP_TRY(c, hipMemsetAsync(c->buf[kPlanWords], 0, sizeof(Words), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

}  // namespace

// the plan: shared with scene_rebuild.hip, which re-makes it for a new topology (ptmi_ctx.h)
PT_HOST {

void drop_plan(ptmi_ctx *c) {
    for (SceneBuf k : {kPlanRefOrder, kPlanOrder, kPlanQnum, kPlanUnits, kPlanExact, kPlanWords}) dfree(c->buf[k]);
    c->upd_planned = false; c->upd_ref_off.clear(); c->upd_off.clear();
}

// the cost of the walked hierarchy as it stands on the device (include/ptmi.h ptmi_scene_update_status); synchronises
int walked_cost(ptmi_ctx *c, double &cost) {
    cost = 0.0;
    const uint32_t m = c->sc.n_wnodes;
    if (m == 0) return PTMI_OK;
    int rc = ensure_words(c);                                   // (before the first plan: scratch only, it is no part of a plan's state)
    if (rc) return rc;
    Words *red = buf_as<Words>(c, kPlanWords);
    k_cost<<<kCostBlocks, TB, 0, c->stream>>>(m, c->sc.wnodes, red);
    HIP_TRY(c, hipGetLastError());
    double part[kCostBlocks];
    HIP_TRY(c, hipMemcpyAsync(part, red->cost, sizeof part, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double sum = 0.0;
    for (double p : part) sum += p;
    const double root = pt_box_area(c->sc.root_min, c->sc.root_max);
    cost = root > 0.0 ? sum / root : 0.0;
    return PTMI_OK;
}

// Made at the first update after an upload. The context's scene is not touched; a failure leaves no plan behind.
int make_plan(ptmi_ctx *c) {
    const auto t0 = std::chrono::steady_clock::now();
    drop_plan(c);
    const bool own = c->sc.own != 0;
    const uint32_t n_ref = c->n_ref_wnodes, n_walk = c->buf[kWnodes] ? c->img.n_wnodes : 0u;
    std::vector<float4> w;
    std::vector<uint32_t> order;
    auto fetch = [&](SceneBuf k, uint32_t n) -> int {
        w.assign((size_t)n * 4, make_float4(0, 0, 0, 0));
        if (n) HIP_TRY(c, hipMemcpy(w.data(), c->buf[k], (size_t)n * 64, hipMemcpyDeviceToHost));
        return PTMI_OK;
    };
    int rc = fetch(kRefWnodes, n_ref);
    if (rc) return rc;
    if (!level_lists(w, c->sc.ref_root_ref, order, c->upd_ref_off)) return fail(c, PTMI_E_STATE, "the uploaded tree's image is not a tree");
    if ((rc = to_device(c, kPlanRefOrder, order))) return rc;
    if (n_walk) {
        if ((rc = fetch(kWnodes, n_walk))) return rc;
        if (!level_lists(w, c->img.root_ref, order, c->upd_off)) return fail(c, PTMI_E_STATE, "the walked image is not a tree");
        if ((rc = to_device(c, kPlanOrder, order))) return rc;
        if (own && c->img.quantised && c->buf[kQnodes]) {
            // a node's number in the quantised image: the inner children of node i stand in that image's node qnum[i]
            std::vector<uint4> q((size_t)n_walk * 2);
            HIP_TRY(c, hipMemcpy(q.data(), c->buf[kQnodes], q.size() * sizeof(uint4), hipMemcpyDeviceToHost));
            std::vector<uint32_t> qnum(n_walk, PT_REF_NONE);
            qnum[c->img.root_ref] = 0u;                             // (the root stays node 0; heights descend from the root)
            for (size_t l = c->upd_off.size() - 1; l-- > 0;)
                for (uint32_t k = c->upd_off[l]; k < c->upd_off[l + 1]; k++) {
                    const uint32_t i = order[k], me = qnum[i];
                    if (me >= n_walk) return fail(c, PTMI_E_STATE, "the quantised image does not follow the walked one");
                    for (int s = 0; s < 2; s++) {
                        const uint32_t ch = pt_wide_ref(&w[(size_t)i * 4], s);
                        if (!(ch & PT_REF_LEAF)) qnum[ch] = q[(size_t)me * 2 + s].w;
                    }
                }
            if ((rc = to_device(c, kPlanQnum, qnum))) return rc;
        }
        if (own) HIP_TRY(c, hipMalloc(&c->buf[kPlanExact], (size_t)n_walk * 2 * sizeof(Box6)));
    }
    if (own) HIP_TRY(c, hipMalloc(&c->buf[kPlanUnits], std::max<size_t>(16, (size_t)c->sc.n_own_tris * sizeof(Box6))));
    if ((rc = ensure_words(c))) return rc;
    c->upd = {};
    if ((rc = walked_cost(c, c->upd.cost_built))) return rc;
    c->upd.cost_now = c->upd.cost_built;
    c->upd.quantised_kept = c->img.quantised ? 1u : 0u;
    c->upd.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->upd_planned = true;
    return PTMI_OK;
}

}  // namespace pt_host

namespace {

// one launch per height of a hierarchy over ranges of the original triangles
int refit_ranges(ptmi_ctx *c, const std::vector<uint32_t> &off, SceneBuf order, uint32_t n_nodes, float4 *w, float4 *w16, float4 *leafbox) {
    for (size_t l = 0; l + 1 < off.size(); l++) {
        const uint32_t m = off[l + 1] - off[l];
        if (m) k_refit_ranges<<<blocks(m), TB, 0, c->stream>>>(m, buf_as<uint32_t>(c, order) + off[l], n_nodes, c->sc.n_tris, c->sc.tris, w, w16, leafbox);
    }
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int check_range(ptmi_ctx *c, const char *what, uint32_t first, uint32_t count, uint32_t have, const void *records) {
    if (!c->have_scene) return fail(c, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if ((uint64_t)first + count > have) return fail(c, PTMI_E_INVALID, "%s [%u, +%u) reach beyond the %u uploaded", what, first, count, have);
    if (count && !records) return fail(c, PTMI_E_INVALID, "NULL records with a non-zero count");
    return PTMI_OK;
}

// the lights' triangle copies of the shade tables, from the device's triangles and lights
int refresh_light_tris(ptmi_ctx *c) {
    const DevScene &s = c->sc;
    if (!s.n_lights) return PTMI_OK;
    float4 *tab = buf_as<float4>(c, kShadeTab) + pt_tab_mats_q(s.n_mats) + (size_t)s.n_lights * (sizeof(ptmi_light) / sizeof(float4));
    k_light_tris<<<blocks(s.n_lights), TB, 0, c->stream>>>(s.n_lights, s.lights, s.tris, s.n_tris, tab);
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

}  // namespace

// the edit of the triangles in three steps around the write of the records: shared with scene_transform.hip (ptmi_ctx.h)
PT_HOST {

int refit_begin(ptmi_ctx *c) {
    if (c->n_ref_wnodes && !c->tree_nested)
        return fail(c, PTMI_E_UNSUPPORTED, "the uploaded tree is not nested and finite: it is walked as uploaded, and a refit would change what its boxes mean");
    return PTMI_OK;
}

int refit_ready(ptmi_ctx *c) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                    // nothing in flight reads the scene any more
    int rc;
    if (!c->upd_planned && (rc = make_plan(c))) { drop_plan(c); return rc; }
    return PTMI_OK;
}

int refit_written(ptmi_ctx *c, std::chrono::steady_clock::time_point t0) {
    int rc;
    const bool own = c->sc.own != 0;
    const uint32_t nt = c->sc.n_tris;
    if (nt == 0) { c->upd.updates++; return PTMI_OK; }
    hipStream_t st = c->stream;
    void *const *d = c->buf;
    Words *red = buf_as<Words>(c, kPlanWords);
    {
        Words w0{};
        for (int k = 0; k < 3; k++) { w0.umin[k] = w0.qmin[k] = 0xFFFFFFFFu; w0.umax[k] = w0.qmax[k] = 0u; }
        HIP_TRY(c, hipMemcpy(red, &w0, offsetof(Words, cost), hipMemcpyHostToDevice));
    }
    // the triangle images, the light triangles
    k_tri_images<<<blocks(nt), TB, 0, st>>>(nt, c->sc.tris, static_cast<float4 *>(d[kRefTripos]), red);
    HIP_TRY(c, hipGetLastError());
    if ((rc = refresh_light_tris(c))) return rc;
    // the tree as uploaded (a single leaf: no node), and the leaf boxes of own leaves
    float4 *leafbox = static_cast<float4 *>(d[kLeafbox]);
    if (c->n_ref_wnodes) {
        if ((rc = refit_ranges(c, c->upd_ref_off, kPlanRefOrder, c->n_ref_wnodes, static_cast<float4 *>(d[kRefWnodes]),
                               static_cast<float4 *>(d[kRefWnodes16]), leafbox))) return rc;
    } else if (c->sc.ref_root_ref != PT_REF_NONE) {
        k_leaf_bounds<<<1, 1, 0, st>>>(c->sc.ref_root_ref, nt, c->sc.tris, leafbox, red);
        HIP_TRY(c, hipGetLastError());
    }
    DevScene next = c->sc;
    ptmi_image_info img = c->img;
    bool drop_quantised = false;
    if (own) {
        // unit boxes and the padding they decide
        const uint32_t nu = c->sc.n_own_tris, nw = c->buf[kWnodes] ? img.n_wnodes : 0u;
        Box6 *unit = buf_as<Box6>(c, kPlanUnits);
        k_units<<<blocks(nu), TB, 0, st>>>(nu, nt, c->sc.tris, leafbox, static_cast<float4 *>(d[kTripos]), unit, red);
        HIP_TRY(c, hipGetLastError());
        Words h;
        HIP_TRY(c, hipMemcpyAsync(&h, red, offsetof(Words, cost), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        float pad;
        (void)pt_own_padding((double)pt_bits_float(h.biggest), pad, img.safe_origin);     // (finite: every vertex was checked above)
        img.pad = pad; next.safe_origin = img.safe_origin;
        for (int k = 0; k < 3; k++) {
            img.root_min[k] = next.root_min[k] = pt_pad_lower(pt_unord_f(h.umin[k]), pad);
            img.root_max[k] = next.root_max[k] = pt_pad_upper(pt_unord_f(h.umax[k]), pad);
        }
        if (nw) {
            float4 *w = static_cast<float4 *>(d[kWnodes]), *w16 = static_cast<float4 *>(d[kWnodes16]);
            for (size_t l = 0; l + 1 < c->upd_off.size(); l++) {
                const uint32_t m = c->upd_off[l + 1] - c->upd_off[l];
                if (m) k_refit_own<<<blocks(m), TB, 0, st>>>(m, buf_as<uint32_t>(c, kPlanOrder) + c->upd_off[l], nw, nu, pad, unit,
                                                             buf_as<Box6>(c, kPlanExact), w, w16, red);
            }
            HIP_TRY(c, hipGetLastError());
            if (img.quantised && d[kQnodes] && d[kPlanQnum]) {
                HIP_TRY(c, hipMemcpyAsync(&h, red, offsetof(Words, cost), hipMemcpyDeviceToHost, st));
                HIP_TRY(c, hipStreamSynchronize(st));
                float mn[3], mx[3];
                for (int k = 0; k < 3; k++) { mn[k] = pt_unord_f(h.qmin[k]); mx[k] = pt_unord_f(h.qmax[k]); }
                PtQuantGrid g;
                if (pt_quant_grid(mn, mx, g.origin, g.scale)) {
                    k_requantise<<<blocks(nw), TB, 0, st>>>(nw, g, w, buf_as<uint32_t>(c, kPlanQnum), static_cast<uint4 *>(d[kQnodes]),
                                                            static_cast<uint4 *>(d[kQnodes16]));
                    HIP_TRY(c, hipGetLastError());
                    for (int k = 0; k < 3; k++) { img.q_origin[k] = next.q_origin[k] = g.origin[k]; img.q_scale[k] = next.q_scale[k] = g.scale[k]; }
                } else drop_quantised = true;                     // bounds the grid cannot hold: the exact nodes are walked
            }
        }
    } else if (c->buf[kWnodes]) {
        // the hierarchy over the reference's leaves: exact unions; its quantised nodes and leaf stream go (include/ptmi.h)
        if ((rc = refit_ranges(c, c->upd_off, kPlanOrder, img.n_wnodes, static_cast<float4 *>(d[kWnodes]), nullptr, nullptr))) return rc;
        drop_quantised = img.quantised != 0;
    }
    // the root box of the tree as uploaded, and the longest edge
    Words h;
    float4 root[4];
    HIP_TRY(c, hipMemcpyAsync(&h, red, offsetof(Words, cost), hipMemcpyDeviceToHost, st));
    if (c->n_ref_wnodes) HIP_TRY(c, hipMemcpyAsync(root, static_cast<float4 *>(d[kRefWnodes]) + 4 * (size_t)c->sc.ref_root_ref, sizeof root, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const Box6 rb = c->n_ref_wnodes ? pt_unite(pt_child_box(root, 0), pt_child_box(root, 1)) : h.leaf;
    for (int k = 0; k < 3; k++) { next.ref_root_min[k] = rb.mn[k]; next.ref_root_max[k] = rb.mx[k]; }
    if (!own)
        for (int k = 0; k < 3; k++) { img.root_min[k] = next.root_min[k] = rb.mn[k]; img.root_max[k] = next.root_max[k] = rb.mx[k]; }
    {
        double emax2; std::memcpy(&emax2, &h.emax2, 8);
        const double k = h.edge_bad ? 0.0 : (emax2 > 0.0 ? std::ldexp(1.0, 98) / emax2 : 3.0e38);
        next.tri_safe_dsum = (float)(k < 3.0e38 ? k : 3.0e38);
    }
    if (drop_quantised) {
        img.quantised = 0u;
        next.qnodes = nullptr; next.leaf_stream = nullptr; next.qnodes16 = nullptr; next.q_cached = 0u;
    }
    HIP_TRY(c, hipMemcpy(c->d_scene, &next, sizeof(DevScene), hipMemcpyHostToDevice));
    c->sc = next; c->img = img;
    if (drop_quantised) { dfree(c->buf[kQnodes]); dfree(c->buf[kLeafStream]); dfree(c->buf[kQnodes16]); dfree(c->buf[kPlanQnum]); }
    c->upd.quantised_kept = img.quantised ? 1u : 0u;
    if ((rc = walked_cost(c, c->upd.cost_now))) return rc;
    for (int k = 0; k < 3; k++) { c->upd.root_min[k] = rb.mn[k]; c->upd.root_max[k] = rb.mx[k]; }
    c->upd.updates++;
    c->upd.refit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

int ptmi_update_triangles(ptmi_ctx *c, uint32_t first, uint32_t count, const ptmi_triangle *tris) {
    if (!c) return PTMI_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = check_range(c, "triangles", first, count, c->sc.n_tris, tris);
    if (rc || (rc = refit_begin(c))) return rc;
    const bool own = c->sc.own != 0;
    for (uint32_t i = 0; i < count; i++)
        for (int k = 0; k < 3; k++) {
            const float a = tris[i].v0[k], b = tris[i].v1[k], d = tris[i].v2[k];
            if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(d))
                return fail(c, PTMI_E_INVALID, "triangle %u has a vertex that is not finite", first + i);
            if (own && (!std::isfinite(a + (b - a)) || !std::isfinite(a + (d - a))))
                return fail(c, PTMI_E_INVALID, "triangle %u: an edge is too long for float32 arithmetic", first + i);
        }
    if ((rc = refit_ready(c))) return rc;
    if (count) {
        HIP_TRY(c, hipMemcpy(static_cast<ptmi_triangle *>(c->buf[kTris]) + first, tris, (size_t)count * sizeof(ptmi_triangle), hipMemcpyHostToDevice));
        motion_widen(c, first, count);                          // while motion is on: the previous positions stay, the dirty range grows
        if ((rc = groups_rebase(c, first, count))) return rc;   // while a group table is in place: these records are their triangles' rest pose
        if ((rc = skin_rebase(c, first, count))) return rc;     // ... and while a skin is: the rest pose of the listed triangles among them
        if ((rc = morph_rebase(c, first, count))) return rc;    // ... and while a morph is: likewise
    }
    return refit_written(c, t0);
}

int ptmi_update_materials(ptmi_ctx *c, uint32_t first, uint32_t count, const ptmi_material *mats) {
    if (!c) return PTMI_E_INVALID;
    int rc = check_range(c, "materials", first, count, c->sc.n_mats, mats);
    if (rc || !count) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    const size_t at = (size_t)first * sizeof(ptmi_material), bytes = (size_t)count * sizeof(ptmi_material);
    HIP_TRY(c, hipMemcpy(static_cast<char *>(c->buf[kMats]) + at, mats, bytes, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(static_cast<char *>(c->buf[kShadeTab]) + at, mats, bytes, hipMemcpyHostToDevice));    // (the table starts with them)
    return PTMI_OK;
}

int ptmi_update_lights(ptmi_ctx *c, uint32_t first, uint32_t count, const ptmi_light *lights) {
    if (!c) return PTMI_E_INVALID;
    int rc = check_range(c, "lights", first, count, c->sc.n_lights, lights);
    if (rc || !count) return rc;
    for (uint32_t i = 0; i < count; i++) {
        if (lights[i].light_type > PTMI_LIGHT_POINT)
            return fail(c, PTMI_E_INVALID, "light %u has unknown type %u", first + i, lights[i].light_type);
        if (lights[i].light_type == PTMI_LIGHT_EMISSIVE && lights[i].triangle_index >= c->sc.n_tris)
            return fail(c, PTMI_E_INVALID, "emissive light %u references triangle %u of %u", first + i, lights[i].triangle_index, c->sc.n_tris);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    const size_t at = (size_t)first * sizeof(ptmi_light), bytes = (size_t)count * sizeof(ptmi_light);
    HIP_TRY(c, hipMemcpy(static_cast<char *>(c->buf[kLights]) + at, lights, bytes, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(static_cast<char *>(c->buf[kShadeTab]) + pt_tab_mats_q(c->sc.n_mats) * sizeof(float4) + at, lights, bytes, hipMemcpyHostToDevice));
    if ((rc = refresh_light_tris(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_scene_update_status(ptmi_ctx *c, struct ptmi_scene_update_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->upd;
    return PTMI_OK;
}

}  // extern "C"
