// scene_image.hip — an uploaded scene: validation of the caller's BVH, the traversal image the kernels walk (the tree as uploaded, a
// hierarchy rebuilt over its leaves, or the library's own leaves: fast_tree.h; quantised: quantise.hip), and its installation on a
// device.
//
// Replaces the reference's scene buffers (src/renderer/renderer.ts: createBuffers :242-355).
#include "ptmi_ctx.h"
#include "fast_tree.h"
#include "wide_node.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <typeinfo>
#include <utility>

namespace {

// ---- scene validation and the traversal image ---------------------------------
// One scene buffer as a preparation leaves it: absent, host bytes (a vector moved in, or the caller's blob), or a buffer on `device` that
// the install takes over or copies.
struct HeldBuf {
    bool present = false;
    std::shared_ptr<const void> keep;        // the vector `host` points into (none: the caller's blob)
    const std::type_info *type = nullptr;    // ... and its type
    const void *host = nullptr;
    void *dev = nullptr;
    int device = -1;
    size_t bytes = 0;
};

// The scene's buffers, and one header for the image the kernels walk.
struct Built {
    HeldBuf buf[kSceneBufs];
    ptmi_image_info img{};                   // the walked image (ptmi_debug_read_image); ref_depth: levels of the tree as uploaded
    uint32_t ref_root_ref = PT_REF_NONE;     // the root of the tree as uploaded
    float ref_root_min[3] = {0, 0, 0}, ref_root_max[3] = {0, 0, 0};
    uint32_t root_ref16 = PT_REF_NONE, ref_root_ref16 = PT_REF_NONE;     // the roots of kWnodes16 / kRefWnodes16
    uint32_t q_top = 0;                      // quantised nodes numbered breadth-first at the front (LDS-resident in the kernel)
    float tri_safe_dsum = 0.0f;              // DevScene::tri_safe_dsum
    uint32_t tree_builder_used = 0;          // ptmi_stats.tree_builder_used
    bool nested = false;                     // the uploaded tree is nested and finite (ptmi_update_triangles refits only such a tree)
    double tree_ms = 0.0;                    // time spent building and quantising the walked hierarchy

    Built() { img.leaves_used = 1; img.root_ref = PT_REF_NONE; }
    Built(const Built &) = delete;
    Built &operator=(const Built &) = delete;
    ~Built() { for (HeldBuf &e : buf) if (e.dev) (void)hipFree(e.dev); }

    template <class T> void hold(int k, std::vector<T> &&v) {
        auto p = std::make_shared<const std::vector<T>>(std::move(v));
        buf[k].present = true; buf[k].host = p->data(); buf[k].bytes = p->size() * sizeof(T); buf[k].keep = std::move(p);
        buf[k].type = &typeid(std::vector<T>);
    }
    void view(int k, const void *host, size_t bytes) { buf[k].present = true; buf[k].host = host; buf[k].bytes = bytes; }
    void on_device(int k, void *dev, size_t bytes, int device) {
        buf[k].present = true; buf[k].dev = dev; buf[k].bytes = bytes; buf[k].device = device;
    }
    template <class T> const std::vector<T> &vec(int k) const {       // an entry held on the host as a vector of T (else empty)
        static const std::vector<T> none;
        const HeldBuf &e = buf[k];
        return e.type && *e.type == typeid(std::vector<T>) ? *static_cast<const std::vector<T> *>(e.keep.get()) : none;
    }
};

// kWnodes / kTripos as the kernels walk them, in a preparation's table or a context's: the reference's entry when no other image was built
bool present(const HeldBuf &e) { return e.present; }
bool present(const void *d) { return d != nullptr; }
template <class E> const E &walked(const E *buf, SceneBuf k) { return present(buf[k]) ? buf[k] : buf[k == kWnodes ? kRefWnodes : kRefTripos]; }

// a copy of a wide-node image whose child references fit 16 bits: an internal node's index, or 0x8000 | (count - 1) << 12 | first
// triangle. false: some reference does not fit (more than 32 767 nodes, a leaf beyond triangle 4 095 or of more than 8 triangles)
bool compact_ref(uint32_t r, uint32_t &o) {
    if (r & PT_REF_LEAF) {
        const uint32_t first = r & PT_LEAF_OFF_MASK, cnt = ((r >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u;
        if (first > 0xFFFu || cnt > 8u) return false;
        o = 0x8000u | ((cnt - 1u) << 12) | first;
    } else {
        if (r > 0x7FFFu) return false;
        o = r;
    }
    return true;
}
bool compact_refs(const std::vector<float4> &w, uint32_t root, std::vector<float4> &out, uint32_t &root16) {
    out = w;
    if (root == PT_REF_NONE || !compact_ref(root, root16)) return false;
    for (size_t i = 0; i < w.size() / 4; i++)
        for (int side = 0; side < 2; side++) {
            uint32_t r16;
            if (!compact_ref(pt_wide_ref(&w[i * 4], side), r16)) return false;
            pt_wide_set_ref(&out[i * 4], side, r16);
        }
    return true;
}

#ifndef PT_LEAVES_DEFAULT
#define PT_LEAVES_DEFAULT 2            /* what ptmi_options.leaves = 0 means (measured: profiles/README.md) */
#endif
#ifndef PT_LEAF_TRIS_DEFAULT
#define PT_LEAF_TRIS_DEFAULT 2         /* ... and ptmi_options.leaf_tris = 0 */
#endif

uint32_t leaf_ref(const ptmi_bvh_node &n) {
    return PT_REF_LEAF | ((n.triangle_count - 1u) << PT_LEAF_OFF_BITS) | n.triangle_offset;
}

// The own tree on `device` (own_tree_gpu.hip) from a device copy of the triangles, made first and kept as b's kTris for the upload to
// take over. false: not built (the caller builds on the host).
bool own_tree_on_device(hipStream_t stream, int device, const ptmi_triangle *tris, uint32_t nt, const std::vector<uint32_t> &which,
                        const std::vector<float4> &leafbox, uint32_t k_max, uint32_t limit, Built &b, PtOwnTreeGpu &g) {
    const size_t bytes = (size_t)nt * sizeof(ptmi_triangle);
    void *d_tris = nullptr;
    if (hipMalloc(&d_tris, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMemcpy(d_tris, tris, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_tris); (void)hipGetLastError(); return false; }
    b.on_device(kTris, d_tris, bytes, device);
    return pt_build_own_tree_gpu(static_cast<const ptmi_triangle *>(d_tris), which, leafbox, k_max, limit, stream, g);
}

// Own leaves, after whichever builder ran (on_device: g on `device`, else t): the walked image and its header, the quantised nodes (the
// device builder made its own) and, for scenes of up to 4 096 triangles, both hierarchies and the quantised nodes once more with 16-bit
// child references (the device builder only runs on larger scenes).
void own_image(Built &b, bool on_device, int device, PtOwnTreeGpu &g, PtOwnTree &t, uint32_t nt, const std::vector<float4> &ref_wnodes) {
    ptmi_image_info &h = b.img;
    const PtOwnTreeHeader &o = on_device ? static_cast<const PtOwnTreeHeader &>(g) : t;
    h.leaves_used = 2u; h.root_ref = o.root_ref; h.depth = o.depth; h.n_leaves = o.n_leaves; h.max_leaf_tris = o.max_leaf_tris;
    for (int k = 0; k < 3; k++) { h.root_min[k] = o.root_min[k]; h.root_max[k] = o.root_max[k]; }
    h.pad = o.pad; h.safe_origin = o.safe_origin;
    b.tree_builder_used = on_device ? 2u : 1u;
    if (on_device) {
        h.n_wnodes = g.n_wnodes; h.n_tris = g.n_tris; h.quantised = g.quantised ? 1u : 0u; b.q_top = g.q_top;
        for (int k = 0; k < 3; k++) { h.q_origin[k] = g.q_origin[k]; h.q_scale[k] = g.q_scale[k]; }
        b.on_device(kWnodes, g.wnodes, (size_t)g.n_wnodes * 64, device);
        b.on_device(kTripos, g.tripos, (size_t)g.n_tris * 48, device);
        if (g.quantised) b.on_device(kQnodes, g.qnodes, (size_t)g.n_wnodes * 32, device);
        g.wnodes = nullptr; g.tripos = nullptr; g.qnodes = nullptr;
        return;
    }
    std::vector<uint4> q;
    float qo[3], qs[3];
    if (pt_quantize_nodes(t.wnodes, q, qo, qs, PT_QCACHE_NODES, b.q_top))
        for (int k = 0; k < 3; k++) { h.q_origin[k] = qo[k]; h.q_scale[k] = qs[k]; }
    else q.clear();
    std::vector<float4> w16, r16;
    uint32_t root16, ref_root16;
    if (nt <= 4096u && !t.wnodes.empty() && compact_refs(t.wnodes, t.root_ref, w16, root16) && compact_refs(ref_wnodes, b.ref_root_ref, r16, ref_root16)) {
        b.root_ref16 = root16; b.ref_root_ref16 = ref_root16;
        if (!q.empty()) {                              // (the quantised nodes are renumbered: node 0 stays the root)
            std::vector<uint4> q16 = q;
            bool ok = true;
            for (uint4 &x : q16) if (!(ok = compact_ref(x.w, x.w))) break;
            if (ok) b.hold(kQnodes16, std::move(q16));
        }
        b.hold(kWnodes16, std::move(w16)); b.hold(kRefWnodes16, std::move(r16));
    }
    h.n_wnodes = (uint32_t)(t.wnodes.size() / 4); h.n_tris = (uint32_t)(t.tripos.size() / 3); h.quantised = q.empty() ? 0u : 1u;
    b.hold(kWnodes, std::move(t.wnodes)); b.hold(kTripos, std::move(t.tripos));
    if (!q.empty()) b.hold(kQnodes, std::move(q));
}

// What the host builder of the own leaves reads: an upload has it at hand, a rebuild reads it back from the device only when it is needed.
struct OwnHostInputs {
    const ptmi_triangle *tris = nullptr;
    const std::vector<uint32_t> *which = nullptr;        // the unit list: the triangles some reachable reference leaf lists, ascending
    const std::vector<float4> *leafbox = nullptr;        // per original triangle, the box of the reference leaf that lists it
    const std::vector<float4> *ref_wnodes = nullptr;     // the tree as uploaded (for its 16-bit copy)
};

// Own leaves over n_units of a scene's nt triangles under `opt`, into b: the one place that says which builder runs and with what limits,
// for an upload (build_image) and a rebuild (rebuild_own_image) alike. device_build(k_max, limit, g): the device builder on the caller's
// device inputs (false: not built); host_inputs(in): the host builder's inputs (false: they could not be had). have_device: there is
// a stream to build on. false: no own leaves were built (b is as it was).
template <class DeviceBuild, class HostInputs>
bool own_leaves(const ptmi_options &opt, bool have_device, int device, uint32_t nt, uint32_t n_units, Built &b, DeviceBuild &&device_build,
                HostInputs &&host_inputs) {
    const uint32_t k_max = opt.leaf_tris ? opt.leaf_tris : (uint32_t)PT_LEAF_TRIS_DEFAULT;
    // small scenes: at most 14 levels, so that a lane's whole node stack fits the 15 LDS entries of two workgroups per CU
    const uint32_t limit = n_units <= 2048 ? 14u : 60u;
    // tree_builder = 2: on the device for scenes above 4 096 triangles. Smaller scenes keep the host builder (a few ms): they get the
    // 16-bit images, and which of the LDS variants fits them turns on a few tens of nodes (cornell_spheres: the host tree has 2 038,
    // within the 2 046 of the quantised 16-bit variant; the device tree 2 109). Also on the host: without a device (the host-only
    // debug entry points) and when the device build fails
    PtOwnTreeGpu g;
    PtOwnTree t;
    const bool on_device = opt.tree_builder == 2u && have_device && nt > 4096u && n_units > 2048u && device_build(k_max, limit, g);
    OwnHostInputs in;
    static const std::vector<float4> none;
    if (!on_device && !(host_inputs(in) && pt_build_own_tree(in.tris, *in.which, *in.leafbox, k_max, limit, t))) return false;
    own_image(b, on_device, device, g, t, nt, in.ref_wnodes ? *in.ref_wnodes : none);
    return true;
}

// The traversal image of a scene under `opt`. tree_builder = 2 builds on `device` through `stream` (none: the host-only debug entry
// points build on the host). err: why a scene is refused.
int build_image(const ptmi_options &opt, hipStream_t stream, int device, const ptmi_triangle *tris, uint32_t nt,
                const ptmi_bvh_node *nodes, uint32_t nn, Built &b, std::string &err) {
    if (nt == 0 || nn == 0) {                                      // empty scene: every ray misses
        b.hold(kRefWnodes, std::vector<float4>()); b.hold(kRefTripos, std::vector<float4>());
        return PTMI_OK;
    }
    if (nt > PT_LEAF_OFF_MASK) return fail(err, PTMI_E_UNSUPPORTED, "more than %u triangles", PT_LEAF_OFF_MASK);
    // leaf <=> triangleCount > 0 (pt.wgsl:271)
    auto check_leaf = [&](uint32_t i) -> int {
        const ptmi_bvh_node &n = nodes[i];
        if (n.triangle_count > PT_LEAF_MAX_TRIS)
            return fail(err, PTMI_E_UNSUPPORTED, "BVH leaf %u holds %u triangles (limit %u)", i, n.triangle_count, PT_LEAF_MAX_TRIS);
        if ((uint64_t)n.triangle_offset + n.triangle_count > nt)
            return fail(err, PTMI_E_INVALID, "BVH leaf %u references triangles [%u,+%u) beyond %u", i, n.triangle_offset, n.triangle_count, nt);
        return PTMI_OK;
    };
    std::vector<uint32_t> wide_of(nn, PT_REF_NONE);
    std::vector<uint8_t> seen(nn, 0);
    struct Item { uint32_t node, depth; };
    std::vector<Item> stack;
    // pass 1: preorder (left first) numbering of the internal nodes
    stack.push_back({0u, 1u});
    uint32_t n_wide = 0, depth = 0, max_leaf_tris = 0;
    uint64_t next_offset = 0;               // leaves must come in ascending triangle order along the left-first DFS (below)
    while (!stack.empty()) {
        Item it = stack.back(); stack.pop_back();
        if (it.node >= nn) return fail(err, PTMI_E_INVALID, "BVH child index %u out of range (%u nodes)", it.node, nn);
        if (seen[it.node]) return fail(err, PTMI_E_INVALID, "BVH node %u is reachable twice", it.node);
        seen[it.node] = 1;
        depth = std::max(depth, it.depth);
        if (it.depth > 62) return fail(err, PTMI_E_UNSUPPORTED, "BVH deeper than 62 levels (the reference's own traversal stack holds 64 entries, pt.wgsl:249)");
        const ptmi_bvh_node &n = nodes[it.node];
        if (n.triangle_count > 0) {
            int rc = check_leaf(it.node); if (rc) return rc;
            // pt.wgsl:274 keeps the FIRST of equally near hits in its left-first DFS; the kernels visit leaves in another
            // order and break ties by the lowest triangle index. The two agree iff leaf ranges ascend along that DFS —
            // true of every tree bvh.ts builds (children split one contiguous range, left = lower part, bvh.ts:114-127).
            if (n.triangle_offset < next_offset)
                return fail(err, PTMI_E_UNSUPPORTED, "BVH leaf %u starts at triangle %u but an earlier leaf of the left-first DFS ends at %llu: "
                            "leaf ranges must ascend in DFS order (as bvh.ts builds them)", it.node, n.triangle_offset, (unsigned long long)next_offset);
            next_offset = (uint64_t)n.triangle_offset + n.triangle_count;
            max_leaf_tris = std::max(max_leaf_tris, n.triangle_count);
            continue;
        }
        wide_of[it.node] = n_wide++;
        stack.push_back({n.right, it.depth + 1});
        stack.push_back({n.left, it.depth + 1});
    }
    std::vector<float4> wnodes((size_t)n_wide * 4, make_float4(0, 0, 0, 0));
    auto ref_of = [&](uint32_t i) { return nodes[i].triangle_count > 0 ? leaf_ref(nodes[i]) : wide_of[i]; };
    for (uint32_t i = 0; i < nn; i++) {
        if (wide_of[i] == PT_REF_NONE) continue;
        const ptmi_bvh_node &L = nodes[nodes[i].left], &R = nodes[nodes[i].right];
        pt_wide_pack(&wnodes[(size_t)wide_of[i] * 4], L.aabb_min, L.aabb_max, ref_of(nodes[i].left), R.aabb_min, R.aabb_max,
                     ref_of(nodes[i].right));
    }
    for (int k = 0; k < 3; k++) { b.ref_root_min[k] = nodes[0].aabb_min[k]; b.ref_root_max[k] = nodes[0].aabb_max[k]; }
    b.ref_root_ref = ref_of(0);
    // the header of the tree as uploaded: the image the kernels walk unless a hierarchy is built below
    ptmi_image_info &h = b.img;
    h.n_wnodes = n_wide; h.n_tris = nt; h.root_ref = b.ref_root_ref; h.depth = h.ref_depth = depth; h.max_leaf_tris = max_leaf_tris;
    for (int k = 0; k < 3; k++) { h.root_min[k] = b.ref_root_min[k]; h.root_max[k] = b.ref_root_max[k]; }
    // Nested tree (each node box contains its children's, all finite)? Then rebuild the hierarchy over the
    // reference's leaves (fast_tree.hip explains why the results cannot change).
    bool nested = n_wide > 0;
    std::vector<PtFastLeaf> leaves;
    for (uint32_t i = 0; i < nn && nested; i++) {
        if (!seen[i]) continue;
        const ptmi_bvh_node &n = nodes[i];
        for (int k = 0; k < 3; k++) nested = nested && std::isfinite(n.aabb_min[k]) && std::isfinite(n.aabb_max[k]);
        if (n.triangle_count > 0) {
            PtFastLeaf l;
            for (int k = 0; k < 3; k++) { l.mn[k] = n.aabb_min[k]; l.mx[k] = n.aabb_max[k]; }
            l.ref = leaf_ref(n); l.weight = n.triangle_count;
            leaves.push_back(l);
        } else {
            for (uint32_t ch : {n.left, n.right})
                for (int k = 0; k < 3; k++)
                    nested = nested && nodes[ch].aabb_min[k] >= n.aabb_min[k] && nodes[ch].aabb_max[k] <= n.aabb_max[k];
        }
    }
    b.nested = nested;
    const uint32_t leaves_mode = opt.leaves ? opt.leaves : (uint32_t)PT_LEAVES_DEFAULT;
    bool own = false;
    if (nested && leaves_mode == 2u && !opt.keep_reference_tree) {
        // The library's own leaves (fast_tree.h). What the reference's semantics need from the uploaded tree is kept beside them: the
        // tree itself (slow rays walk it) and, per triangle, the box of the leaf that lists it (the winner's verification).
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> which;
        which.reserve(nt);
        std::vector<float4> leafbox((size_t)nt * 2, make_float4(0, 0, 0, 0));
        for (const PtFastLeaf &l : leaves) {            // (leaf ranges ascend and do not overlap: checked above)
            const uint32_t first = l.ref & PT_LEAF_OFF_MASK;
            for (uint32_t k = 0; k < l.weight; k++) {
                which.push_back(first + k);
                leafbox[2 * (size_t)(first + k)] = make_float4(l.mn[0], l.mn[1], l.mn[2], 0.0f);
                leafbox[2 * (size_t)(first + k) + 1] = make_float4(l.mx[0], l.mx[1], l.mx[2], 0.0f);
            }
        }
        std::sort(which.begin(), which.end());
        own = own_leaves(opt, stream != nullptr, device, nt, (uint32_t)which.size(), b,
                         [&](uint32_t k_max, uint32_t limit, PtOwnTreeGpu &g) {
                             return own_tree_on_device(stream, device, tris, nt, which, leafbox, k_max, limit, b, g);
                         },
                         [&](OwnHostInputs &in) { in.tris = tris; in.which = &which; in.leafbox = &leafbox; in.ref_wnodes = &wnodes; return true; });
        if (own) b.hold(kLeafbox, std::move(leafbox));
        b.tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    std::vector<float4> fast;                   // a hierarchy rebuilt over the reference's leaves
    if (nested && leaves.size() >= 2 && !opt.keep_reference_tree && !own) {
        const auto t0 = std::chrono::steady_clock::now();
        // tree_builder = 2: on the device (gpu_tree.hip); the host builder when that is not wanted, not possible (ptmi_debug_image_stats
        // has no device) or refused
        uint32_t root = PT_REF_NONE, fast_depth = 0;
        const bool on_device = opt.tree_builder == 2u && stream && pt_build_fast_tree_gpu(leaves, fast, root, fast_depth, stream);
        if (!on_device) pt_build_fast_tree(leaves, fast, root, fast_depth);
        h.n_wnodes = (uint32_t)(fast.size() / 4); h.root_ref = root; h.depth = fast_depth;
        b.tree_builder_used = on_device ? 2u : 1u;
        b.tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // triangle images: v0, e1 = v1 - v0, e2 = v2 - v0 (pt.wgsl:128-129; one IEEE subtraction each)
    std::vector<float4> tripos((size_t)nt * 3);
    for (uint32_t i = 0; i < nt; i++) {
        const ptmi_triangle &t = tris[i];
        tripos[3 * (size_t)i + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], 0.0f);
        tripos[3 * (size_t)i + 1] = make_float4(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2], 0.0f);
        tripos[3 * (size_t)i + 2] = make_float4(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2], 0.0f);
    }
    {   // longest edge squared, in double; NaN / inf edges give 0 (no ray is "bounded" then)
        double emax2 = 0.0; bool finite = true;
        for (size_t k = 0; k < tripos.size(); k++) {
            if (k % 3 == 0) continue;
            const float4 &e = tripos[k];
            const double l2 = (double)e.x * e.x + (double)e.y * e.y + (double)e.z * e.z;
            if (!(l2 <= 1.7e308)) finite = false; else if (l2 > emax2) emax2 = l2;
        }
        const double k = !finite ? 0.0 : (emax2 > 0.0 ? std::ldexp(1.0, 98) / emax2 : 3.0e38);
        b.tri_safe_dsum = (float)(k < 3.0e38 ? k : 3.0e38);
    }
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint4> q;
        std::vector<uint32_t> leaf_stream;
        if (!fast.empty() && pt_quantize_tree(leaves, fast, tripos, q, leaf_stream, h.q_origin, h.q_scale, PT_QCACHE_NODES, b.q_top)) {
            h.quantised = 1u;
            b.hold(kQnodes, std::move(q)); b.hold(kLeafStream, std::move(leaf_stream));
        }
        b.tree_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!fast.empty()) b.hold(kWnodes, std::move(fast));
    b.hold(kRefWnodes, std::move(wnodes)); b.hold(kRefTripos, std::move(tripos));
    return PTMI_OK;
}

}  // namespace

// A scene prepared on the host (validation + traversal image: everything of an upload that does not depend on the device), and the
// caller's blobs it was made from. ptmi_upload_scene = prepare + install; ptmi_multi_upload_scene prepares ONCE and installs on N devices.
struct PtPrepared {
    Built b;                                 // the triangles, materials and lights included
    uint32_t nt, nm, nl;
    double build_ms;
    bool take_device_buffers = false;        // the one install may take b's device buffers instead of copying them (single device)
};

// The shade tables of a scene (pt_device.h): raw copies of the uploaded records, in the order k_shade stages them.
static std::vector<float4> shade_tables(const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                                        const ptmi_light *lights, uint32_t nl) {
    std::vector<float4> tab(pt_tab_mats_q(nm) + pt_tab_lights_q(nl), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    char *at = reinterpret_cast<char *>(tab.data());
    if (nm) std::memcpy(at, mats, (size_t)nm * sizeof(ptmi_material));
    at += pt_tab_mats_q(nm) * sizeof(float4);                                   // (behind the materials: the material of zeros)
    if (nl) std::memcpy(at, lights, (size_t)nl * sizeof(ptmi_light));
    at += (size_t)nl * sizeof(ptmi_light);
    for (uint32_t i = 0; i < nl; i++)
        if (lights[i].light_type == PTMI_LIGHT_EMISSIVE && lights[i].triangle_index < nt)
            std::memcpy(at + (size_t)i * sizeof(ptmi_triangle), &tris[lights[i].triangle_index], sizeof(ptmi_triangle));
    return tab;
}

// One buffer of a preparation on c's device, in *out: taken over (`take`, and it is on that device), else allocated and copied. An empty
// buffer gets 16 zeroed bytes.
static hipError_t place(const ptmi_ctx *c, HeldBuf &h, bool take, void **out) {
    if (h.dev && take && h.device == c->device) { *out = h.dev; h.dev = nullptr; return hipSuccess; }
    hipError_t e = hipMalloc(out, h.bytes ? h.bytes : 16);
    if (e != hipSuccess) return e;
    if (h.dev) return h.device == c->device ? hipMemcpy(*out, h.dev, h.bytes, hipMemcpyDeviceToDevice)
                                            : hipMemcpyPeer(*out, c->device, h.dev, h.device, h.bytes);
    return h.bytes ? hipMemcpy(*out, h.host, h.bytes, hipMemcpyHostToDevice) : hipMemset(*out, 0, 16);
}

PtPrepared *pt_prepare_scene(ptmi_ctx *c, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                             const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl, int *rc_out) {
    auto bad = [&](int rc) -> PtPrepared * { *rc_out = rc; return nullptr; };
    if (!c) return bad(PTMI_E_INVALID);
    if ((nt && !tris) || (nm && !mats) || (nn && !nodes) || (nl && !lights))
        return bad(fail(c, PTMI_E_INVALID, "NULL blob with a non-zero count"));
    if (hipSetDevice(c->device) != hipSuccess) return bad(fail(c, PTMI_E_HIP, "hipSetDevice(%d) failed", c->device));
    for (uint32_t i = 0; i < nl; i++) {
        if (lights[i].light_type > PTMI_LIGHT_POINT)
            return bad(fail(c, PTMI_E_INVALID, "light %u has unknown type %u", i, lights[i].light_type));
        if (lights[i].light_type == PTMI_LIGHT_EMISSIVE && lights[i].triangle_index >= nt)
            return bad(fail(c, PTMI_E_INVALID, "emissive light %u references triangle %u of %u", i, lights[i].triangle_index, nt));
    }
    const auto t_start = std::chrono::steady_clock::now();
    PtPrepared *p = new PtPrepared();
    int rc = build_image(c->opt, c->stream, c->device, tris, nt, nodes, nn, p->b, c->err);
    if (rc) { delete p; return bad(rc); }
    if (!p->b.buf[kTris].present) p->b.view(kTris, tris, (size_t)nt * sizeof(ptmi_triangle));     // (else the device copy)
    p->b.view(kMats, mats, (size_t)nm * sizeof(ptmi_material));
    p->b.view(kLights, lights, (size_t)nl * sizeof(ptmi_light));
    p->b.hold(kShadeTab, shade_tables(tris, nt, mats, nm, lights, nl));
    p->nt = nt; p->nm = nm; p->nl = nl;
    p->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    *rc_out = PTMI_OK;
    return p;
}
void pt_free_prepared(PtPrepared *p) { delete p; }

int pt_install_scene(ptmi_ctx *c, PtPrepared *prep) {
    if (!c || !prep) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    const auto t_start = clk::now();
    Built &b = prep->b;
    // Allocate and fill the new buffers first; the context keeps its previous scene until all of them exist. An empty buffer gets 16
    // zeroed bytes. Buffers the preparation made on a device are taken over (the one install on that device) or copied.
    const auto t_copy = clk::now();
    void *n[kSceneBufs] = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < kSceneBufs && e == hipSuccess; k++) {
        if (b.buf[k].present) e = place(c, b.buf[k], prep->take_device_buffers, &n[k]);
    }
    // while motion is on (ptmi_set_motion) the previous positions are re-made for the new scene: filled below, from its triangles
    if (e == hipSuccess && c->motion_on) {
        e = hipMalloc(&n[kMotionPrev], motion_prev_bytes(prep->nt));
        if (e == hipSuccess && !prep->nt) e = hipMemset(n[kMotionPrev], 0, motion_prev_bytes(0u));
    }
    if (e != hipSuccess) {
        for (void *&p : n) dfree(p);
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "scene upload failed: %s (the previous scene, if any, is still in place)", hipGetErrorString(e));
    }
    HIP_TRY(c, sync_all(c));                  // nothing in flight reads the old buffers any more
    for (int k = 0; k < kSceneBufs; k++) { dfree(c->buf[k]); c->buf[k] = n[k]; }
    void *const *d = c->buf;
    const ptmi_image_info &h = b.img;
    const bool own = h.leaves_used == 2u;
    DevScene &s = c->sc;
    s.tris = static_cast<const ptmi_triangle *>(d[kTris]); s.n_tris = prep->nt;
    s.mats = static_cast<const ptmi_material *>(d[kMats]); s.n_mats = prep->nm;
    s.lights = static_cast<const ptmi_light *>(d[kLights]); s.n_lights = prep->nl;
    s.ref_wnodes = static_cast<const float4 *>(d[kRefWnodes]); s.ref_root_ref = b.ref_root_ref; s.has_fast = d[kWnodes] ? 1u : 0u;
    s.wnodes = static_cast<const float4 *>(walked(d, kWnodes));
    s.n_wnodes = h.n_wnodes;
    s.tripos = static_cast<const float4 *>(walked(d, kTripos));
    s.ref_tripos = static_cast<const float4 *>(d[kRefTripos]);
    s.qnodes = static_cast<const uint4 *>(d[kQnodes]); s.leaf_stream = static_cast<const uint32_t *>(d[kLeafStream]);
    for (int k = 0; k < 3; k++) { s.q_origin[k] = h.q_origin[k]; s.q_scale[k] = h.q_scale[k]; }
    s.q_cached = b.q_top;
    s.tri_safe_dsum = b.tri_safe_dsum;
    for (int k = 0; k < 3; k++) {
        s.ref_root_min[k] = b.ref_root_min[k]; s.ref_root_max[k] = b.ref_root_max[k];
        s.root_min[k] = h.root_min[k]; s.root_max[k] = h.root_max[k];
    }
    s.root_ref = h.root_ref;
    s.own = own ? 1u : 0u;
    s.n_own_tris = own ? h.n_tris : 0u;
    s.tri_leafbox = static_cast<const float4 *>(d[kLeafbox]);
    s.wnodes16 = static_cast<const float4 *>(d[kWnodes16]); s.ref_wnodes16 = static_cast<const float4 *>(d[kRefWnodes16]);
    s.qnodes16 = static_cast<const uint4 *>(d[kQnodes16]);
    s.root_ref16 = b.root_ref16; s.ref_root_ref16 = b.ref_root_ref16;
    s.safe_origin = h.safe_origin;
    s.verify_stat = &c->d_counters[kCtVerifyFailed];
    s.self = c->d_scene;
    s.shade_tab = static_cast<const float4 *>(d[kShadeTab]);
    HIP_TRY(c, hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice));
    c->img = h;
    c->have_scene = true;
    c->n_ref_wnodes = (uint32_t)(b.buf[kRefWnodes].bytes / 64); c->tree_nested = b.nested;
    c->upd_planned = false; c->upd_ref_off.clear(); c->upd_off.clear(); c->upd = {}; c->reb = {};
    if (c->motion_on) {
        const int rc = motion_fill(c);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    // the alpha cutoff table belonged to the old scene's materials (its buffer went with the others above); the loops' arrays go too
    c->alpha_present = false; c->alpha_cutout = c->alpha_layers = 0u;
    c->blend_present = false; c->blend_count = c->blend_layers = c->blend_seed = 0u;        // ... and so did the blend table
    for (int k = kAlphaO; k <= kAlphaHits; k++) dfree(c->lane.buf[k]);
    lane_views(c->lane);
    groups_forget(c);                          // the group table named the old scene's triangles (its buffers went with the others above)
    skin_forget(c);                            // ... and so did the skin
    morph_forget(c);                           // ... and the morph
    c->st.leaves_used = h.leaves_used;
    c->st.leaf_tris_used = h.max_leaf_tris;
    c->st.tree_builder_used = b.tree_builder_used;
    c->st.upload_copy_ms = ms_since(t_copy);
    c->st.upload_tree_ms = b.tree_ms;
    c->st.upload_ms = prep->build_ms + ms_since(t_start);
    return PTMI_OK;
}

// ptmi_rebuild_tree's build (ptmi_ctx.h). The device builder reads the context's own buffers; the host builder's inputs are read back
// (at most 512 KB for the scenes that always take it). Nothing of the context changes.
int pt_host::rebuild_own_image(ptmi_ctx *c, const ptmi_options &opt, const uint32_t *d_which, uint32_t n_units, OwnRebuilt &out) {
    const uint32_t nt = c->sc.n_tris;
    void *const *d = c->buf;
    Built b;
    b.img = c->img;                                                  // (ref_depth stays; what follows is what build_image starts an own image from)
    b.img.quantised = 0u;
    for (int k = 0; k < 3; k++) b.img.q_origin[k] = b.img.q_scale[k] = 0.0f;
    b.ref_root_ref = c->sc.ref_root_ref;
    std::vector<ptmi_triangle> tris;
    std::vector<uint32_t> which;
    std::vector<float4> leafbox, ref_wnodes;
    hipError_t e = hipSuccess;
    auto fetch = [&](auto &v, size_t n, const void *from) {
        v.resize(n);
        if (n && e == hipSuccess) e = hipMemcpy(v.data(), from, n * sizeof(v[0]), hipMemcpyDeviceToHost);
    };
    const bool own = own_leaves(opt, true, c->device, nt, n_units, b,
        [&](uint32_t k_max, uint32_t limit, PtOwnTreeGpu &g) {
            return pt_build_own_tree_gpu(c->sc.tris, d_which, n_units, static_cast<const float4 *>(d[kLeafbox]), k_max, limit, c->stream, g);
        },
        [&](OwnHostInputs &in) {
            fetch(tris, nt, d[kTris]); fetch(which, n_units, d_which); fetch(leafbox, (size_t)nt * 2, d[kLeafbox]);
            fetch(ref_wnodes, (size_t)c->n_ref_wnodes * 4, d[kRefWnodes]);
            in.tris = tris.data(); in.which = &which; in.leafbox = &leafbox; in.ref_wnodes = &ref_wnodes;
            return e == hipSuccess;
        });
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, PTMI_E_HIP, "reading the scene back for the host builder failed: %s", hipGetErrorString(e)); }
    if (!own) return fail(c, PTMI_E_STATE, "the own-leaf builder refused the loaded triangles");      // (an update admits only finite ones)
    for (SceneBuf k : {kWnodes, kTripos, kQnodes, kWnodes16, kRefWnodes16, kQnodes16})
        if (b.buf[k].present && (e = place(c, b.buf[k], true, &out.buf[k])) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, PTMI_E_HIP, "placing the rebuilt image failed: %s", hipGetErrorString(e));
        }
    out.img = b.img; out.q_top = b.q_top; out.root_ref16 = b.root_ref16; out.ref_root_ref16 = b.ref_root_ref16;
    out.builder_used = b.tree_builder_used;
    return PTMI_OK;
}

extern "C" {

int ptmi_upload_scene(ptmi_ctx *c, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                      const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl) {
    int rc = PTMI_OK;
    PtPrepared *p = pt_prepare_scene(c, tris, nt, mats, nm, nodes, nn, lights, nl, &rc);
    if (!p) return rc;
    p->take_device_buffers = true;
    rc = pt_install_scene(c, p);
    pt_free_prepared(p);
    return rc;
}

int ptmi_debug_image_stats(const ptmi_triangle *tris, uint32_t nt, const ptmi_bvh_node *nodes, uint32_t nn, double out[8]) {
    if (!out || (nt && !tris) || (nn && !nodes)) return PTMI_E_INVALID;
    for (int i = 0; i < 8; i++) out[i] = 0.0;
    ptmi_options opt;
    default_options(opt);
    opt.leaves = 1;                                 // the image over the reference's leaves (ptmi_debug_build_image: the own one)
    Built b;
    int rc = build_image(opt, nullptr, -1, tris, nt, nodes, nn, b, g_create_err);     // host-only: never touches a device
    if (rc) return rc;
    const std::vector<float4> &fast_wnodes = b.vec<float4>(kWnodes), &tripos = b.vec<float4>(kRefTripos);
    const std::vector<uint4> &qnodes = b.vec<uint4>(kQnodes);
    const std::vector<uint32_t> &leaf_stream = b.vec<uint32_t>(kLeafStream);
    const float *q_origin = b.img.q_origin, *q_scale = b.img.q_scale;
    out[0] = (double)(fast_wnodes.size() / 4); out[2] = fast_wnodes.empty() ? 0.0 : (double)b.img.depth;
    out[3] = (double)(qnodes.size() / 2); out[4] = (double)leaf_stream.size();
    if (qnodes.empty()) return PTMI_OK;
    // every quantised child box, decoded with the kernel's own fmaf, must contain the exact child box it stands for
    double viol = 0.0, infl = 0.0; size_t boxes = 0, leaves = 0, bad_hdr = 0;
    auto area = [](const float *lo, const float *hi) {
        double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return 2.0 * (x * y + y * z + z * x);
    };
    // the quantised nodes are renumbered (top levels first): walk both images together from their roots
    std::vector<std::pair<uint32_t, uint32_t>> todo;       // (node of the exact image, node of the quantised image)
    todo.push_back({0u, 0u});
    size_t visited = 0;
    while (!todo.empty()) {
        const uint32_t i = todo.back().first, qi = todo.back().second;
        todo.pop_back();
        if ((size_t)qi * 2 + 1 >= qnodes.size() || (size_t)i * 4 + 3 >= fast_wnodes.size()) { bad_hdr++; continue; }
        visited++;
        const float4 *w = &fast_wnodes[(size_t)i * 4];
        const float lo[2][3] = {{w[0].x, w[0].y, w[0].z}, {w[1].z, w[1].w, w[2].x}};
        const float hi[2][3] = {{w[0].w, w[1].x, w[1].y}, {w[2].y, w[2].z, w[2].w}};
        uint32_t refs[2]; std::memcpy(&refs[0], &w[3].x, 4); std::memcpy(&refs[1], &w[3].y, 4);
        for (int ch = 0; ch < 2; ch++) {
            const uint4 q = qnodes[(size_t)qi * 2 + ch];
            const uint32_t pl[6] = {q.x & 0xFFFFu, q.x >> 16, q.y & 0xFFFFu, q.y >> 16, q.z & 0xFFFFu, q.z >> 16};   // lo.xyz, hi.xyz
            float dlo[3], dhi[3];
            for (int k = 0; k < 3; k++) {
                dlo[k] = std::fmaf(q_scale[k], (float)pl[k], q_origin[k]);
                dhi[k] = std::fmaf(q_scale[k], (float)pl[3 + k], q_origin[k]);
                if (!(dlo[k] <= lo[ch][k]) || !(dhi[k] >= hi[ch][k])) viol += 1.0;
            }
            const double a0 = area(lo[ch], hi[ch]);
            if (a0 > 0.0) { infl += area(dlo, dhi) / a0 - 1.0; boxes++; }
            if (refs[ch] & PT_REF_LEAF) {
                leaves++;
                if (!(q.w & PT_REF_LEAF)) { bad_hdr++; continue; }
                const uint32_t *h = &leaf_stream[q.w & ~PT_REF_LEAF];
                float hl[3], hh[3]; std::memcpy(hl, h, 12); std::memcpy(hh, h + 4, 12);
                const uint32_t first = refs[ch] & PT_LEAF_OFF_MASK, cnt = ((refs[ch] >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u;
                bool ok = h[3] == first && h[7] == cnt;
                for (int k = 0; k < 3; k++) ok = ok && hl[k] == lo[ch][k] && hh[k] == hi[ch][k];
                for (uint32_t t = 0; t < cnt && ok; t++)
                    for (int j = 0; j < 3; j++) {
                        const float4 &v = tripos[3 * (size_t)(first + t) + j];
                        float g[3]; std::memcpy(g, h + 8 + 9 * t + 3 * j, 12);
                        ok = ok && std::memcmp(&g[0], &v.x, 4) == 0 && std::memcmp(&g[1], &v.y, 4) == 0 && std::memcmp(&g[2], &v.z, 4) == 0;
                    }
                if (!ok) bad_hdr++;
            } else if (q.w & PT_REF_LEAF) bad_hdr++;
            else {
                // an inner box is the exact union of its two children's boxes (what makes any topology equivalent, §3.2)
                if ((size_t)refs[ch] * 4 + 3 < fast_wnodes.size()) {
                    const float4 *cw = &fast_wnodes[(size_t)refs[ch] * 4];
                    const float clo[3] = {std::min(cw[0].x, cw[1].z), std::min(cw[0].y, cw[1].w), std::min(cw[0].z, cw[2].x)};
                    const float chi[3] = {std::max(cw[0].w, cw[2].y), std::max(cw[1].x, cw[2].z), std::max(cw[1].y, cw[2].w)};
                    for (int k = 0; k < 3; k++) if (clo[k] != lo[ch][k] || chi[k] != hi[ch][k]) { bad_hdr++; break; }
                }
                todo.push_back({refs[ch], q.w});
            }
        }
    }
    if (visited != qnodes.size() / 2) bad_hdr++;          // every node reached exactly once (a tree: no node can be reached twice)
    out[1] = (double)leaves; out[5] = viol; out[6] = boxes ? infl / (double)boxes : 0.0; out[7] = (double)bad_hdr;
    return PTMI_OK;
}

int ptmi_debug_build_image(const ptmi_triangle *tris, uint32_t nt, const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_options *opt,
                           ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12, float *leafbox8) {
    if (!info || (nt && !tris) || (nn && !nodes)) return PTMI_E_INVALID;
    std::memset(info, 0, sizeof *info);
    ptmi_options o;
    default_options(o);
    if (opt) { o.leaves = opt->leaves; o.leaf_tris = opt->leaf_tris; o.keep_reference_tree = opt->keep_reference_tree; }
    Built b;
    int rc = build_image(o, nullptr, -1, tris, nt, nodes, nn, b, g_create_err);       // host-only: never touches a device
    if (rc) return rc;
    *info = b.img;
    const struct { const HeldBuf &from; void *to; } out[] = {
        {walked(b.buf, kWnodes), wnodes16}, {b.buf[kQnodes], qnodes8}, {walked(b.buf, kTripos), tripos12}, {b.buf[kLeafbox], leafbox8}};
    for (const auto &x : out) if (x.to && x.from.bytes) std::memcpy(x.to, x.from.host, x.from.bytes);
    return PTMI_OK;
}

int ptmi_debug_read_image(ptmi_ctx *c, ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12, float *leafbox8) {
    if (!c || !info) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    *info = c->img;
    if (!c->have_scene) return PTMI_OK;
    void *const *d = c->buf;
    const struct { const void *from; void *to; size_t bytes; } out[] = {
        {walked(d, kWnodes), wnodes16, (size_t)info->n_wnodes * 64},
        {d[kQnodes], qnodes8, info->quantised ? (size_t)info->n_wnodes * 32 : 0},
        {walked(d, kTripos), tripos12, (size_t)info->n_tris * 48},
        {d[kLeafbox], leafbox8, info->leaves_used == 2 ? (size_t)c->sc.n_tris * 32 : 0}};
    for (const auto &x : out) if (x.to && x.bytes) HIP_TRY(c, hipMemcpy(x.to, x.from, x.bytes, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
