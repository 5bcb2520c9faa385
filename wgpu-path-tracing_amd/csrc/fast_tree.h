// fast_tree.h — the hierarchies built at upload and their quantised images: the FAST tree over the reference's leaves and the OWN tree
// over the triangles (host: fast_tree.hip; device: gpu_tree.hip, own_tree_gpu.hip), and the two quantisers (quantise.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#ifndef PT_OWN_C_BOX
#define PT_OWN_C_BOX 1.0             /* own leaves' cost model: a box-pair step (the unit) */
#endif
#ifndef PT_OWN_C_TRI
#define PT_OWN_C_TRI 0.9             /* ... one triangle test (54 against ~60 vector instructions) */
#endif
#ifndef PT_OWN_C_OPEN
#define PT_OWN_C_OPEN 0.35           /* ... opening a leaf (its entry leaves the lane's list, the loop is set up, a share of a vote) */
#endif
#ifndef PT_OWN_SLIVER
#define PT_OWN_SLIVER 16.0           /* own leaves: a triangle whose longest edge squared exceeds this x |e1 x e2| is a SLIVER */
#endif

// Slivers (pt_own_sliver) enter the own hierarchy with the box of their REFERENCE leaf added to their own. Moller-Trumbore's (u, v) lose
// accuracy as 1 / (sin of the triangle's smallest angle x sin of the ray's angle to its plane): for a thin triangle it can accept a
// ray that passes far outside the triangle's padded box while the reference still tests the triangle (its leaf box passes), and a
// hierarchy over the triangles' own boxes would not (tests/test_own_leaves_grazing_host.py: ratios of 100 and up, at any angle). Through
// the leaf box the own leaves test such a triangle whenever the reference does, whatever the triangle test computes. Every triangle
// cannot take that path — the leaf boxes are what the own leaves are there to avoid (Cornell: 9.2 triangle tests per closest-hit ray
// instead of 2.8, more than leaves = 1) — so a non-sliver still relies on the padding, which rays within ~1e-3 rad of its plane can
// defeat (measured rate). No triangle of the benchmark scenes is a sliver (the largest ratio there is 5.5).
// Squares only (no square root), products and sums in double without contraction: both builders decide alike.
__host__ __device__ inline bool pt_own_sliver(const float *a, const float *b, const float *c) {
#pragma clang fp contract(off)
    const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
    const double e2[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
    const double e3[3] = {(double)c[0] - b[0], (double)c[1] - b[1], (double)c[2] - b[2]};
    const double x = e1[1] * e2[2] - e1[2] * e2[1], y = e1[2] * e2[0] - e1[0] * e2[2], z = e1[0] * e2[1] - e1[1] * e2[0];
    const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
    const double l3 = e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2];
    const double longest = l1 > l2 ? (l1 > l3 ? l1 : l3) : (l2 > l3 ? l2 : l3);
    return longest * longest > (PT_OWN_SLIVER * PT_OWN_SLIVER) * (x * x + y * y + z * z);
}

struct PtFastLeaf {
    float mn[3], mx[3];     // the leaf's own box, as stored in the reference node
    uint32_t ref;           // PT_REF_LEAF | (count-1) << 26 | first triangle
    uint32_t weight;        // triangle count (SAH weight)
};

// wnodes: 4 float4 per wide node in preorder (layout of pt_device.h); root_ref: wide-node index, or the
// leaf reference when there is a single leaf; depth: levels including the leaves.
void pt_build_fast_tree(const std::vector<PtFastLeaf> &leaves, std::vector<float4> &wnodes, uint32_t &root_ref,
                        uint32_t &depth);

// The same kind of hierarchy built on the device `s` belongs to (gpu_tree.hip: Morton-order linear BVH; ptmi_options.tree_builder = 2).
// Synchronises the stream. false: could not (allocation failure, non-finite centroids, more than 60 levels) — the caller builds on the host.
bool pt_build_fast_tree_gpu(const std::vector<PtFastLeaf> &leaves, std::vector<float4> &wnodes, uint32_t &root_ref, uint32_t &depth,
                            hipStream_t s);

// Quantised image of that hierarchy for the global traversal variant (quantise.hip; layout: traverse.hip, QuantMem).
//   qnodes      2 uint4 per wide node: child boxes as 16-bit plane numbers on the grid origin + k * scale, rounded outward
//               (wide_node.h pt_quantise_child: verified with the same fmaf the kernel evaluates), child references (leaf:
//               PT_REF_LEAF | dword offset into `stream`)
//   stream      per leaf: exact box (the reference node's), first triangle, count, then v0, e1, e2 of each triangle (9 dwords)
// tripos: 3 float4 per triangle (v0, e1, e2), indexed by triangle. Returns false when the hierarchy cannot be quantised
// (non-finite boxes, a stream beyond 2^31 dwords); the caller then keeps the exact image.
bool pt_quantize_tree(const std::vector<PtFastLeaf> &leaves, const std::vector<float4> &wnodes, const std::vector<float4> &tripos,
                      std::vector<uint4> &qnodes, std::vector<uint32_t> &stream, float origin[3], float scale[3],
                      uint32_t top_nodes, uint32_t &n_top);
// The quantised nodes are renumbered: the first n_top (<= top_nodes) are the top of the tree in breadth-first order (the
// kernel keeps them in LDS), the others follow in their preorder. The root stays node 0.

// ---- the library's OWN leaves (ptmi_options.leaves = 2) ------------------------------------------------------
// A full-sweep SAH hierarchy over the TRIANGLES themselves (bvh.ts:86-127 cuts leaves of <= 4 triangles from 11 equal-count candidates
// on one axis, and a ray then tests ~10 triangles where ~2.5 suffice), built down to single triangles and collapsed bottom-up into
// leaves of at most `max_leaf` triangles wherever the surface-area estimate says the leaf is cheaper than the box step.
//   wnodes   4 float4 per wide node, preorder; every child box PADDED outward by `pad`, so that the kernels' fused slab test
//            fma(bound, 1/d, -o/d) accepts every ray the exact box would (for origins within `safe_origin` of the coordinate origin)
//   tripos   3 float4 per listed triangle in LEAF order: (v0, bits(ORIGINAL triangle index)), (e1, 0), (e2, 0); a leaf reference
//            is PT_REF_LEAF | (count - 1) << 26 | position of its first triangle in this array
struct PtOwnTreeHeader {               // what both builders report beside the buffers
    uint32_t root_ref = 0xFFFFFFFFu, depth = 0, n_leaves = 0, max_leaf_tris = 0;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};     // padded
    float pad = 0.0f, safe_origin = 0.0f;
};
struct PtOwnTree : PtOwnTreeHeader {
    std::vector<float4> wnodes, tripos;
};
struct ptmi_triangle;
// which: the original indices of the triangles to build over (those some reachable reference leaf lists), ascending.
// leafbox: per ORIGINAL triangle index, (min.xyz, 0), (max.xyz, 0) of the reference leaf that lists it (added to a sliver's box).
// depth_limit: most levels (leaves included) the tree may have. false: a vertex is not finite (the caller keeps the reference's leaves).
bool pt_build_own_tree(const ptmi_triangle *tris, const std::vector<uint32_t> &which, const std::vector<float4> &leafbox,
                       uint32_t max_leaf, uint32_t depth_limit, PtOwnTree &out);
// The same tree built on the device `s` belongs to (own_tree_gpu.hip; ptmi_options.tree_builder = 2), from the device copy of the
// triangles: Morton-sorted clusters merged by PLOC, collapsed with the host's cost model, emitted and quantised in place. The device
// buffers have the layouts of PtOwnTree::wnodes / tripos and of pt_quantize_nodes (qnodes: NULL when the scene has no quantised image);
// pad, safe_origin and the root box equal the host build's bit for bit (they depend on the triangle set only). Synchronises the stream.
// false: could not (a non-finite vertex, more than depth_limit levels, an allocation or HIP failure); nothing is left allocated.
struct PtOwnTreeGpu : PtOwnTreeHeader {
    float4 *wnodes = nullptr, *tripos = nullptr;
    uint4 *qnodes = nullptr;
    uint32_t n_wnodes = 0, n_tris = 0, q_top = 0;
    bool quantised = false;
    float q_origin[3] = {0, 0, 0}, q_scale[3] = {0, 0, 0};
    void release();                        // frees the device buffers (hipFree) and resets the fields
};
bool pt_build_own_tree_gpu(const ptmi_triangle *d_tris, const std::vector<uint32_t> &which, const std::vector<float4> &leafbox,
                           uint32_t max_leaf, uint32_t depth_limit, hipStream_t s, PtOwnTreeGpu &out);
// ... with the unit list (n_units entries) and the leaf boxes in device memory as well (a rebuild has them there: scene_rebuild.hip); the
// entry above copies its vectors to the device and calls this one. Nothing per triangle crosses the bus.
bool pt_build_own_tree_gpu(const ptmi_triangle *d_tris, const uint32_t *d_which, uint32_t n_units, const float4 *d_leafbox,
                           uint32_t max_leaf, uint32_t depth_limit, hipStream_t s, PtOwnTreeGpu &out);
// The 16-bit grid of both quantisers and of the device builder over the bounds [mn, mx]: origin = mn, the smallest scale whose last plane reaches mx (checked
// with fmaf). false: the bounds are not finite.
bool pt_quant_grid(const float mn[3], const float mx[3], float origin[3], float scale[3]);
// Quantised nodes of any wide-node hierarchy whose leaf references are to stay as they are (own leaves): 2 uint4 per node as in
// pt_quantize_tree, numbered with the top n_top <= top_nodes nodes first in breadth-first order, the rest in preorder.
bool pt_quantize_nodes(const std::vector<float4> &wnodes, std::vector<uint4> &qnodes, float origin[3], float scale[3],
                       uint32_t top_nodes, uint32_t &n_top);
