// quantise.hip — host code: a wide-node hierarchy quantised onto one 16-bit grid over the scene (declarations: fast_tree.h).
//
// Both quantised images hold 2 uint4 per wide node: per child three words of 16-bit plane numbers and the child's reference
// (wide_node.h pt_quantise_child: rounded outward, checked with the fmaf the kernels decode with). The nodes are renumbered: the top of
// the tree breadth-first at the front (the kernels keep those in LDS), everything else in its preorder; the root stays node 0.
//   over the reference's leaves (leaves = 1; pt_quantize_tree, walked by traverse.hip)   a leaf child's reference becomes PT_REF_LEAF |
//       the dword offset of its record in the leaf stream: the reference node's exact box, first triangle and count, then v0, e1, e2 of
//       each triangle, in the order the leaves hang off the preorder nodes
//   over the library's own leaves (leaves = 2; pt_quantize_nodes, walked by traverse_own.hip)   leaf references stay as they are
// The device builder quantises its own tree with the same grid and the same child function (own_tree_gpu.hip k_quantise).
//
// One grid for the whole scene suits scenes whose boxes are not many orders of magnitude smaller than the scene. Where they are (a
// chain of boxes shrinking geometrically), the rounded boxes would admit far more rays than the exact ones: same results, much more
// work. Such scenes (mean relative growth of the child boxes' surface area above 0.25) keep the exact image.
#include "fast_tree.h"
#include "pt_device.h"
#include "wide_node.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>

bool pt_quant_grid(const float mn[3], const float mx[3], float origin[3], float scale[3]) {
    for (int k = 0; k < 3; k++) {
        origin[k] = mn[k];
        const double ext = (double)mx[k] - (double)mn[k];
        float s = (float)(ext / 65535.0);
        if (!std::isfinite(s)) return false;
        if (ext > 0.0) {
            if (!(s > 0.0f)) s = std::numeric_limits<float>::denorm_min();
            int guard = 0;
            while (std::fmaf(s, 65535.0f, origin[k]) < mx[k] && guard++ < 64) s = std::nextafterf(s, INFINITY);   // the last plane reaches the far side
            if (std::fmaf(s, 65535.0f, origin[k]) < mx[k]) return false;
        }
        scale[k] = s;
    }
    return true;
}

namespace {

// The grid over [mn, mx], the renumbering, and the nodes filled in parallel. leaf_ref(node, side, ref, out): what a leaf child's
// reference becomes (it may write what belongs to that leaf; false: the leaf is not valid). false: no grid, an invalid leaf, or the
// grid is too coarse for this scene's boxes; qnodes is then empty (origin, scale and n_top keep what was computed).
template <class LeafRef>
bool quantise(const std::vector<float4> &wnodes, const float mn[3], const float mx[3], uint32_t top_nodes, LeafRef leaf_ref,
              std::vector<uint4> &qnodes, float origin[3], float scale[3], uint32_t &n_top) {
    const size_t n_nodes = wnodes.size() / 4;
    if (!pt_quant_grid(mn, mx, origin, scale)) return false;
    const PtQuantGrid g{{origin[0], origin[1], origin[2]}, {scale[0], scale[1], scale[2]}};
    // new numbers: the top of the tree breadth-first (root first), then everything else in preorder
    std::vector<uint32_t> renum(n_nodes, PT_REF_NONE);
    {
        std::vector<uint32_t> bfs; bfs.reserve(top_nodes);
        bfs.push_back(0u);
        for (size_t h = 0; h < bfs.size() && bfs.size() < top_nodes; h++)
            for (int c = 0; c < 2 && bfs.size() < top_nodes; c++) {
                const uint32_t ref = pt_wide_ref(&wnodes[(size_t)bfs[h] * 4], c);
                if (!(ref & PT_REF_LEAF)) bfs.push_back(ref);
            }
        for (size_t k = 0; k < bfs.size(); k++) renum[bfs[k]] = (uint32_t)k;
        n_top = (uint32_t)bfs.size();
        uint32_t next = n_top;
        for (size_t i = 0; i < n_nodes; i++) if (renum[i] == PT_REF_NONE) renum[i] = next++;
    }
    qnodes.resize(n_nodes * 2);
    auto fill = [&](size_t i0, size_t i1, double &growth, size_t &grown, char &ok) {
        for (size_t i = i0; i < i1; i++)
            for (int c = 0; c < 2; c++) {
                const PtWideChild ch = pt_wide_child(&wnodes[i * 4], c);
                uint32_t ref = ch.ref;
                if (!(ref & PT_REF_LEAF)) ref = renum[ref];
                else if (!leaf_ref(i, c, ch.ref, ref)) { ok = 0; continue; }
                const PtQuantChild q = pt_quantise_child(g, ch.lo, ch.hi, ref);
                qnodes[(size_t)renum[i] * 2 + c] = q.q;
                if (q.grown) { growth += q.growth; grown++; }
            }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_thr = n_nodes < 65536 ? 1 : std::min<size_t>(16, hw ? hw : 1);
    std::vector<double> gr(n_thr, 0.0); std::vector<size_t> gn(n_thr, 0); std::vector<char> oks(n_thr, 1);
    {
        std::vector<std::thread> pool;
        for (size_t t = 1; t < n_thr; t++)
            pool.emplace_back([&, t] { fill(n_nodes * t / n_thr, n_nodes * (t + 1) / n_thr, gr[t], gn[t], oks[t]); });
        fill(0, n_nodes / n_thr, gr[0], gn[0], oks[0]);
        for (auto &th : pool) th.join();
    }
    double growth = 0.0; size_t grown = 0;       // mean relative growth of the child boxes' surface area
    bool ok = true;
    for (size_t t = 0; t < n_thr; t++) { growth += gr[t]; grown += gn[t]; ok = ok && oks[t]; }
    if (!ok || (grown && growth / (double)grown > 0.25)) { qnodes.clear(); return false; }
    return true;
}

}  // namespace

bool pt_quantize_nodes(const std::vector<float4> &wnodes, std::vector<uint4> &qnodes, float origin[3], float scale[3],
                       uint32_t top_nodes, uint32_t &n_top) {
    qnodes.clear(); n_top = 0;
    const size_t n_nodes = wnodes.size() / 4;
    if (n_nodes == 0) return false;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};      // of the child boxes
    for (size_t i = 0; i < n_nodes; i++)
        for (int c = 0; c < 2; c++) {
            const PtWideChild ch = pt_wide_child(&wnodes[i * 4], c);
            for (int k = 0; k < 3; k++) {
                if (!std::isfinite(ch.lo[k]) || !std::isfinite(ch.hi[k]) || ch.lo[k] > ch.hi[k]) return false;
                mn[k] = std::min(mn[k], ch.lo[k]); mx[k] = std::max(mx[k], ch.hi[k]);
            }
        }
    return quantise(wnodes, mn, mx, top_nodes, [](size_t, int, uint32_t, uint32_t &) { return true; }, qnodes, origin, scale, n_top);
}

bool pt_quantize_tree(const std::vector<PtFastLeaf> &leaves, const std::vector<float4> &wnodes, const std::vector<float4> &tripos,
                      std::vector<uint4> &qnodes, std::vector<uint32_t> &stream, float origin[3], float scale[3],
                      uint32_t top_nodes, uint32_t &n_top) {
    qnodes.clear(); stream.clear(); n_top = 0;
    const size_t n_nodes = wnodes.size() / 4;
    if (n_nodes == 0 || leaves.empty()) return false;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};      // of the leaves' boxes
    size_t n_tri_refs = 0;
    for (const PtFastLeaf &l : leaves) {
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(l.mn[k]) || !std::isfinite(l.mx[k]) || l.mn[k] > l.mx[k]) return false;
            mn[k] = std::min(mn[k], l.mn[k]); mx[k] = std::max(mx[k], l.mx[k]);
        }
        n_tri_refs += l.weight;
    }
    if (leaves.size() * 8 + n_tri_refs * 9 >= (1ull << 31)) return false;
    // the leaf stream, in the order the leaves hang off the preorder nodes (neighbours in the tree are neighbours in memory): every
    // leaf child is assigned its place here (sequential, two words per node); the parallel fill then writes the records
    const size_t n_tris = tripos.size() / 3;
    std::vector<uint32_t> leaf_of_first(n_tris, PT_REF_NONE);         // a leaf is identified by its first triangle
    for (size_t i = 0; i < leaves.size(); i++) {
        const uint32_t first = leaves[i].ref & PT_LEAF_OFF_MASK;
        if (first >= n_tris) return false;
        leaf_of_first[first] = (uint32_t)i;
    }
    auto count_of = [](uint32_t ref) { return ((ref >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u; };
    std::vector<uint32_t> child_off(n_nodes * 2, 0u);
    size_t total = 0;
    for (size_t i = 0; i < n_nodes; i++)
        for (int c = 0; c < 2; c++) {
            const uint32_t ref = pt_wide_ref(&wnodes[i * 4], c);
            if (ref & PT_REF_LEAF) { child_off[i * 2 + c] = (uint32_t)total; total += 8 + 9 * (size_t)count_of(ref); }
        }
    if (total >= (1ull << 31)) return false;
    stream.assign(total, 0u);
    auto leaf_record = [&](size_t i, int c, uint32_t ref, uint32_t &out) {
        const uint32_t first = ref & PT_LEAF_OFF_MASK, cnt = count_of(ref);
        const uint32_t li = first < n_tris ? leaf_of_first[first] : PT_REF_NONE;
        if (li == PT_REF_NONE || leaves[li].ref != ref || (size_t)first + cnt > n_tris) return false;
        const PtFastLeaf &l = leaves[li];
        uint32_t *h = &stream[child_off[i * 2 + c]];
        std::memcpy(h, l.mn, 12); h[3] = first; std::memcpy(h + 4, l.mx, 12); h[7] = cnt;
        for (uint32_t t = 0; t < cnt; t++)
            for (int j = 0; j < 3; j++) std::memcpy(h + 8 + 9 * t + 3 * j, &tripos[3 * (size_t)(first + t) + j], 12);
        out = PT_REF_LEAF | child_off[i * 2 + c];
        return true;
    };
    if (quantise(wnodes, mn, mx, top_nodes, leaf_record, qnodes, origin, scale, n_top)) return true;
    stream.clear();
    return false;
}
