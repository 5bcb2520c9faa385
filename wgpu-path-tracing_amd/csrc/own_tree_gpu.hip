// own_tree_gpu.hip — the library's OWN-leaf hierarchy (ptmi_options.leaves = 2) built on the device (ptmi_options.tree_builder = 2).
//
// It produces what pt_build_own_tree + pt_quantize_nodes produce on the host (fast_tree.hip, quantise.hip: the same layouts, the same
// padding, and the quantisation of wide_node.h itself), over another topology. Any topology is allowed: the
// kernels break ties by the lowest triangle index and verify every winner against its reference leaf's box, so only the work per ray
// depends on the tree.
//
//   units     one box per listed triangle, the host's (pt_box.h pt_unit_box); |coordinate| of the unit boxes max-reduced for the
//             padding (exact in f32)
//   PLOC      Morton codes of the unit centroids, made unique by the unit's index and radix-sorted (hipCUB); then repeatedly: every
//             cluster's nearest neighbour within +-PT_PLOC_RADIUS sorted positions (smallest surface area of the union, ties to the
//             lower position), mutual pairs merged into a new node at the lower position, survivors compacted in order by a prefix sum
//             (Meister & Bittner 2018). The key (area, lower position, higher position) is symmetric, so the globally smallest pair is
//             always mutual and every pass merges at least once.
//   collapse  bottom-up with one arrival counter per node (agent-scope release / acquire hand-off): the second thread to arrive
//             computes the host's cost model (fast_tree.hip, Collapse) from both children's stored values, so the result does not
//             depend on the order of arrival
//   emit      every node walks up to the root summing the offsets its ancestors stored for it: its preorder number among the
//             surviving inner nodes, its first position in leaf order, its level. Inner nodes write their wide node (child boxes
//             padded outward by the host's pt_box.h pt_pad_lower / pt_pad_upper), units write their triangle (v0, bits(original index)), e1, e2
//   quantise  the host's grid (quantise.hip pt_quant_grid) from the min / max of the padded boxes; the top PT_QCACHE_NODES nodes
//             breadth-first at the front, the others in preorder; every child through the host's own wide_node.h pt_quantise_child
//
// The build reads the triangles, the unit list and the leaf boxes from device memory: an upload copies the latter two there first, a
// rebuild (scene_rebuild.hip) has them there already. Both go through one body.
// Every step is deterministic: the same scene gives the same bytes on every run and every device. Scratch is sized from the scene and
// owned by the scope of one build (pt_dev_build.h DevScratch); any failure returns false and the caller builds on the host.
#include "pt_box.h"
#include "pt_dev_build.h"
#include "pt_device.h"
#include "ptmi_layout.h"

#include <chrono>
#include <cmath>
#include <vector>

#ifndef PT_PLOC_RADIUS
#define PT_PLOC_RADIUS 16            /* neighbours searched on each side of a cluster (sorted positions) */
#endif

namespace {

constexpr int TB = 256;
constexpr int R = PT_PLOC_RADIUS;
constexpr int kMaxPasses = 1024;     // PLOC passes before the build is refused (a backstop: real scenes take 40 - 70)

struct Red {                          // reductions of the build, zeroed before it
    uint32_t biggest;                 // bits of max |coordinate| over the unit boxes (non-negative floats order as integers)
    uint32_t bad;                     // a non-finite coordinate
    uint32_t cmin[3], cmax[3];        // ord() of the unit centroids' bounds
    uint32_t depth, max_leaf, n_top;
    uint32_t ploc_depth;              // levels of the deepest cluster so far (a unit: 1)
    uint32_t qmin[3], qmax[3];        // ord() of the padded child boxes' bounds
};

__global__ void k_units(uint32_t n, const ptmi_triangle *__restrict__ tris, const uint32_t *__restrict__ which,
                        const float4 *__restrict__ leafbox, Box6 *__restrict__ box, Red *red) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const ptmi_triangle &t = tris[which[i]];
    const PtUnitBox u = pt_unit_box(t.v0, t.v1, t.v2, [&] { return pt_leafbox_row(leafbox, which[i]); });
    box[i] = u.box;
    if (u.bad) { atomicOr(&red->bad, 1u); return; }
    atomicMax(&red->biggest, u.biggest);
    for (int k = 0; k < 3; k++) {
        const uint32_t c = pt_ord(0.5f * u.box.mn[k] + 0.5f * u.box.mx[k]);
        atomicMin(&red->cmin[k], c); atomicMax(&red->cmax[k], c);
    }
}

__global__ void k_morton(uint32_t n, const Box6 *__restrict__ box, float3 lo, float3 inv, unsigned long long *__restrict__ keys) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const Box6 b = box[i];
    keys[i] = ((unsigned long long)pt_morton30(b.mn, b.mx, lo, inv) << 32) | i;
}

__global__ void k_first_clusters(uint32_t n, const unsigned long long *__restrict__ keys, uint32_t *__restrict__ clu) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i < n) clu[i] = (uint32_t)keys[i];               // low 32 bits: the unit
}

// nearest neighbour of every cluster within +-R positions; the block's boxes and its halo are staged in LDS
__global__ void __launch_bounds__(TB) k_nearest(uint32_t m, const uint32_t *__restrict__ clu, const Box6 *__restrict__ box,
                                                 uint32_t *__restrict__ nn) {
    __shared__ Box6 s[TB + 2 * R];
    const int base = (int)(blockIdx.x * TB) - R;
    for (int k = threadIdx.x; k < TB + 2 * R; k += TB) {
        const int j = base + k;
        if (j >= 0 && j < (int)m) s[k] = box[clu[j]];
    }
    __syncthreads();
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= (int)m) return;
    const Box6 me = s[threadIdx.x + R];
    double best = INFINITY; int bj = -1;
    const int j0 = max(0, i - R), j1 = min((int)m - 1, i + R);
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        const double a = pt_box_area(pt_unite(me, s[j - base]));
        if (a < best || bj < 0) { best = a; bj = j; }              // ascending j, strict <: ties go to the lower position
    }
    nn[i] = (uint32_t)bj;
}

// flags: high word = this position creates a node (the lower end of a mutual pair), low word = it survives
__global__ void k_mark(uint32_t m, const uint32_t *__restrict__ nn, unsigned long long *__restrict__ flags) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i > m) return;
    if (i == m) { flags[i] = 0ull; return; }
    const uint32_t j = nn[i];
    const bool mutual = nn[j] == i;
    flags[i] = mutual ? (i < j ? ((1ull << 32) | 1ull) : 0ull) : 1ull;
}

__global__ void k_merge(uint32_t m, uint32_t n, uint32_t first_new, const uint32_t *__restrict__ clu, const uint32_t *__restrict__ nn,
                        const unsigned long long *__restrict__ flags, const unsigned long long *__restrict__ ex, Box6 *__restrict__ box,
                        uint2 *__restrict__ child, uint32_t *__restrict__ parent, uint8_t *__restrict__ level, uint32_t *__restrict__ out,
                        Red *red) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= m) return;
    const unsigned long long f = flags[i];
    if (!(f & 1ull)) return;
    const unsigned long long e = ex[i];
    uint32_t node = clu[i];
    if (f >> 32) {
        const uint32_t a = clu[i], b = clu[nn[i]];
        node = first_new + (uint32_t)(e >> 32);
        child[node - n] = make_uint2(a, b);
        box[node] = pt_unite(box[a], box[b]);
        parent[a] = node; parent[b] = node;
        const uint32_t lv = 1u + max(a < n ? 1u : (uint32_t)level[a - n], b < n ? 1u : (uint32_t)level[b - n]);
        level[node - n] = (uint8_t)min(lv, 255u);                      // (the build is refused long before 255)
        atomicMax(&red->ploc_depth, lv);
    }
    out[(uint32_t)e] = node;
}

struct Step { uint32_t parent, pre, tri, parent_leaf; };   // what a node adds on its way up: see k_emit

// bottom-up: one thread per unit; the second to arrive at a node evaluates it
__global__ void k_collapse(uint32_t n, uint32_t max_leaf, double c_box, double c_tri, double c_open, const Box6 *__restrict__ box,
                           const uint2 *__restrict__ child, const uint32_t *__restrict__ parent, uint32_t *__restrict__ arrived,
                           uint32_t *__restrict__ cnt, uint32_t *__restrict__ icnt, double *__restrict__ cost,
                           uint32_t *__restrict__ leafy, Step *__restrict__ step) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= n) return;
    cnt[v] = 1u; icnt[v] = 0u; cost[v] = c_open + c_tri; leafy[v] = 1u;
    uint32_t node = parent[v];
    while (node != PT_REF_NONE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");           // this thread's stores before its ticket
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&arrived[node - n], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // the other child's stores are visible from here on
        const uint2 ch = child[node - n];
        const Box6 bl = box[ch.x], br = box[ch.y];
        const double a = pt_box_area(pt_unite(bl, br));
        const double lc = cost[ch.x], rc = cost[ch.y];
        const double inner = c_box + (a > 0.0 ? (pt_box_area(bl) * lc + pt_box_area(br) * rc) / a : lc + rc);
        const uint32_t k = cnt[ch.x] + cnt[ch.y];
        const double as_leaf = c_open + c_tri * (double)k;
        const bool lf = k <= max_leaf && as_leaf <= inner;
        cnt[node] = k; cost[node] = lf ? as_leaf : inner; leafy[node] = lf ? 1u : 0u;
        icnt[node] = lf ? 0u : 1u + icnt[ch.x] + icnt[ch.y];
        step[ch.x] = Step{node, 1u, 0u, lf ? 1u : 0u};
        step[ch.y] = Step{node, 1u + icnt[ch.x], cnt[ch.x], lf ? 1u : 0u};
        node = parent[node];
    }
}

// one thread per node: walk to the root, then write what this node owns in the image
__global__ void k_emit(uint32_t n_all, uint32_t n, uint32_t root, float pad, const ptmi_triangle *__restrict__ tris,
                       const uint32_t *__restrict__ which, const Box6 *__restrict__ box, const uint2 *__restrict__ child,
                       const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ icnt, const uint32_t *__restrict__ leafy,
                       const Step *__restrict__ step, float4 *__restrict__ wn, float4 *__restrict__ tp, Red *red) {
    const uint32_t v = blockIdx.x * TB + threadIdx.x;
    if (v >= n_all) return;
    if (v >= n && leafy[v]) return;                              // a collapsed node: its units write its triangles
    uint32_t pre = 0, tri = 0, lvl = 1, u = v;
    bool emitted = true;
    while (u != root) {
        const Step s = step[u];
        pre += s.pre; tri += s.tri; lvl++;
        if (s.parent_leaf) emitted = false;
        u = s.parent;
    }
    if (v < n) {                                                 // a unit: its triangle at its place in leaf order
        const uint32_t orig = which[v];
        const ptmi_triangle &t = tris[orig];
        tp[3 * (size_t)tri + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], __uint_as_float(orig));
        tp[3 * (size_t)tri + 1] = make_float4(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2], 0.0f);
        tp[3 * (size_t)tri + 2] = make_float4(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2], 0.0f);
        return;
    }
    if (!emitted) return;
    const uint2 ch = child[v - n];
    const uint32_t c[2] = {ch.x, ch.y};
    const uint32_t cpre[2] = {pre + 1u, pre + 1u + icnt[ch.x]}, ctri[2] = {tri, tri + cnt[ch.x]};
    Box6 b[2]; uint32_t ref[2];
    for (int s = 0; s < 2; s++) {
        const Box6 e = box[c[s]];
        for (int k = 0; k < 3; k++) {
            b[s].mn[k] = pt_pad_lower(e.mn[k], pad); b[s].mx[k] = pt_pad_upper(e.mx[k], pad);
            atomicMin(&red->qmin[k], pt_ord(b[s].mn[k])); atomicMax(&red->qmax[k], pt_ord(b[s].mx[k]));
        }
        if (leafy[c[s]]) {
            ref[s] = PT_REF_LEAF | ((cnt[c[s]] - 1u) << PT_LEAF_OFF_BITS) | ctri[s];
            atomicMax(&red->max_leaf, cnt[c[s]]);
        } else {
            ref[s] = cpre[s];
        }
    }
    atomicMax(&red->depth, lvl + 1u);                            // the children sit one level down
    pt_wide_pack(wn + 4 * (size_t)pre, b[0].mn, b[0].mx, ref[0], b[1].mn, b[1].mx, ref[1]);
}

// the top `top` nodes breadth-first from the root (one thread: a few hundred steps)
__global__ void k_top(const float4 *__restrict__ wn, uint32_t top, uint32_t *__restrict__ renum, Red *red) {
    __shared__ uint32_t bfs[PT_QCACHE_NODES];
    uint32_t len = 0;
    bfs[len++] = 0u;
    for (uint32_t h = 0; h < len && len < top; h++) {
        const float4 *w = wn + 4 * (size_t)bfs[h];
        const uint32_t refs[2] = {pt_wide_ref(w, 0), pt_wide_ref(w, 1)};
        for (int c = 0; c < 2 && len < top; c++)
            if (!(refs[c] & PT_REF_LEAF)) bfs[len++] = refs[c];
    }
    for (uint32_t k = 0; k < len; k++) renum[bfs[k]] = k;
    red->n_top = len;
}

__global__ void k_rest_flags(uint32_t m, const uint32_t *__restrict__ renum, uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i < m) flags[i] = renum[i] == PT_REF_NONE ? 1u : 0u;
}

// every child of every node through the host's quantisation (wide_node.h); the nodes' new numbers from k_top and the scan
__global__ void k_quantise(uint32_t m, PtQuantGrid g, const float4 *__restrict__ wn, const uint32_t *__restrict__ renum,
                           const uint32_t *__restrict__ rest, const Red *red, uint4 *__restrict__ qn, double *__restrict__ growth,
                           uint32_t *__restrict__ grown) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= m) return;
    const uint32_t n_top = red->n_top;
    auto number = [&](uint32_t j) { const uint32_t r = renum[j]; return r != PT_REF_NONE ? r : n_top + rest[j]; };
    const uint32_t me = number(i);
    double gsum = 0.0; uint32_t gn = 0;
    for (int c = 0; c < 2; c++) {
        const PtWideChild ch = pt_wide_child(wn + 4 * (size_t)i, c);
        const PtQuantChild q = pt_quantise_child(g, ch.lo, ch.hi, (ch.ref & PT_REF_LEAF) ? ch.ref : number(ch.ref));
        qn[(size_t)me * 2 + c] = q.q;
        if (q.grown) { gsum += q.growth; gn++; }
    }
    growth[i] = gsum; grown[i] = gn;
}

// the build itself; every allocation is mem's until the three buffers of `out` leave through keep(). The stream may still be busy on failure.
bool build_own_tree(const ptmi_triangle *d_tris, const uint32_t *d_which, uint32_t n, const float4 *d_leafbox, uint32_t max_leaf,
                    uint32_t depth_limit, hipStream_t s, DevScratch &mem, PtOwnTreeGpu &out) {
    if (n < 2 || n > PT_LEAF_OFF_MASK || !d_which || !d_leafbox) return false;
    max_leaf = std::max(1u, std::min(max_leaf, PT_LEAF_MAX_TRIS));
    const uint32_t n_all = 2 * n - 1;
    auto blocks = [](uint32_t k) { return dim3((k + TB - 1) / TB); };
    auto read = [&](void *to, const void *from, size_t bytes) { return hip_ok(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, s)); };
    auto settled = [&] { return hip_ok(hipStreamSynchronize(s)) && hip_ok(hipGetLastError()); };

    // units
    Box6 *d_box = mem.get<Box6>(n_all);
    Red *d_red = mem.get<Red>(1);
    if (mem.failed) return false;
    Red h{};
    for (int k = 0; k < 3; k++) { h.cmin[k] = h.qmin[k] = 0xFFFFFFFFu; h.cmax[k] = h.qmax[k] = 0u; }
    if (!hip_ok(hipMemcpyAsync(d_red, &h, sizeof h, hipMemcpyHostToDevice, s))) return false;
    k_units<<<blocks(n), TB, 0, s>>>(n, d_tris, d_which, d_leafbox, d_box, d_red);
    if (!read(&h, d_red, sizeof h) || !settled()) return false;
    if (h.bad) return false;                                     // a non-finite vertex: the host refuses it too
    float pad, safe_origin;
    if (!pt_own_padding((double)pt_bits_float(h.biggest), pad, safe_origin)) return false;

    // Morton keys, sorted
    float lo[3], inv[3];
    for (int k = 0; k < 3; k++) { lo[k] = pt_unord_f(h.cmin[k]); inv[k] = pt_inv_extent(lo[k], pt_unord_f(h.cmax[k])); }
    unsigned long long *d_keys = mem.get<unsigned long long>(n), *d_keys2 = mem.get<unsigned long long>(n);
    if (mem.failed) return false;
    k_morton<<<blocks(n), TB, 0, s>>>(n, d_box, make_float3(lo[0], lo[1], lo[2]), make_float3(inv[0], inv[1], inv[2]), d_keys);
    size_t tmp_bytes = 0;
    {   // one scratch for the sort, the per-pass scan and the final scan and reductions: the largest of them
        unsigned long long *u64 = nullptr; uint32_t *u32 = nullptr; double *f64 = nullptr;
        size_t need[5] = {0, 0, 0, 0, 0};
        if (!hip_ok(pt_sort_keys_bytes(need[0], n, s)) ||
            !hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, need[1], u64, u64, (int)n + 1, s)) ||
            !hip_ok(hipcub::DeviceScan::ExclusiveSum(nullptr, need[2], u32, u32, (int)n, s)) ||
            !hip_ok(hipcub::DeviceReduce::Sum(nullptr, need[3], f64, f64, (int)n, s)) ||
            !hip_ok(hipcub::DeviceReduce::Sum(nullptr, need[4], u32, u32, (int)n, s))) return false;
        tmp_bytes = *std::max_element(need, need + 5);
    }
    void *d_tmp = mem.get<char>(tmp_bytes ? tmp_bytes : 16);
    if (!d_tmp || !hip_ok(pt_sort_keys(d_tmp, tmp_bytes, d_keys, d_keys2, n, s))) return false;

    // PLOC passes: each merges at least the globally closest pair. Collapsing takes at most max_leaf - 1 levels off a path, so a cluster
    // deeper than depth_limit + max_leaf - 1 levels can never give a tree within the limit: the build is refused as soon as one appears
    // (nested triangles along a line merge one pair per pass into a chain), before the passes and the emit walk grow with the depth.
    // The number of passes is capped as well (measured: 39 for 3 876 triangles, 62 for a million).
    uint32_t *d_clu[2] = {mem.get<uint32_t>(n), mem.get<uint32_t>(n)}, *d_nn = mem.get<uint32_t>(n);
    unsigned long long *d_flags = mem.get<unsigned long long>((size_t)n + 1), *d_ex = mem.get<unsigned long long>((size_t)n + 1);
    uint2 *d_child = mem.get<uint2>(n - 1);
    uint32_t *d_parent = mem.get<uint32_t>(n_all);
    uint8_t *d_level = mem.get<uint8_t>(n - 1);
    if (mem.failed || !hip_ok(hipMemsetAsync(d_parent, 0xFF, (size_t)n_all * 4, s))) return false;
    k_first_clusters<<<blocks(n), TB, 0, s>>>(n, d_keys2, d_clu[0]);
    uint32_t m = n, next = n;
    for (int cur = 0, pass = 0; m > 1; cur ^= 1, pass++) {
        if (pass >= kMaxPasses) return false;
        k_nearest<<<blocks(m), TB, 0, s>>>(m, d_clu[cur], d_box, d_nn);
        k_mark<<<blocks(m + 1), TB, 0, s>>>(m, d_nn, d_flags);
        if (!hip_ok(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_flags, d_ex, (int)m + 1, s))) return false;
        k_merge<<<blocks(m), TB, 0, s>>>(m, n, next, d_clu[cur], d_nn, d_flags, d_ex, d_box, d_child, d_parent, d_level, d_clu[cur ^ 1],
                                         d_red);
        unsigned long long tot = 0;
        uint32_t deepest = 0;
        if (!read(&tot, d_ex + m, 8) || !read(&deepest, &d_red->ploc_depth, 4) || !hip_ok(hipStreamSynchronize(s))) return false;
        const uint32_t made = (uint32_t)(tot >> 32), left = (uint32_t)tot;
        if (made == 0 || left + made != m) return false;          // cannot happen (see the top); refuse rather than loop
        if (deepest > depth_limit + max_leaf - 1u) return false; // too deep for any collapse: the host builds
        next += made; m = left;
    }
    if (!hip_ok(hipGetLastError())) return false;
    const uint32_t root = next - 1;
    if (root != n_all - 1) return false;

    // collapse
    uint32_t *d_arr = mem.get<uint32_t>(n - 1), *d_cnt = mem.get<uint32_t>(n_all), *d_icnt = mem.get<uint32_t>(n_all);
    uint32_t *d_leafy = mem.get<uint32_t>(n_all);
    double *d_cost = mem.get<double>(n_all);
    Step *d_step = mem.get<Step>(n_all);
    if (mem.failed || !hip_ok(hipMemsetAsync(d_arr, 0, (size_t)(n - 1) * 4, s))) return false;
    k_collapse<<<blocks(n), TB, 0, s>>>(n, max_leaf, PT_OWN_C_BOX, PT_OWN_C_TRI, PT_OWN_C_OPEN, d_box, d_child, d_parent, d_arr,
                                        d_cnt, d_icnt, d_cost, d_leafy, d_step);
    uint32_t n_inner = 0, root_leafy = 0;
    if (!read(&n_inner, d_icnt + root, 4) || !read(&root_leafy, d_leafy + root, 4) || !settled()) return false;
    if (root_leafy || n_inner == 0) return false;                // a single leaf (never above 32 triangles): the host's case
    mem.drop(d_clu[0], d_clu[1], d_nn, d_flags, d_ex, d_arr, d_cost);

    // emit
    float4 *d_wn = mem.get<float4>(4 * (size_t)n_inner), *d_tp = mem.get<float4>(3 * (size_t)n);
    if (mem.failed) return false;
    k_emit<<<blocks(n_all), TB, 0, s>>>(n_all, n, root, pad, d_tris, d_which, d_box, d_child, d_cnt, d_icnt, d_leafy, d_step, d_wn, d_tp, d_red);
    Box6 rb;
    if (!read(&rb, d_box + root, sizeof rb) || !read(&h, d_red, sizeof h) || !settled()) return false;
    if (h.depth > depth_limit) return false;
    rb = pt_pad_box(rb, pad);                                    // the root box depends on the triangle set only: the host's, bit for bit
    for (int k = 0; k < 3; k++) {
        out.root_min[k] = rb.mn[k]; out.root_max[k] = rb.mx[k];
        if (!std::isfinite(rb.mn[k]) || !std::isfinite(rb.mx[k])) return false;
    }
    out.pad = pad; out.safe_origin = safe_origin;
    out.root_ref = 0u; out.depth = h.depth; out.n_wnodes = n_inner; out.n_tris = n;
    out.n_leaves = n_inner + 1u; out.max_leaf_tris = h.max_leaf;
    mem.drop(d_step, d_child, d_box, d_parent, d_cnt, d_icnt, d_leafy);

    // quantised nodes (none when the 16-bit grid is too coarse for the scene, as on the host)
    out.quantised = false;
    uint4 *d_qn = nullptr;
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) { mn[k] = pt_unord_f(h.qmin[k]); mx[k] = pt_unord_f(h.qmax[k]); }
    PtQuantGrid g;
    if (pt_quant_grid(mn, mx, g.origin, g.scale)) {
        d_qn = mem.get<uint4>(2 * (size_t)n_inner);
        uint32_t *d_renum = mem.get<uint32_t>(n_inner), *d_rest_f = mem.get<uint32_t>(n_inner), *d_rest = mem.get<uint32_t>(n_inner);
        double *d_growth = mem.get<double>(n_inner);
        uint32_t *d_grown = mem.get<uint32_t>(n_inner);
        double *d_growth_sum = mem.get<double>(1);
        uint32_t *d_grown_sum = mem.get<uint32_t>(1);
        if (mem.failed || !hip_ok(hipMemsetAsync(d_renum, 0xFF, (size_t)n_inner * 4, s))) return false;
        k_top<<<1, 1, 0, s>>>(d_wn, std::min<uint32_t>(PT_QCACHE_NODES, n_inner), d_renum, d_red);
        k_rest_flags<<<blocks(n_inner), TB, 0, s>>>(n_inner, d_renum, d_rest_f);
        if (!hip_ok(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_rest_f, d_rest, (int)n_inner, s))) return false;
        k_quantise<<<blocks(n_inner), TB, 0, s>>>(n_inner, g, d_wn, d_renum, d_rest, d_red, d_qn, d_growth, d_grown);
        if (!hip_ok(hipcub::DeviceReduce::Sum(d_tmp, tmp_bytes, d_growth, d_growth_sum, (int)n_inner, s)) ||
            !hip_ok(hipcub::DeviceReduce::Sum(d_tmp, tmp_bytes, d_grown, d_grown_sum, (int)n_inner, s))) return false;
        double growth = 0.0; uint32_t grown = 0;
        if (!read(&growth, d_growth_sum, 8) || !read(&grown, d_grown_sum, 4) || !read(&h, d_red, sizeof h) || !settled()) return false;
        if (!(grown && growth / (double)grown > 0.25)) {
            out.quantised = true; out.q_top = h.n_top;
            for (int k = 0; k < 3; k++) { out.q_origin[k] = g.origin[k]; out.q_scale[k] = g.scale[k]; }
        }
    }
    if (!out.quantised) { mem.drop(d_qn); d_qn = nullptr; }
    out.wnodes = mem.keep(d_wn); out.tripos = mem.keep(d_tp); out.qnodes = mem.keep(d_qn);
    return true;
}

}  // namespace

// one build in a scratch of its own: `build` takes every allocation from it (false: it could not build)
template <class Build>
static bool build_in_scope(hipStream_t s, PtOwnTreeGpu &out, Build &&build) {
    out.release();
    bool ok;
    {
        DevScratch mem;
        ok = build(mem);
        (void)hipStreamSynchronize(s);                           // nothing of ours may still run when the scratch goes
    }
    if (!ok) { (void)hipGetLastError(); out.release(); }
    return ok;
}

bool pt_build_own_tree_gpu(const ptmi_triangle *d_tris, const uint32_t *d_which, uint32_t n_units, const float4 *d_leafbox,
                           uint32_t max_leaf, uint32_t depth_limit, hipStream_t s, PtOwnTreeGpu &out) {
    return build_in_scope(s, out, [&](DevScratch &mem) {
        return build_own_tree(d_tris, d_which, n_units, d_leafbox, max_leaf, depth_limit, s, mem, out);
    });
}

// an upload has the unit list and the leaf boxes on the host: copy, then the build above
bool pt_build_own_tree_gpu(const ptmi_triangle *d_tris, const std::vector<uint32_t> &which, const std::vector<float4> &leafbox,
                           uint32_t max_leaf, uint32_t depth_limit, hipStream_t s, PtOwnTreeGpu &out) {
    return build_in_scope(s, out, [&](DevScratch &mem) {
        const uint32_t n = (uint32_t)which.size();
        uint32_t *d_which = mem.get<uint32_t>(n);
        float4 *d_leafbox = mem.get<float4>(leafbox.size());
        if (mem.failed || n < 2 ||
            !hip_ok(hipMemcpyAsync(d_which, which.data(), (size_t)n * 4, hipMemcpyHostToDevice, s)) ||
            !hip_ok(hipMemcpyAsync(d_leafbox, leafbox.data(), leafbox.size() * sizeof(float4), hipMemcpyHostToDevice, s))) return false;
        return build_own_tree(d_tris, d_which, n, d_leafbox, max_leaf, depth_limit, s, mem, out);
    });
}

void PtOwnTreeGpu::release() {
    (void)hipFree(wnodes); (void)hipFree(tripos); (void)hipFree(qnodes);
    *this = PtOwnTreeGpu();
}
