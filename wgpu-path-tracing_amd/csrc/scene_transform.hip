// scene_transform.hip — objects moved on the device (include/ptmi.h: ptmi_set_triangle_groups, ptmi_transform_groups).
//
// The caller tags every uploaded triangle with a group id once; the context then keeps the REST POSE (v0, v1, v2, n0, n1, n2 of every
// triangle, 6 float4 = 96 bytes) beside the table. ptmi_transform_groups sets matrices for some groups: every member's live record
// becomes T(rest) and the refit of ptmi_update_triangles follows (scene_update.hip refit_written: the same routine, not a copy).
//
// All-or-nothing by a CHECK PASS followed by a WRITE PASS (no staging buffer): the check pass reads the rest pose only, transforms the
// three vertices and applies ptmi_update_triangles' vertex checks; the smallest offending triangle goes through a wave ballot and one
// atomicMin per wave into word 0 of buf[kGroupMap]. Only when that word is still "none" does the write pass run, which writes the six
// float4 of named members and nothing else. Both passes are one kernel template, so they cannot disagree on the arithmetic.
//
// Layout: eight lanes per triangle, one float4 each. Lanes 0-5 of an octet take the six float4 of the 96-byte rest record (0-2 a
// vertex, 3-5 a normal), lanes 6 and 7 idle, so a wave covers 8 triangles and stores into whole 128-byte lines of the live records.
// The group word and the op index are read by lane 0 of the octet and broadcast with __shfl. The op records of a launch sit in LDS
// (96 bytes each; at most kChunk = 512 per launch, 48 KB); a call with more ops runs one launch per chunk of 512. Octets whose group
// the launch does not name load and store nothing beyond those two words.
//
// -DPT_TRANSFORM_LANES=1 builds the layout this one was measured against instead (a lane per triangle, the same arithmetic through the
// same functions): an A/B switch for tools/transform_cost.py, never the default. The numbers are in profiles/README.md.
#include "ptmi_ctx.h"
#include "pt_transform.h"   // transform_row, vertex_bad and the record constants, shared with scene_skin.hip

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace {

#ifndef PT_TRANSFORM_LANES
#define PT_TRANSFORM_LANES 8
#endif
static_assert(PT_TRANSFORM_LANES == 8 || PT_TRANSFORM_LANES == 1, "eight lanes per triangle, or one");

constexpr int TB = 256;
constexpr int kOctets = TB / PT_TRANSFORM_LANES;   // triangles per block and round
constexpr uint32_t kChunk = 512u;            // op records per launch (LDS)
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxGroups = 65536u;
constexpr uint32_t kMapHead = 4u;            // words in front of the group -> op map; word 0: the check pass's smallest offender
static_assert(sizeof(struct ptmi_transform_status) == 32, "ptmi_transform_status is 32 bytes");

// the rows [first, first + count) of the live records to the rest pose: a thread per float4
__global__ void __launch_bounds__(TB) k_rest_snapshot(uint32_t first, uint32_t count, const float4 *__restrict__ live, float4 *__restrict__ rest) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= (size_t)count * kRestQ) return;
    const size_t tri = first + i / kRestQ, q = i % kRestQ;
    rest[tri * kRestQ + q] = live[tri * kLiveQ + q];
}

// Triangles [tri_first, tri_end) against the ops [op_first, op_first + op_count) of the call. WRITE: the six float4 of named members
// go to `live`. Otherwise nothing of the scene is written: the three vertices are checked and the smallest offender goes to *first_bad.
// Every lane of a wave reaches every __shfl and the ballot (no early return; the loop bounds are the same for a whole block).
template <bool WRITE>
__global__ void __launch_bounds__(TB) k_transform(uint32_t tri_first, uint32_t tri_end, uint32_t n_groups, const uint32_t *__restrict__ group,
                                                  const uint32_t *__restrict__ map, const ptmi_group_transform *__restrict__ ops,
                                                  uint32_t op_first, uint32_t op_count, const float4 *__restrict__ rest, float4 *live,
                                                  uint32_t own, uint32_t *first_bad) {
    extern __shared__ float4 s_ops4[];
    const float4 *src = reinterpret_cast<const float4 *>(ops + op_first);
    for (uint32_t i = threadIdx.x; i < op_count * kOpQ; i += TB) s_ops4[i] = src[i];
    __syncthreads();
    const float *s_ops = reinterpret_cast<const float *>(s_ops4);
    const uint32_t lane = threadIdx.x & 63u, l8 = threadIdx.x & 7u, head = lane & ~7u;
    const uint32_t stride = gridDim.x * kOctets;
    uint32_t worst = kNone;
    for (uint32_t base = tri_first + blockIdx.x * kOctets; base < tri_end; base += stride) {
        const uint32_t tri = base + (threadIdx.x >> 3);
        uint32_t op = kNone;
        if (l8 == 0u && tri < tri_end) {
            const uint32_t g = group[tri];
            if (g < n_groups) op = map[g];
        }
        op = (uint32_t)__shfl((int)op, (int)head);
        const bool named = op >= op_first && op - op_first < op_count;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (named && l8 < (WRITE ? 6u : 3u)) {
            r = transform_row(s_ops + (size_t)(op - op_first) * (kOpQ * 4), l8, rest[(size_t)tri * kRestQ + l8]);
            if (WRITE) live[(size_t)tri * kLiveQ + l8] = r;
        }
        if (!WRITE) {
            // lane 0 of the octet holds a = v0', lanes 1 and 2 hold b and d
            const float4 a = make_float4(__shfl(r.x, (int)head), __shfl(r.y, (int)head), __shfl(r.z, (int)head), 0.0f);
            const bool bad = named && l8 < 3u && vertex_bad(a, r, own && l8 != 0u);
            const unsigned long long mask = __ballot(bad);
            if (mask) {                                              // triangles ascend with the lane: the lowest set bit is the smallest
                const uint32_t l = (uint32_t)__ffsll((long long)mask) - 1u;
                worst = min(worst, base + ((threadIdx.x & ~63u) >> 3) + (l >> 3));
            }
        }
    }
    if (!WRITE && lane == 0u && worst != kNone) atomicMin(first_bad, worst);
}

// The layout the one above was measured against (PT_TRANSFORM_LANES = 1): a lane per triangle, which walks the six float4 of its
// record itself - every load and store of a wave strides by a whole record. The same arguments, the same results.
template <bool WRITE>
__global__ void __launch_bounds__(TB) k_transform_lane(uint32_t tri_first, uint32_t tri_end, uint32_t n_groups, const uint32_t *__restrict__ group,
                                                       const uint32_t *__restrict__ map, const ptmi_group_transform *__restrict__ ops,
                                                       uint32_t op_first, uint32_t op_count, const float4 *__restrict__ rest, float4 *live,
                                                       uint32_t own, uint32_t *first_bad) {
    extern __shared__ float4 s_ops4[];
    const float4 *src = reinterpret_cast<const float4 *>(ops + op_first);
    for (uint32_t i = threadIdx.x; i < op_count * kOpQ; i += TB) s_ops4[i] = src[i];
    __syncthreads();
    const float *s_ops = reinterpret_cast<const float *>(s_ops4);
    const uint32_t stride = gridDim.x * TB;
    uint32_t worst = kNone;
    for (uint32_t base = tri_first + blockIdx.x * TB; base < tri_end; base += stride) {
        const uint32_t tri = base + threadIdx.x;
        uint32_t op = kNone;
        if (tri < tri_end) {
            const uint32_t g = group[tri];
            if (g < n_groups) op = map[g];
        }
        const bool named = op >= op_first && op - op_first < op_count;
        bool bad = false;
        if (named) {
            const float *o = s_ops + (size_t)(op - op_first) * (kOpQ * 4);
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (uint32_t q = 0; q < (WRITE ? 6u : 3u); q++) {
                const float4 r = transform_row(o, q, rest[(size_t)tri * kRestQ + q]);
                if (WRITE) live[(size_t)tri * kLiveQ + q] = r;
                else {
                    if (q == 0u) a = r;
                    bad = bad || vertex_bad(a, r, own && q != 0u);
                }
            }
        }
        if (!WRITE) {
            const unsigned long long mask = __ballot(bad);
            if (mask) worst = min(worst, base + (threadIdx.x & ~63u) + (uint32_t)__ffsll((long long)mask) - 1u);
        }
    }
    if (!WRITE && (threadIdx.x & 63u) == 0u && worst != kNone) atomicMin(first_bad, worst);
}

dim3 blocks_for(size_t threads) { return dim3((unsigned)((threads + TB - 1) / TB)); }

int snapshot(ptmi_ctx *c, uint32_t first, uint32_t count, void *rest) {
    if (!count) return PTMI_OK;
    k_rest_snapshot<<<blocks_for((size_t)count * kRestQ), TB, 0, c->stream>>>(first, count, reinterpret_cast<const float4 *>(c->sc.tris),
                                                                              static_cast<float4 *>(rest));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

// one pass over the call's ops, a launch per chunk of kChunk: over the triangles between the chunk's lowest and highest member
template <bool WRITE>
int run_pass(ptmi_ctx *c, const ptmi_group_transform *ops, uint32_t n_ops) {
    uint32_t *head = static_cast<uint32_t *>(c->buf[kGroupMap]);
    for (uint32_t f = 0; f < n_ops; f += kChunk) {
        const uint32_t cnt = std::min(kChunk, n_ops - f);
        uint32_t lo = kNone, hi = 0u;
        for (uint32_t i = f; i < f + cnt; i++) {
            const uint32_t g = ops[i].group;
            if (c->grp_members[g]) { lo = std::min(lo, c->grp_lo[g]); hi = std::max(hi, c->grp_hi[g]); }
        }
        if (lo == kNone) continue;
        const uint32_t first = lo & ~7u, end = hi + 1u;              // (an octet's eight records start on a line of the group table)
        const uint32_t want = (end - first + kOctets - 1) / kOctets, most = (uint32_t)std::max(1, c->n_cu) * 8u;
#if PT_TRANSFORM_LANES == 1
        const auto kernel = k_transform_lane<WRITE>;
#else
        const auto kernel = k_transform<WRITE>;
#endif
        kernel<<<dim3(std::min(want, most)), TB, (size_t)cnt * sizeof(ptmi_group_transform), c->stream>>>(
            first, end, c->tf.n_groups, static_cast<const uint32_t *>(c->buf[kGroupTab]), head + kMapHead,
            static_cast<const ptmi_group_transform *>(c->buf[kGroupOps]), f, cnt, static_cast<const float4 *>(c->buf[kGroupRest]),
            reinterpret_cast<float4 *>(const_cast<ptmi_triangle *>(c->sc.tris)), c->sc.own, head);
    }
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

}  // namespace

int pt_check_triangle_groups(const ptmi_ctx *c, const uint32_t *group, uint32_t n, uint32_t *n_groups_out, std::string &err) {
    if (!c->have_scene) return fail(err, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if (!group || n == 0u) return PTMI_OK;                          // a removal
    if (n != c->sc.n_tris) return fail(err, PTMI_E_INVALID, "n_triangles %u is not the loaded scene's %u", n, c->sc.n_tris);
    uint32_t top = 0u;
    for (uint32_t i = 0; i < n; i++) top = std::max(top, group[i]);
    if (top >= kMaxGroups) return fail(err, PTMI_E_UNSUPPORTED, "group id %u: at most %u groups", top, kMaxGroups);
    if (n_groups_out) *n_groups_out = top + 1u;
    return PTMI_OK;
}

int pt_check_group_transforms(const ptmi_ctx *c, const ptmi_group_transform *ops, uint32_t n_ops, std::string &err) {
    if (!c->grp_present) return fail(err, PTMI_E_STATE, "no group table is in place (ptmi_set_triangle_groups)");
    if (n_ops && !ops) return fail(err, PTMI_E_INVALID, "NULL ops with a non-zero count");
    std::vector<uint8_t> seen(c->tf.n_groups, 0);
    for (uint32_t i = 0; i < n_ops; i++) {
        const ptmi_group_transform &o = ops[i];
        if (o.reserved0 || o.reserved1) return fail(err, PTMI_E_INVALID, "op %u: ptmi_group_transform.reserved must be 0", i);
        if (o.group >= c->tf.n_groups) return fail(err, PTMI_E_INVALID, "op %u names group %u of %u", i, o.group, c->tf.n_groups);
        if (seen[o.group]) return fail(err, PTMI_E_INVALID, "op %u: group %u is named twice", i, o.group);
        seen[o.group] = 1;
        for (float v : o.m) if (!std::isfinite(v)) return fail(err, PTMI_E_INVALID, "op %u: a matrix entry is not finite", i);
        for (float v : o.nm) if (!std::isfinite(v)) return fail(err, PTMI_E_INVALID, "op %u: a normal-matrix entry is not finite", i);
    }
    return PTMI_OK;
}

PT_HOST {

void groups_forget(ptmi_ctx *c) {
    for (SceneBuf k : {kGroupTab, kGroupRest, kGroupOps, kGroupMap}) dfree(c->buf[k]);
    c->grp_present = false; c->grp_ops_cap = 0;
    c->grp_lo.clear(); c->grp_hi.clear(); c->grp_members.clear(); c->grp_map.clear(); c->grp_moved.clear(); c->grp_mats.clear();
    c->tf = {};
}

int groups_rebase(ptmi_ctx *c, uint32_t first, uint32_t count) {
    if (!c->grp_present) return PTMI_OK;
    return snapshot(c, first, count, c->buf[kGroupRest]);
}

}  // namespace pt_host

extern "C" {

// The new buffers exist and are filled before anything of the context changes, so a failed call keeps the previous table.
int ptmi_set_triangle_groups(ptmi_ctx *c, const uint32_t *group, uint32_t n) {
    if (!c) return PTMI_E_INVALID;
    uint32_t ng = 0u;
    const int rc = pt_check_triangle_groups(c, group, n, &ng, c->err);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    if (!group || n == 0u) { groups_forget(c); return PTMI_OK; }
    std::vector<uint32_t> map((size_t)kMapHead + ng, kNone);
    void *tab = nullptr, *rest = nullptr, *dmap = nullptr;
    hipError_t e = hipMalloc(&tab, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&rest, (size_t)n * kRestQ * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&dmap, map.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(tab, group, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dmap, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    int rs = PTMI_OK;
    if (e == hipSuccess && !(rs = snapshot(c, 0u, n, rest))) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || rs) {
        dfree(tab); dfree(rest); dfree(dmap);
        if (rs) return rs;
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "the group table could not be made: %s (the previous table, if any, is still in place)", hipGetErrorString(e));
    }
    groups_forget(c);
    c->buf[kGroupTab] = tab; c->buf[kGroupRest] = rest; c->buf[kGroupMap] = dmap;
    c->grp_present = true;
    c->grp_map = std::move(map);
    c->grp_lo.assign(ng, kNone); c->grp_hi.assign(ng, 0u); c->grp_members.assign(ng, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t g = group[i];
        if (!c->grp_members[g]++) c->grp_lo[g] = i;                  // (ascending i: the first member is the lowest)
        c->grp_hi[g] = i;
    }
    c->grp_moved.assign(ng, 0); c->grp_mats.assign(ng, ptmi_group_transform{});
    c->tf.present = 1u; c->tf.n_groups = ng; c->tf.first_bad = kNone;
    return PTMI_OK;
}

int ptmi_transform_groups(ptmi_ctx *c, const ptmi_group_transform *ops, uint32_t n_ops) {
    if (!c) return PTMI_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = pt_check_group_transforms(c, ops, n_ops, c->err);
    if (rc || (rc = refit_begin(c))) return rc;
    uint32_t lo = kNone, hi = 0u, moved = 0u;
    for (uint32_t i = 0; i < n_ops; i++) {
        const uint32_t g = ops[i].group;
        if (!c->grp_members[g]) continue;
        lo = std::min(lo, c->grp_lo[g]); hi = std::max(hi, c->grp_hi[g]); moved += c->grp_members[g];
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                        // nothing in flight reads the scene any more
    uint32_t *head = static_cast<uint32_t *>(c->buf[kGroupMap]);
    if (moved) {
        if (c->grp_ops_cap < n_ops) {
            dfree(c->buf[kGroupOps]); c->grp_ops_cap = 0;
            HIP_TRY(c, hipMalloc(&c->buf[kGroupOps], (size_t)n_ops * sizeof(ptmi_group_transform)));
            c->grp_ops_cap = n_ops;
        }
        HIP_TRY(c, hipMemcpy(c->buf[kGroupOps], ops, (size_t)n_ops * sizeof(ptmi_group_transform), hipMemcpyHostToDevice));
        // the map of this call (and "none" in the check pass's word); the host's copy goes back to all "not named" at once
        for (uint32_t i = 0; i < n_ops; i++) c->grp_map[kMapHead + ops[i].group] = i;
        const hipError_t e = hipMemcpy(head, c->grp_map.data(), c->grp_map.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        for (uint32_t i = 0; i < n_ops; i++) c->grp_map[kMapHead + ops[i].group] = kNone;
        HIP_TRY(c, e);
        // the check pass: nothing of the scene is written before it has found nothing
        if ((rc = run_pass<false>(c, ops, n_ops))) return rc;
        uint32_t bad = kNone;
        HIP_TRY(c, hipMemcpyAsync(&bad, head, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (bad != kNone) {
            c->tf.first_bad = bad;
            return fail(c, PTMI_E_INVALID, "triangle %u: a transformed vertex is not finite%s (nothing was changed)", bad,
                        c->sc.own ? ", or an edge is too long for float32 arithmetic" : "");
        }
    }
    if ((rc = refit_ready(c))) return rc;                           // the plan, at the first edit after an upload
    if (moved) {
        if ((rc = run_pass<true>(c, ops, n_ops))) return rc;
        motion_widen(c, lo, hi - lo + 1u);                          // while motion is on: from the lowest to the highest member named
    }
    if ((rc = refit_written(c, t0))) return rc;
    for (uint32_t i = 0; i < n_ops; i++) { c->grp_moved[ops[i].group] = 1; c->grp_mats[ops[i].group] = ops[i]; }
    c->tf.transforms++; c->tf.last_moved = moved; c->tf.first_bad = kNone;
    c->tf.transform_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PTMI_OK;
}

// the cofactors of the upper 3 x 3 (a_ij = m[4 i + j]), each a*b - c*d in double in that order
void ptmi_normal_matrix(const float m[12], float nm[9]) {
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    nm[0] = (float)(a11 * a22 - a12 * a21); nm[1] = (float)(a12 * a20 - a10 * a22); nm[2] = (float)(a10 * a21 - a11 * a20);
    nm[3] = (float)(a02 * a21 - a01 * a22); nm[4] = (float)(a00 * a22 - a02 * a20); nm[5] = (float)(a01 * a20 - a00 * a21);
    nm[6] = (float)(a01 * a12 - a02 * a11); nm[7] = (float)(a02 * a10 - a00 * a12); nm[8] = (float)(a00 * a11 - a01 * a10);
}

int ptmi_transform_status(ptmi_ctx *c, struct ptmi_transform_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->tf;
    return PTMI_OK;
}

int ptmi_debug_read_triangles(ptmi_ctx *c, uint32_t first, uint32_t count, ptmi_triangle *out) {
    if (!c) return PTMI_E_INVALID;
    if (!c->have_scene) return fail(c, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if ((uint64_t)first + count > c->sc.n_tris)
        return fail(c, PTMI_E_INVALID, "triangles [%u, +%u) reach beyond the %u uploaded", first, count, c->sc.n_tris);
    if (!count) return PTMI_OK;
    if (!out) return fail(c, PTMI_E_INVALID, "out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, hipMemcpy(out, c->sc.tris + first, (size_t)count * sizeof(ptmi_triangle), hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
