// scene_transform.hip — objects moved on the device (include/ptmi.h: ptmi_set_triangle_groups, ptmi_transform_groups).
//
// The caller tags every uploaded triangle with a group id once; the context then keeps the REST POSE (v0, v1, v2, n0, n1, n2 of every
// triangle, 6 float4 = 96 bytes) beside the table. ptmi_transform_groups sets matrices for some groups: every member's live record
// becomes T(rest) and the refit of ptmi_update_triangles follows (scene_update.hip refit_written: the same routine, not a copy).
//
// All-or-nothing by a CHECK PASS followed by a WRITE PASS (no staging buffer), the sequence every pose source runs (scene_pose.hip
// pose_refusable; the check word is word 0 of buf[kGroupMap]). This file's own: the table and its host bookkeeping, the group -> op map
// of a call, and k_transform, one kernel template for both passes, so they cannot disagree on the arithmetic. The check pass reads the
// rest pose only and applies ptmi_update_triangles' vertex checks to the three transformed vertices; the write pass writes the six
// float4 of named members and nothing else.
//
// Layout: eight lanes per triangle, one float4 each (pt_transform.h Octet has the coordinates and why lanes 6 and 7 idle). The group
// word and the op index are read by lane 0 of the octet and broadcast with __shfl. The op records of a launch sit in LDS (96 bytes
// each; at most kChunk = 512 per launch, 48 KB); a call with more ops runs one launch per chunk of 512. Octets whose group the launch
// does not name load and store nothing beyond those two words.
#include "ptmi_ctx.h"
#include "pt_dev_scratch.h"
#include "pt_transform.h"   // the arithmetic, the octet layout, the check tail and the constants, shared with scene_skin.hip

#include <algorithm>
#include <chrono>

namespace {

constexpr uint32_t kChunk = 512u;            // op records per launch (LDS)
constexpr uint32_t kMaxGroups = 65536u;
static_assert(sizeof(struct ptmi_transform_status) == 32, "ptmi_transform_status is 32 bytes");

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
    const Octet o = octet_here();
    uint32_t worst = kNone;
    for (uint32_t base = tri_first + blockIdx.x * kOctets; base < tri_end; base += octet_stride()) {
        const uint32_t tri = base + o.slot;
        uint32_t op = kNone;
        if (o.l8 == 0u && tri < tri_end) {
            const uint32_t g = group[tri];
            if (g < n_groups) op = map[g];
        }
        op = (uint32_t)__shfl((int)op, (int)o.head);
        const bool named = op >= op_first && op - op_first < op_count;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (named && o.l8 < (WRITE ? 6u : 3u)) {
            r = transform_row(s_ops + (size_t)(op - op_first) * (kOpQ * 4), o.l8, rest[(size_t)tri * kRestQ + o.l8]);
            if (WRITE) live[(size_t)tri * kLiveQ + o.l8] = r;
        }
        if (!WRITE) worst = check_tail(o, r, named, own, base, worst);
    }
    if (!WRITE && o.lane == 0u && worst != kNone) atomicMin(first_bad, worst);
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
        k_transform<WRITE><<<pose_blocks(end - first, c->n_cu), TB, (size_t)cnt * sizeof(ptmi_group_transform), c->stream>>>(
            first, end, c->tf.n_groups, static_cast<const uint32_t *>(c->buf[kGroupTab]), head + kPoseHead,
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
    return check_matrix_records(ops, n_ops, "op", "ptmi_group_transform", err, [&](uint32_t i, const ptmi_group_transform &o) -> int {
        if (o.group >= c->tf.n_groups) return fail(err, PTMI_E_INVALID, "op %u names group %u of %u", i, o.group, c->tf.n_groups);
        if (seen[o.group]) return fail(err, PTMI_E_INVALID, "op %u: group %u is named twice", i, o.group);
        seen[o.group] = 1;
        return PTMI_OK;
    });
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
    return pose_snapshot(c, first, count, nullptr, c->buf[kGroupRest]);
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
    std::vector<uint32_t> map((size_t)kPoseHead + ng, kNone);
    DevScratch fresh;                                               // freed on every way out but the last
    uint32_t *tab = fresh.get<uint32_t>(n);
    float4 *rest = fresh.get<float4>((size_t)n * kRestQ);
    uint32_t *dmap = fresh.get<uint32_t>(map.size());
    hipError_t e = fresh.error;
    int rs = PTMI_OK;
    if (hip_ok(e) && hip_ok(e = hipMemcpy(tab, group, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        hip_ok(e = hipMemcpy(dmap, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        !(rs = pose_snapshot(c, 0u, n, nullptr, rest))) e = hipStreamSynchronize(c->stream);
    if (rs) return rs;
    if (!hip_ok(e)) {
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "the group table could not be made: %s (the previous table, if any, is still in place)", hipGetErrorString(e));
    }
    groups_forget(c);
    c->buf[kGroupTab] = fresh.keep(tab); c->buf[kGroupRest] = fresh.keep(rest); c->buf[kGroupMap] = fresh.keep(dmap);
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
    if (rc) return rc;
    uint32_t lo = kNone, hi = 0u, moved = 0u;
    for (uint32_t i = 0; i < n_ops; i++) {
        const uint32_t g = ops[i].group;
        if (!c->grp_members[g]) continue;
        lo = std::min(lo, c->grp_lo[g]); hi = std::max(hi, c->grp_hi[g]); moved += c->grp_members[g];
    }
    uint32_t *head = static_cast<uint32_t *>(c->buf[kGroupMap]);
    auto stage = [&]() -> int {
        if (c->grp_ops_cap < n_ops) {
            dfree(c->buf[kGroupOps]); c->grp_ops_cap = 0;
            HIP_TRY(c, hipMalloc(&c->buf[kGroupOps], (size_t)n_ops * sizeof(ptmi_group_transform)));
            c->grp_ops_cap = n_ops;
        }
        HIP_TRY(c, hipMemcpy(c->buf[kGroupOps], ops, (size_t)n_ops * sizeof(ptmi_group_transform), hipMemcpyHostToDevice));
        // the map of this call (and "none" in the check word); the host's copy goes back to all "not named" at once
        for (uint32_t i = 0; i < n_ops; i++) c->grp_map[kPoseHead + ops[i].group] = i;
        const hipError_t e = hipMemcpy(head, c->grp_map.data(), c->grp_map.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        for (uint32_t i = 0; i < n_ops; i++) c->grp_map[kPoseHead + ops[i].group] = kNone;
        HIP_TRY(c, e);
        return PTMI_OK;
    };
    auto pass = [&](bool write) { return write ? run_pass<true>(c, ops, n_ops) : run_pass<false>(c, ops, n_ops); };
    PoseCall p{stage, pass};
    p.moves = moved != 0u;                                          // ops on memberless groups alone: the refit and the counters, no pass
    p.check_word = head; p.first_bad = &c->tf.first_bad; p.how = "transformed";
    p.lo = lo; p.hi = hi;                                           // from the lowest to the highest member named
    if ((rc = pose_refusable(c, t0, p))) return rc;
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
