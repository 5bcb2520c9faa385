// scene_skin.hip — skinned triangles posed on the device (include/ptmi.h: ptmi_set_skin, ptmi_pose_skin).
//
// The caller lists the skinned triangles once (ascending indices) with three corner records each (four joints, four weights); the
// context keeps, PER LISTED TRIANGLE and in list order, the index (buf[kSkinList]), the corner records (buf[kSkinCorners], 96 bytes)
// and the REST POSE (buf[kSkinRest]: v0, v1, v2, n0, n1, n2, 96 bytes). ptmi_pose_skin sends one 96-byte record per joint: every
// listed triangle's live record becomes the blend of its joints' matrices applied to its rest record, and the refit of
// ptmi_update_triangles follows (scene_update.hip refit_written: the same routine, not a copy).
//
// All-or-nothing by a CHECK PASS followed by a WRITE PASS, the sequence every pose source runs (scene_pose.hip pose_refusable; the
// check word is word 0 of buf[kSkinJoints]). This file's own: the list and the corner records, the blend, and k_skin, one kernel
// template for both passes: the check pass skins the three vertices and applies ptmi_update_triangles' vertex checks.
//
// Layout: the kernel walks the LIST, eight lanes per listed triangle, one float4 each (pt_transform.h Octet has the coordinates and why
// lanes 6 and 7 idle). Lane q < 6 of an octet loads float4 q of the rest record and float4 q of the corner records, so neighbouring
// lanes read neighbouring float4 of both arrays; the corner record of corner k (joints in float4 2k, weights in float4 2k + 1) reaches
// the lanes that need it through __shfl. Lanes 0-2 blend the 12 entries of m for their corner and transform a vertex, lanes 3-5 blend
// the 9 entries of nm and transform a normal; no lane blends both. The stores go to whole 128-byte lines of the live records,
// scattered as the list is. Because the list ascends, the smallest offending entry of a wave is its smallest offending triangle.
// The joint records sit in LDS up to kLdsJoints = 512 of them (48 KB); a second instantiation of the same template reads them from
// global memory up to 65 536. Either way one launch covers the whole list.
#include "ptmi_ctx.h"
#include "pt_dev_scratch.h"
#include "pt_transform.h"   // the arithmetic, the octet layout, the check tail and the constants, shared with scene_transform.hip

#include <algorithm>
#include <chrono>
#include <cmath>

namespace {

constexpr uint32_t kLdsJoints = 512u;        // joint records a block keeps in LDS
constexpr uint32_t kMaxJoints = 65536u;
static_assert(sizeof(ptmi_skin_corner) == 32 && 3 * sizeof(ptmi_skin_corner) == kRestQ * sizeof(float4), "three corner records are 6 float4");
static_assert(sizeof(struct ptmi_skin_status) == 32, "ptmi_skin_status is 32 bytes");
static_assert(kLdsJoints * sizeof(ptmi_joint_transform) == 48u * 1024u, "the joint records of the LDS instantiation take 48 KB");

// word e of the blend of four joint records (24 words each, at J) by the weights w: the order of include/ptmi.h, every slot evaluated
__device__ __forceinline__ float blend(const float *J, uint4 j, float4 w, int e) {
    return ((w.x * J[j.x * kOpWords + e] + w.y * J[j.y * kOpWords + e]) + w.z * J[j.z * kOpWords + e]) + w.w * J[j.w * kOpWords + e];
}

// The list entries [0, n_listed). WRITE: the six float4 of every listed triangle go to `live`. Otherwise nothing of the scene is
// written: the three vertices are checked and the smallest offending triangle goes to *first_bad. LDS: the joint records are copied to
// shared memory first (n_joints <= kLdsJoints), else they are read where they are.
// Every lane of a wave reaches every __shfl and the ballot (no early return; the loop bounds are the same for a whole block).
template <bool WRITE, bool LDS>
__global__ void __launch_bounds__(TB) k_skin(uint32_t n_listed, const uint32_t *__restrict__ list, const float4 *__restrict__ corners,
                                             const float4 *__restrict__ rest, const float4 *__restrict__ joints, uint32_t n_joints,
                                             float4 *live, uint32_t own, uint32_t *first_bad) {
    extern __shared__ float4 s_joints4[];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < n_joints * kOpQ; i += TB) s_joints4[i] = joints[i];
        __syncthreads();
    }
    const float *J = LDS ? reinterpret_cast<const float *>(s_joints4) : reinterpret_cast<const float *>(joints);
    const Octet o = octet_here();
    const uint32_t corner = o.l8 < 3u ? o.l8 : (o.l8 < 6u ? o.l8 - 3u : 0u);    // whose corner record this lane blends by
    const int src = (int)(o.head + 2u * corner);
    uint32_t worst = kNone;                                              // the smallest offending list entry this lane has seen
    for (uint32_t base = blockIdx.x * kOctets; base < n_listed; base += octet_stride()) {
        const uint32_t entry = base + o.slot;
        const bool listed = entry < n_listed;
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cq = p;
        uint32_t tri = 0u;
        if (listed && o.l8 < 6u) {
            p = rest[(size_t)entry * kRestQ + o.l8];
            cq = corners[(size_t)entry * kRestQ + o.l8];
        }
        if (WRITE) {
            if (listed && o.l8 == 0u) tri = list[entry];
            tri = (uint32_t)__shfl((int)tri, (int)o.head);
        }
        uint4 j;
        float4 w;
        j.x = (uint32_t)__shfl(__float_as_int(cq.x), src); j.y = (uint32_t)__shfl(__float_as_int(cq.y), src);
        j.z = (uint32_t)__shfl(__float_as_int(cq.z), src); j.w = (uint32_t)__shfl(__float_as_int(cq.w), src);
        w.x = __shfl(cq.x, src + 1); w.y = __shfl(cq.y, src + 1); w.z = __shfl(cq.z, src + 1); w.w = __shfl(cq.w, src + 1);
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (listed && o.l8 < (WRITE ? 6u : 3u)) {
            float b[kOpWords] = {};                                      // the blended record: m for a vertex lane, nm for a normal lane
            if (o.l8 < 3u) {
#pragma unroll
                for (int e = 0; e < 12; e++) b[kOpM + e] = blend(J, j, w, kOpM + e);
            } else {
#pragma unroll
                for (int e = 0; e < 9; e++) b[kOpNm + e] = blend(J, j, w, kOpNm + e);
            }
            r = transform_row(b, o.l8, p);
            if (WRITE) live[(size_t)tri * kLiveQ + o.l8] = r;
        }
        if (!WRITE) worst = check_tail(o, r, listed, own, base, worst);
    }
    if (!WRITE && o.lane == 0u && worst != kNone) atomicMin(first_bad, list[worst]);   // (the list ascends: the smallest entry is the smallest triangle)
}

uint32_t *head_of(ptmi_ctx *c) { return static_cast<uint32_t *>(c->buf[kSkinJoints]); }

// one pass over the whole list: the LDS instantiation up to kLdsJoints joints, the global-memory one above
template <bool WRITE>
int run_pass(ptmi_ctx *c) {
    const uint32_t n = c->skin.n_skinned, nj = c->skin.n_joints;
    const bool lds = nj <= kLdsJoints;
    const auto kernel = lds ? k_skin<WRITE, true> : k_skin<WRITE, false>;
    kernel<<<pose_blocks(n, c->n_cu), TB, lds ? (size_t)nj * sizeof(ptmi_joint_transform) : 0, c->stream>>>(
        n, static_cast<const uint32_t *>(c->buf[kSkinList]), static_cast<const float4 *>(c->buf[kSkinCorners]),
        static_cast<const float4 *>(c->buf[kSkinRest]),
        reinterpret_cast<const float4 *>(static_cast<const char *>(c->buf[kSkinJoints]) + kPoseHeadBytes), nj,
        reinterpret_cast<float4 *>(const_cast<ptmi_triangle *>(c->sc.tris)), c->sc.own, head_of(c));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

}  // namespace

int pt_check_skin(const ptmi_ctx *c, const uint32_t *triangle, const ptmi_skin_corner *corners, uint32_t n, uint32_t n_joints,
                  std::string &err) {
    if (!c->have_scene) return fail(err, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if (!triangle || n == 0u) return PTMI_OK;                       // a removal
    if (!corners) return fail(err, PTMI_E_INVALID, "corners is NULL");
    if (n_joints == 0u) return fail(err, PTMI_E_INVALID, "n_joints is 0");
    if (n_joints > kMaxJoints) return fail(err, PTMI_E_UNSUPPORTED, "%u joints: at most %u", n_joints, kMaxJoints);
    for (uint32_t i = 0; i < n; i++) {
        if (triangle[i] >= c->sc.n_tris) return fail(err, PTMI_E_INVALID, "entry %u names triangle %u of %u", i, triangle[i], c->sc.n_tris);
        if (i && triangle[i] <= triangle[i - 1]) return fail(err, PTMI_E_INVALID, "entry %u: the list is not strictly ascending", i);
        for (int k = 0; k < 3; k++) {
            const ptmi_skin_corner &q = corners[3 * (size_t)i + k];
            for (int s = 0; s < 4; s++) {
                if (q.joint[s] >= n_joints) return fail(err, PTMI_E_INVALID, "entry %u corner %d names joint %u of %u", i, k, q.joint[s], n_joints);
                if (!std::isfinite(q.weight[s])) return fail(err, PTMI_E_INVALID, "entry %u corner %d: a weight is not finite", i, k);
            }
        }
    }
    return PTMI_OK;
}

int pt_check_skin_pose(const ptmi_ctx *c, const ptmi_joint_transform *joints, uint32_t n_joints, std::string &err) {
    if (!c->skin.present) return fail(err, PTMI_E_STATE, "no skin is in place (ptmi_set_skin)");
    if (!joints) return fail(err, PTMI_E_INVALID, "joints is NULL");
    if (n_joints != c->skin.n_joints) return fail(err, PTMI_E_INVALID, "%u joints: the skin was set with %u", n_joints, c->skin.n_joints);
    return check_matrix_records(joints, n_joints, "joint", "ptmi_joint_transform", err, [&](uint32_t i, const ptmi_joint_transform &o) -> int {
        if (o.group != i) return fail(err, PTMI_E_INVALID, "record %u names joint %u: a pose lists every joint in order", i, o.group);
        return PTMI_OK;
    });
}

PT_HOST {

void skin_forget(ptmi_ctx *c) {
    for (SceneBuf k : {kSkinList, kSkinCorners, kSkinRest, kSkinJoints}) dfree(c->buf[k]);
    c->skin_list.clear();
    c->skin = {};
}

int skin_rebase(ptmi_ctx *c, uint32_t first, uint32_t count) {
    if (!c->skin.present) return PTMI_OK;
    const auto &l = c->skin_list;
    const uint32_t e0 = (uint32_t)(std::lower_bound(l.begin(), l.end(), first) - l.begin());
    const uint64_t end = (uint64_t)first + count;
    const uint32_t e1 = end > kNone ? (uint32_t)l.size() : (uint32_t)(std::lower_bound(l.begin(), l.end(), (uint32_t)end) - l.begin());
    return pose_snapshot(c, e0, e1 - e0, c->buf[kSkinList], c->buf[kSkinRest]);
}

}  // namespace pt_host

extern "C" {

// The new buffers exist and are filled before anything of the context changes, so a failed call keeps the previous skin.
int ptmi_set_skin(ptmi_ctx *c, const uint32_t *triangle, const ptmi_skin_corner *corners, uint32_t n, uint32_t n_joints) {
    if (!c) return PTMI_E_INVALID;
    const int rc = pt_check_skin(c, triangle, corners, n, n_joints, c->err);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    if (!triangle || n == 0u) { skin_forget(c); return morph_relink(c); }   // (a morph in place writes to the live records again)
    const size_t rec = (size_t)n * kRestQ * sizeof(float4);
    DevScratch fresh;                                               // freed on every way out but the last
    uint32_t *list = fresh.get<uint32_t>(n);
    char *corn = fresh.get<char>(rec), *rest = fresh.get<char>(rec), *jnt = fresh.get<char>(kPoseHeadBytes + (size_t)n_joints * sizeof(ptmi_joint_transform));
    hipError_t e = fresh.error;
    int rs = PTMI_OK;
    if (hip_ok(e) && hip_ok(e = hipMemcpy(list, triangle, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        hip_ok(e = hipMemcpy(corn, corners, rec, hipMemcpyHostToDevice)) && !(rs = pose_snapshot(c, 0u, n, list, rest)))
        e = hipStreamSynchronize(c->stream);
    if (rs) return rs;
    if (!hip_ok(e)) {
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "the skin could not be made: %s (the previous skin, if any, is still in place)", hipGetErrorString(e));
    }
    skin_forget(c);
    c->buf[kSkinList] = fresh.keep(list); c->buf[kSkinCorners] = fresh.keep(corn); c->buf[kSkinRest] = fresh.keep(rest);
    c->buf[kSkinJoints] = fresh.keep(jnt);
    c->skin_list.assign(triangle, triangle + n);
    c->skin.present = 1u; c->skin.n_joints = n_joints; c->skin.n_skinned = n; c->skin.first_bad = kNone;
    return morph_relink(c);                                         // a morph in place: its entries that this list names go to the new rest rows
}

int ptmi_pose_skin(ptmi_ctx *c, const ptmi_joint_transform *joints, uint32_t n_joints) {
    if (!c) return PTMI_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = pt_check_skin_pose(c, joints, n_joints, c->err);
    if (rc) return rc;
    uint32_t *head = head_of(c);
    auto stage = [&]() -> int {
        HIP_TRY(c, hipMemsetAsync(head, 0xFF, kPoseHeadBytes, c->stream));  // "none" in the check word
        HIP_TRY(c, hipMemcpy(reinterpret_cast<char *>(head) + kPoseHeadBytes, joints, (size_t)n_joints * sizeof(ptmi_joint_transform), hipMemcpyHostToDevice));
        return PTMI_OK;
    };
    auto pass = [&](bool write) { return write ? run_pass<true>(c) : run_pass<false>(c); };
    PoseCall p{stage, pass};
    p.check_word = head; p.first_bad = &c->skin.first_bad; p.how = "skinned";
    p.lo = c->skin_list.front(); p.hi = c->skin_list.back();       // from the lowest to the highest listed triangle
    if ((rc = pose_refusable(c, t0, p))) return rc;
    c->skin.poses++; c->skin.first_bad = kNone;
    c->morph.skin_stale = 0u;                                       // what ptmi_pose_morph left in the rest rows is in the live records now
    c->skin.pose_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PTMI_OK;
}

int ptmi_skin_status(ptmi_ctx *c, struct ptmi_skin_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->skin;
    return PTMI_OK;
}

}  // extern "C"
