// pt_transform.h — what scene_transform.hip (triangle groups), scene_skin.hip (skinning) and, for the layout, the check tail and the
// constants, scene_morph.hip (morph targets) share on the device: one float4 of a rest
// record through a 96-byte matrix record, ptmi_update_triangles' checks on a transformed vertex, the eight-lanes-per-record layout of
// their kernels and the tail of their check pass, and the constants of their launches and buffers. Said once so that the two features
// cannot disagree on a bit (include/ptmi.h ptmi_transform_groups has the formulas). The snapshot kernel and the host sequence they share
// are scene_pose.hip's. Device code but for the constants and pose_blocks, the one host function (the grid of a launch).
#pragma once
#include "ptmi.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

static_assert(sizeof(ptmi_group_transform) == 96 && sizeof(ptmi_group_transform) % sizeof(float4) == 0, "a matrix record is 6 float4");
constexpr int kRestQ = 6;                    // float4 per triangle of a rest pose: v0, v1, v2, n0, n1, n2
constexpr int kLiveQ = (int)(sizeof(ptmi_triangle) / sizeof(float4));
constexpr int kOpQ = (int)(sizeof(ptmi_group_transform) / sizeof(float4));
constexpr int kOpWords = kOpQ * 4;
constexpr int kOpM = (int)(offsetof(ptmi_group_transform, m) / sizeof(float));
constexpr int kOpNm = (int)(offsetof(ptmi_group_transform, nm) / sizeof(float));

constexpr int TB = 256;                      // threads per block of every kernel here
constexpr uint32_t kOctets = TB / 8;         // records per block and round: eight lanes each
constexpr uint32_t kNone = 0xFFFFFFFFu;
// buf[kGroupMap] and buf[kSkinJoints] begin with this many words, the records of the call (the group -> op map; the joints) follow.
// Word 0 is the CHECK WORD: the smallest offending triangle of the check pass, kNone before it and while it has found none.
constexpr uint32_t kPoseHead = 4u;
constexpr size_t kPoseHeadBytes = kPoseHead * sizeof(uint32_t);
// the blocks of a pass over `slots` records: one round each, or 8 per compute unit that stride over the rest
inline dim3 pose_blocks(uint32_t slots, int n_cu) { return dim3(std::min((slots + kOctets - 1) / kOctets, (uint32_t)std::max(1, n_cu) * 8u)); }

__device__ __forceinline__ bool finite1(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }

// one float4 of the rest record through the op o (24 words): q < 3 a vertex, else a normal. The arithmetic of include/ptmi.h.
__device__ __forceinline__ float4 transform_row(const float *o, uint32_t q, float4 p) {
    float4 r;
    if (q < 3u) {
        const float *m = o + kOpM;
        r.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
        r.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
        r.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
    } else {
        const float *nm = o + kOpNm;
        const float qx = (nm[0] * p.x + nm[1] * p.y) + nm[2] * p.z;
        const float qy = (nm[3] * p.x + nm[4] * p.y) + nm[5] * p.z;
        const float qz = (nm[6] * p.x + nm[7] * p.y) + nm[8] * p.z;
        const float l2 = (qx * qx + qy * qy) + qz * qz;
        r.x = qx; r.y = qy; r.z = qz;
        if (l2 > 0.0f) {
            const float len = __builtin_sqrtf(l2);                  // correctly rounded, as '/' is (pt_math.h)
            r.x = qx / len; r.y = qy / len; r.z = qz / len;
        }
    }
    r.w = p.w;                                                       // the padding word keeps its bits
    return r;
}
// scene_update.hip's checks on one transformed vertex b beside the first, a (b is a itself for the first)
__device__ __forceinline__ bool vertex_bad(float4 a, float4 b, bool edge) {
    bool bad = !finite1(b.x) || !finite1(b.y) || !finite1(b.z);
    if (edge) bad = bad || !finite1(a.x + (b.x - a.x)) || !finite1(a.y + (b.y - a.y)) || !finite1(a.z + (b.z - a.z));
    return bad;
}

// Where a thread stands when eight lanes share a record, one float4 each (lanes 0-2 a vertex, 3-5 a normal, 6 and 7 idle, so that a
// wave covers 8 records and stores whole 128-byte lines): its lane in the wave and in the octet, the octet's first lane (whose words
// the others take by __shfl), and the octet's slot in the block. A block's round covers slots [base, base + kOctets).
struct Octet {
    uint32_t lane, l8, head, slot;
};
__device__ __forceinline__ Octet octet_here() { return {threadIdx.x & 63u, threadIdx.x & 7u, threadIdx.x & 63u & ~7u, threadIdx.x >> 3}; }
__device__ __forceinline__ uint32_t octet_stride() { return gridDim.x * kOctets; }

// The tail of a check pass's round; EVERY lane of the wave calls it. r: what this lane made of its float4 (lanes 0-2 of an octet hold
// a = v0', b and d); active: the octet has a record this pass moves; base: the first slot of the block's round. Returns `worst`, the
// smallest offending slot this wave has seen, with this round's folded in: lane 0 of the wave sends it on after the last round, once
// it is a triangle. Relies on two things: slots ascend with the lane, so the lowest set bit of the ballot is the wave's smallest
// offender; and no lane has returned early, so every __shfl and the ballot see the whole wave.
__device__ __forceinline__ uint32_t check_tail(const Octet &o, float4 r, bool active, uint32_t own, uint32_t base, uint32_t worst) {
    const float4 a = make_float4(__shfl(r.x, (int)o.head), __shfl(r.y, (int)o.head), __shfl(r.z, (int)o.head), 0.0f);
    const bool bad = active && o.l8 < 3u && vertex_bad(a, r, own && o.l8 != 0u);
    const unsigned long long mask = __ballot(bad);
    if (mask) {
        const uint32_t l = (uint32_t)__ffsll((long long)mask) - 1u;
        worst = min(worst, base + ((threadIdx.x & ~63u) >> 3) + (l >> 3));
    }
    return worst;
}
