// pt_transform.h — the arithmetic scene_transform.hip (triangle groups) and scene_skin.hip (skinning) share: one float4 of a rest record
// through a 96-byte matrix record, and ptmi_update_triangles' checks on a transformed vertex. Device code; said once so that the two
// features cannot disagree on a bit (include/ptmi.h ptmi_transform_groups has the formulas).
#pragma once
#include "ptmi.h"

#include <cstddef>
#include <cstdint>

static_assert(sizeof(ptmi_group_transform) == 96 && sizeof(ptmi_group_transform) % sizeof(float4) == 0, "a matrix record is 6 float4");
constexpr int kRestQ = 6;                    // float4 per triangle of a rest pose: v0, v1, v2, n0, n1, n2
constexpr int kLiveQ = (int)(sizeof(ptmi_triangle) / sizeof(float4));
constexpr int kOpQ = (int)(sizeof(ptmi_group_transform) / sizeof(float4));
constexpr int kOpWords = kOpQ * 4;
constexpr int kOpM = (int)(offsetof(ptmi_group_transform, m) / sizeof(float));
constexpr int kOpNm = (int)(offsetof(ptmi_group_transform, nm) / sizeof(float));

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
