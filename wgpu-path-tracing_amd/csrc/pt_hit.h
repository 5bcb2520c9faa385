// pt_hit.h — where on its triangle a hit lies, shared by the kernels that ask: `shade` (shade.hip) for the shading state of a hit, the
// alpha-cutout resolve kernels (alpha.hip) for the hole test and the distance along the original ray, k_hit_uv (reproject.hip) for
// ptmi_debug_intersect and the motion-aware reprojection.
//
// The hit record carries (t, triangle) only. The barycentric (u, v) are the ones `extend` computed when it accepted the hit,
// recomputed by the same tri_test (pt_math.h) on the same operands: e1 and e2 are the same single IEEE subtractions the traversal
// image was built with (scene_image.hip). Every caller gets them from tri_hit, so they agree with `extend` and with each other bit
// for bit.
#pragma once
#include "pt_device.h"
#include "pt_math.h"

namespace {

PT_DEV v3 ld3(const float *p) { return mk3(p[0], p[1], p[2]); }

// tri_test's t (-1 where it rejects the hit) and (u, v), which stand either way, for the ray (ro, rd) and the triangle (v0, v1, v2);
// e1, e2 for the caller that goes on with them
PT_DEV float tri_hit(v3 v0, v3 v1, v3 v2, v3 ro, v3 rd, float &u, float &v, v3 &e1, v3 &e2) {
    e1 = sub3(v1, v0); e2 = sub3(v2, v0);
    return tri_test(v0, e1, e2, ro, rd, u, v);
}
PT_DEV float tri_hit(const ptmi_triangle &T, v3 ro, v3 rd, float &u, float &v) {
    v3 e1, e2;
    return tri_hit(ld3(T.v0), ld3(T.v1), ld3(T.v2), ro, rd, u, v, e1, e2);
}

// One texture coordinate at (u, v) from its values c0, c1, c2 at the vertices: rayTriangleIntersect's interpolation, pt.wgsl:159-226
PT_DEV float hit_texcoord(float c0, float c1, float c2, float u, float v) {
    const float w = 1.0f - u - v;
    return fma1(c2, v, fma1(c1, u, c0 * w));
}

}  // namespace
