// pt_box.h — the box arithmetic of the tree builders, said once: the host builder (fast_tree.hip), the device builders (gpu_tree.hip,
// own_tree_gpu.hip) and the refit (scene_update.hip) promise each other's results bit for bit, and these are the pieces that promise
// rests on. Plain float and double operations in a fixed order, compiled without contraction like everything else. Nothing but those
// four files includes this header: the traversal and shade files have no use for it.
#pragma once
#include "fast_tree.h"
#include "wide_node.h"

#include <float.h>

#ifndef PT_OWN_PAD_LOG2
#define PT_OWN_PAD_LOG2 (-16)        /* own leaves' boxes grow by 2^this x the largest coordinate magnitude of the scene */
#endif

struct Box6 { float mn[3], mx[3]; };

// std::min / std::max exactly: the first argument unless the second is strictly smaller / larger (NaN and -0 / +0 behave as there)
__host__ __device__ inline float pt_min(float a, float b) { return b < a ? b : a; }
__host__ __device__ inline float pt_max(float a, float b) { return a < b ? b : a; }

__host__ __device__ inline Box6 pt_empty_box() { return {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }
__host__ __device__ inline Box6 pt_unite(const Box6 &a, const float *lo, const float *hi) {
    Box6 u;
    for (int k = 0; k < 3; k++) { u.mn[k] = pt_min(a.mn[k], lo[k]); u.mx[k] = pt_max(a.mx[k], hi[k]); }
    return u;
}
__host__ __device__ inline Box6 pt_unite(const Box6 &a, const Box6 &b) { return pt_unite(a, b.mn, b.mx); }
__host__ __device__ inline double pt_box_area(const Box6 &b) { return pt_box_area(b.mn, b.mx); }
__host__ __device__ inline Box6 pt_child_box(const float4 *w, int side) {          // child `side` of the wide node at w[0..3]
    const PtWideChild c = pt_wide_child(w, side);
    return {{c.lo[0], c.lo[1], c.lo[2]}, {c.hi[0], c.hi[1], c.hi[2]}};
}

// ---- own leaves: the outward padding (fast_tree.h) -------------------------------------------------------------
// a bound moved outward by pad, and by one float where pad is too small to move it
__host__ __device__ inline float pt_pad_lower(float x, float pad) { const float y = x - pad; return y < x ? y : nextafterf(x, -INFINITY); }
__host__ __device__ inline float pt_pad_upper(float x, float pad) { const float y = x + pad; return y > x ? y : nextafterf(x, INFINITY); }
__host__ __device__ inline Box6 pt_pad_box(const Box6 &b, float pad) {
    Box6 p;
    for (int k = 0; k < 3; k++) { p.mn[k] = pt_pad_lower(b.mn[k], pad); p.mx[k] = pt_pad_upper(b.mx[k], pad); }
    return p;
}
// pad and safe_origin of a scene whose unit boxes reach `biggest` = max |coordinate| (extra_log2: experiments only). false: pad is not
// finite. The rounding of the fused tests stays below a quarter of the padding for origins up to safe_origin.
inline bool pt_own_padding(double biggest, float &pad, float &safe_origin, int extra_log2 = 0) {
    pad = pt_max((float)ldexp(biggest, PT_OWN_PAD_LOG2 + extra_log2), FLT_MIN);
    const double so = 8.0 * biggest;
    safe_origin = (float)(3.0e38 < so ? 3.0e38 : so);
    return isfinite(pad);
}

// ---- own leaves: the unit box of one listed triangle ---------------------------------------------------------------------------------
// The box of a, b, c and of a + (b - a), a + (c - a) as the intersection test sees them; a sliver's (fast_tree.h pt_own_sliver) grown by
// the box of its reference leaf, which leaf_box() fetches (it is not called for any other triangle). biggest: the bits of max
// |coordinate| of the result, taken after that union (an uploaded tree's leaf box may reach beyond its triangles, and the padding must
// cover what is walked); non-negative floats order as their bits. bad: a coordinate or a sum is not finite (the box is not to be used).
struct PtUnitBox { Box6 box; uint32_t biggest; bool bad; };
template <class LeafBox>
__host__ __device__ inline PtUnitBox pt_unit_box(const float *a, const float *b, const float *c, LeafBox leaf_box) {
    PtUnitBox u{{}, 0u, false};
    for (int k = 0; k < 3; k++) {
        const float b2 = a[k] + (b[k] - a[k]), c2 = a[k] + (c[k] - a[k]);
        if (!isfinite(a[k]) || !isfinite(b[k]) || !isfinite(c[k]) || !isfinite(b2) || !isfinite(c2)) u.bad = true;
        u.box.mn[k] = pt_min(pt_min(pt_min(a[k], b[k]), pt_min(c[k], b2)), c2);
        u.box.mx[k] = pt_max(pt_max(pt_max(a[k], b[k]), pt_max(c[k], b2)), c2);
    }
    if (pt_own_sliver(a, b, c)) u.box = pt_unite(u.box, leaf_box());
    for (int k = 0; k < 3; k++) {
        const uint32_t lo = pt_float_bits(fabsf(u.box.mn[k])), hi = pt_float_bits(fabsf(u.box.mx[k]));
        u.biggest = u.biggest < lo ? lo : u.biggest;
        u.biggest = u.biggest < hi ? hi : u.biggest;
    }
    return u;
}
// the reference leaf's box of original triangle `orig` in the per-triangle table (min.xyz, 0), (max.xyz, 0)
__host__ __device__ inline Box6 pt_leafbox_row(const float4 *leafbox, uint32_t orig) {
    const float4 lo = leafbox[2 * (size_t)orig], hi = leafbox[2 * (size_t)orig + 1];
    return {{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
}

// ---- order-preserving float <-> uint (min / max reductions with integer atomics) ------------------------------------------------------
__host__ __device__ inline uint32_t pt_ord(float f) { const uint32_t u = pt_float_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float pt_unord_f(uint32_t u) { return pt_bits_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// ---- Morton codes ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t pt_expand10(uint32_t v) {          // 10 bits -> every third bit
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
// 1 / (hi - lo) of the centroid bounds on one axis, 0 where that is no finite positive number
inline float pt_inv_extent(float lo, float hi) { const float e = hi - lo; return (e > 0.0f && isfinite(1.0f / e)) ? 1.0f / e : 0.0f; }
// the 30-bit code of the centroid of [mn, mx] on the centroid bounds (lo, inv = pt_inv_extent per axis): 10 bits per axis, clamped, NaN -> 0
__host__ __device__ inline uint32_t pt_morton30(const float *mn, const float *mx, float3 lo, float3 inv) {
    const float cx = (0.5f * mn[0] + 0.5f * mx[0] - lo.x) * inv.x;
    const float cy = (0.5f * mn[1] + 0.5f * mx[1] - lo.y) * inv.y;
    const float cz = (0.5f * mn[2] + 0.5f * mx[2] - lo.z) * inv.z;
    auto q = [](float v) { v = v * 1024.0f; v = v < 0.0f ? 0.0f : (v > 1023.0f ? 1023.0f : v); return (uint32_t)v; };
    return (pt_expand10(q(cx)) << 2) | (pt_expand10(q(cy)) << 1) | pt_expand10(q(cz));
}
