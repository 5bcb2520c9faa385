// wide_node.h — the 64-byte wide node (layout: pt_device.h) taken apart and put together, and the quantisation of one child box onto
// the scene's 16-bit grid. The ONE definition of both for the host builders (fast_tree.hip), the host quantisers (quantise.hip), the
// device builder (own_tree_gpu.hip) and the scene image (scene_image.hip).
//
// Soundness rule of the grid: a quantised box, decoded with the very fmaf the kernels evaluate (traverse.hip, traverse_own.hip:
// fmaf(scale, plane, origin)), contains the exact box. Products and sums in double without contraction: host and device decide alike.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

__host__ __device__ inline uint32_t pt_float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
__host__ __device__ inline float pt_bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

struct PtWideChild { float lo[3], hi[3]; uint32_t ref; };

// child `side` (0 left, 1 right) of the wide node at w[0..3]
__host__ __device__ inline PtWideChild pt_wide_child(const float4 *w, int side) {
    if (side == 0) return {{w[0].x, w[0].y, w[0].z}, {w[0].w, w[1].x, w[1].y}, pt_float_bits(w[3].x)};
    return {{w[1].z, w[1].w, w[2].x}, {w[2].y, w[2].z, w[2].w}, pt_float_bits(w[3].y)};
}
__host__ __device__ inline uint32_t pt_wide_ref(const float4 *w, int side) { return pt_float_bits(side ? w[3].y : w[3].x); }
__host__ __device__ inline void pt_wide_set_ref(float4 *w, int side, uint32_t ref) { (side ? w[3].y : w[3].x) = pt_bits_float(ref); }
__host__ __device__ inline void pt_wide_set_box(float4 *w, int side, const float *lo, const float *hi) {
    if (side == 0) { w[0] = make_float4(lo[0], lo[1], lo[2], hi[0]); w[1].x = hi[1]; w[1].y = hi[2]; }
    else { w[1].z = lo[0]; w[1].w = lo[1]; w[2] = make_float4(lo[2], hi[0], hi[1], hi[2]); }
}
// the whole node: both boxes, both references, the two spare words zero
__host__ __device__ inline void pt_wide_pack(float4 *w, const float *llo, const float *lhi, uint32_t lref, const float *rlo,
                                             const float *rhi, uint32_t rref) {
    w[0] = make_float4(llo[0], llo[1], llo[2], lhi[0]);
    w[1] = make_float4(lhi[1], lhi[2], rlo[0], rlo[1]);
    w[2] = make_float4(rlo[2], rhi[0], rhi[1], rhi[2]);
    w[3] = make_float4(pt_bits_float(lref), pt_bits_float(rref), 0.0f, 0.0f);
}

// The grid of a quantised image: plane k of an axis lies at fmaf(scale, k, origin), k = 0 .. 65535 (pt_quant_grid makes it).
struct PtQuantGrid { float origin[3], scale[3]; };

__host__ __device__ inline float pt_plane(const PtQuantGrid &g, int k, uint32_t u) { return fmaf(g.scale[k], (float)u, g.origin[k]); }
// a plane number whose plane is <= v / >= v: the quotient in double, rounded outward, then moved outward while the kernels' fmaf puts
// its plane on the wrong side of v. It is the nearest such plane except where the neighbour's plane ROUNDS onto v itself while the
// quotient stays short of it: then one plane further out, which is as sound.
__host__ __device__ inline uint32_t pt_plane_lo(const PtQuantGrid &g, int k, float v) {
    if (!(g.scale[k] > 0.0f)) return 0u;
    const double q = floor(((double)v - (double)g.origin[k]) / (double)g.scale[k]);
    uint32_t u = q <= 0.0 ? 0u : q >= 65535.0 ? 65535u : (uint32_t)q;
    while (u > 0u && pt_plane(g, k, u) > v) u--;
    return u;
}
__host__ __device__ inline uint32_t pt_plane_hi(const PtQuantGrid &g, int k, float v) {
    if (!(g.scale[k] > 0.0f)) return 0u;
    const double q = ceil(((double)v - (double)g.origin[k]) / (double)g.scale[k]);
    uint32_t u = q <= 0.0 ? 0u : q >= 65535.0 ? 65535u : (uint32_t)q;
    while (u < 65535u && pt_plane(g, k, u) < v) u++;
    return u;
}

__host__ __device__ inline double pt_box_area(const float *lo, const float *hi) {
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return 2.0 * (x * y + y * z + z * x);
}

// One child box [lo, hi] on the grid. q: lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16, `ref` (what the quantised image is
// to hold for this child). growth: by how much the decoded box's surface area exceeds the exact one's, relative, at most 1e6; counted
// (grown) only when the exact box has an area. The areas are finite (extents of finite floats, in double), so no NaN reaches the cap.
struct PtQuantChild { uint4 q; double growth; bool grown; };
__host__ __device__ inline PtQuantChild pt_quantise_child(const PtQuantGrid &g, const float *lo, const float *hi, uint32_t ref) {
    uint32_t ql[3], qh[3];
    float dl[3], dh[3];
    for (int k = 0; k < 3; k++) {
        ql[k] = pt_plane_lo(g, k, lo[k]); qh[k] = pt_plane_hi(g, k, hi[k]);
        dl[k] = pt_plane(g, k, ql[k]); dh[k] = pt_plane(g, k, qh[k]);
    }
    PtQuantChild r{make_uint4(ql[0] | (ql[1] << 16), ql[2] | (qh[0] << 16), qh[1] | (qh[2] << 16), ref), 0.0, false};
    const double a0 = pt_box_area(lo, hi);
    if (a0 > 0.0) { const double t = pt_box_area(dl, dh) / a0 - 1.0; r.growth = 1e6 < t ? 1e6 : t; r.grown = true; }
    return r;
}
