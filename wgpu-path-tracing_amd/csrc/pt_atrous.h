// pt_atrous.h — the edge-avoiding a-trous pass that denoise.hip (the camera's frame) and bake_denoise.hip (a lightmap) both run, said
// once over a guide policy, and the launches of a filter's passes. Each of the two files states its own arithmetic in its header
// comment, in the order its numpy model restates it; what is here is the part the two statements have word for word in common:
// the 64 x 4 workgroup, g3x3 of the variance, the 5x5 B3-spline taps walked dy outer / dx inner, w_n and w_l, the five running
// sums from the centre's h0^2, and the divisions.
//
// Both filters keep a guide plane of (unit normal, one float of their own) per pixel whose normal is all zero where the pixel has no
// surface (a miss; an uncovered texel). Such a pixel is never a tap and is never filtered. A policy adds what else its filter knows:
//   kMasked           the surface-less pixels carry no data at all: they are not read (g3x3 skips them, and a tap's guide is tested
//                     before its colour is loaded), and they are not written except by the last pass, which writes zeros.
//                     false: such a pixel is a value like any other to g3x3 and every pass writes it through, the last pass's
//                     epilogue included.
//   Centre, centre()  what the centre keeps for its taps beside its guide, loaded once
//   weight()          the one geometric weight of tap qi against the centre, at `off` = |(dx, dy)| step pixels
//   finish()          the last pass's epilogue on the value about to be written
// (An LDS-tiled form for steps 1 and 2 was not built.)
#pragma once
#include "pt_device.h"
#include "pt_math.h"

#include <utility>

namespace pt_atrous {

constexpr int DX = 64, DY = 4;          // a wave is one 64-pixel row segment: every tap row of a plane is one coalesced 1 KiB load
inline dim3 block() { return dim3(DX, DY); }
inline dim3 grid(uint32_t W, uint32_t H) { return dim3((W + DX - 1) / DX, (H + DY - 1) / DY); }

PT_DEV float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV bool finite4(float4 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && __builtin_isfinite(v.w);
}
PT_DEV bool nonzero3(float4 g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f; }

// LAST: the final pass, which ends with the policy's epilogue; the others write (rgb, variance)
template <class Guide, bool LAST>
__global__ __launch_bounds__(DX * DY) void k_pass(uint32_t W, uint32_t H, uint32_t step, float phi_c, float phi_n,
                                                  const float4 *__restrict__ guide, const Guide G, const float4 *__restrict__ src,
                                                  float4 *__restrict__ dst) {
    const uint32_t x = blockIdx.x * DX + threadIdx.x, y = blockIdx.y * DY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 gp = guide[i];
    const bool surface = nonzero3(gp);
    if (Guide::kMasked && !surface) {
        if (LAST) dst[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 cp = src[i];
    float4 o = cp;
    if (surface && finite4(cp)) {
        // g3x3(var): the centre is one of its taps, so the weight sum is at least 1/4
        float sv = 0.0f, sk = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = (int)y + dy;
            if (qy < 0 || qy >= (int)H) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = (int)x + dx;
                if (qx < 0 || qx >= (int)W) continue;
                const size_t qi = (size_t)qy * W + qx;
                if (Guide::kMasked && !nonzero3(guide[qi])) continue;
                const float4 q = src[qi];
                if (!finite4(q)) continue;
                const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                sv = sv + k * q.w;
                sk = sk + k;
            }
        }
        const float lp = lum(cp.x, cp.y, cp.z);
        const float den_l = phi_c * __builtin_sqrtf(sv / sk) + 1e-6f;
        const typename Guide::Centre at = G.centre(i, gp);
        constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const float w0 = h[2] * h[2];
        float sw = w0, sr = w0 * cp.x, sg = w0 * cp.y, sb = w0 * cp.z, s2 = w0 * w0 * cp.w;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = (int)y + dy * (int)step;
            if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int qx = (int)x + dx * (int)step;
                if (qx < 0 || qx >= (int)W) continue;
                const size_t qi = (size_t)qy * W + qx;
                const float4 gq = guide[qi];
                if (Guide::kMasked && !nonzero3(gq)) continue;
                const float4 q = src[qi];
                if (!finite4(q) || !nonzero3(gq)) continue;
                const float wn = __builtin_powf(max1(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z), phi_n);
                const float off = (float)step * __builtin_sqrtf((float)(dx * dx + dy * dy));
                const float wg = G.weight(at, gp, gq, qi, off);
                const float wl = __builtin_expf(-__builtin_fabsf(lp - lum(q.x, q.y, q.z)) / den_l);
                const float w = h[dy + 2] * h[dx + 2] * wn * wg * wl;
                sw = sw + w;
                sr = sr + w * q.x; sg = sg + w * q.y; sb = sb + w * q.z;
                s2 = s2 + w * w * q.w;
            }
        }
        o = make_float4(sr / sw, sg / sw, sb / sw, s2 / (sw * sw));
    }
    if (LAST) G.finish(i, o);
    dst[i] = o;
}

// The passes of one filter on stream s, its prepass already queued: a holds (rgb, variance) and guide the guide plane. p.iterations
// (at least 1) passes of step 1, 2, 4, ... ping-pong between a and b, and the last one writes `out`, or the spare one of the two
// planes where out is NULL. Returns the plane the result is in.
template <class Guide>
float4 *launch_passes(hipStream_t s, const AtrousArgs &p, const float4 *guide, const Guide &G, float4 *a, float4 *b, float4 *out) {
    float4 *src = a, *spare = b;
    for (uint32_t it = 0; it + 1u < p.iterations; it++) {
        hipLaunchKernelGGL((k_pass<Guide, false>), grid(p.W, p.H), block(), 0, s, p.W, p.H, 1u << it, p.phi_color, p.phi_normal, guide, G,
                           src, spare);
        std::swap(src, spare);
    }
    float4 *const to = out ? out : spare;
    hipLaunchKernelGGL((k_pass<Guide, true>), grid(p.W, p.H), block(), 0, s, p.W, p.H, 1u << (p.iterations - 1u), p.phi_color, p.phi_normal,
                       guide, G, src, to);
    return to;
}

}  // namespace pt_atrous
