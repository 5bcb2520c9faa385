// bake_denoise.hip — ptmi_bake_denoise (include/ptmi.h): an edge-avoiding a-trous wavelet filter over a baked lightmap,
// guided by the bake surface instead of by first-hit planes. It reads the surface's records, the output buffer and the sample-moments
// plane and writes context-owned planes; none of its inputs are written. The gutter fill that follows it is bake.hip's kernel.
// No counterpart in the reference, which renders from a camera only.
//
// T = the surface's record of a texel (position P, covered flag, normal), R = the output buffer, M = the moments plane.
//   prepass   uncovered texel: guide N = guide P = cv = 0. Covered texel:
//               len2 = nx nx + ny ny + nz nz;  len = sqrt(len2);  n^ = (nx / len, ny / len, nz / len)
//               f = the smallest non-zero |P - P_q| over the covered 4-neighbours q inside the map, taken in the order x - 1, x + 1,
//                   y - 1, y + 1, with |d| = sqrt(dx dx + dy dy + dz dz); 0 if there is none (the texel's footprint in the scene)
//               guide N = (n^, f);  guide P = (P, 1);  cv = (R.rgb, max(0, M.y - M.x M.x) / max(M.z, 1))
//   pass i    step = 2^i. A covered centre p with a finite cv takes the 5x5 B3-spline taps h = (1/16, 1/4, 3/8, 1/4, 1/16) at offsets
//             (dx, dy) step, dy outer, dx inner, those q that are inside the map, covered (guide N non-zero) and finite:
//               w_n = pow(max(0, n^_p.x n^_q.x + n^_p.y n^_q.y + n^_p.z n^_q.z), phi_normal)
//               D = P_q - P_p;  dist = sqrt(D.x D.x + D.y D.y + D.z D.z);  plane = |n^_p.x D.x + n^_p.y D.y + n^_p.z D.z|
//               off = (float)step * sqrt((float)(dx dx + dy dy));  e = max(plane, dist - kStretch * off * f_p)
//               w_x = exp(-e / (phi_position * f_p + 1e-6))
//               w_l = exp(-|l_p - l_q| / (phi_color * sqrt(g3x3(var)_p) + 1e-6)),  l = 0.2126 r + 0.7152 g + 0.0722 b
//               w = h[dy] * h[dx] * w_n * w_x * w_l
//             colour = sum w c / sum w, var = sum w^2 var / (sum w)^2, the sums starting from the centre's h0^2 (and h0^4 var) and
//             growing in tap order. g3x3 is the (1/4, 1/8, 1/16) Gaussian of the variance over the 3x3 texels (at distance 1, whatever
//             the step) that are inside the map, covered and finite, divided by the sum of their weights; the centre is one of them.
//             A covered centre that is not finite keeps its value. An uncovered centre is neither read nor, before the last pass, written.
//   last pass writes (rgb, 1) for a covered texel and (0, 0, 0, 0) for every other: the masked plane bake.hip's k_bake_mask makes.
// kStretch = 4 is the chart stretch the filter tolerates: a tap on the centre's plane closer than kStretch footprints per texel of
// offset has e = 0 and pays no penalty; a parallel surface is cut by `plane`, a far part of the same plane by `dist`.
// Every expression is written in the order tests/bake_denoise_ref.py restates it; the library builds with -ffp-contract=off, so the
// only differences to a float32 numpy restatement are exp and pow (a few ulp).
//
// The kernels are the plain global-memory form: 64 x 4 workgroups, so a wave is one 64-texel row segment and every tap row of a plane
// is one coalesced 1 KiB load. A lane whose texel is uncovered leaves after its guide load, so a wave of 64 uncovered texels retires
// there; a tap whose guide N is zero loads neither its position nor its colour. The pass itself is pt_atrous.h's, shared with
// denoise.hip; what is the lightmap's own is the prepass and SurfaceGuide below: w_x, and the uncovered texels masked out.
#include "ptmi_ctx.h"
#include "pt_atrous.h"

#include <algorithm>

namespace {

using namespace pt_atrous;

constexpr float kStretch = 4.0f;

PT_DEV float len3(float x, float y, float z) { return __builtin_sqrtf(x * x + y * y + z * z); }

__global__ __launch_bounds__(DX * DY) void k_bd_prepass(uint32_t W, uint32_t H, const float4 *__restrict__ texels,
                                                        const float4 *__restrict__ radiance, const float4 *__restrict__ moments,
                                                        float4 *__restrict__ guide_n, float4 *__restrict__ guide_p,
                                                        float4 *__restrict__ cv) {
    const uint32_t x = blockIdx.x * DX + threadIdx.x, y = blockIdx.y * DY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 tp = texels[2 * i];
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (__float_as_uint(tp.w) == 0u) {
        guide_n[i] = zero; guide_p[i] = zero; cv[i] = zero;
        return;
    }
    const float4 n = texels[2 * i + 1];
    const float len = len3(n.x, n.y, n.z);
    float f = 0.0f;
    auto neighbour = [&](size_t q) {
        const float4 tq = texels[2 * q];
        if (__float_as_uint(tq.w) == 0u) return;
        const float d = len3(tp.x - tq.x, tp.y - tq.y, tp.z - tq.z);
        if (d > 0.0f && (f == 0.0f || d < f)) f = d;
    };
    if (x > 0u) neighbour(i - 1);
    if (x + 1u < W) neighbour(i + 1);
    if (y > 0u) neighbour(i - W);
    if (y + 1u < H) neighbour(i + W);
    const float4 c = radiance[i], m = moments[i];
    guide_n[i] = make_float4(n.x / len, n.y / len, n.z / len, f);
    guide_p[i] = make_float4(tp.x, tp.y, tp.z, 1.0f);
    cv[i] = make_float4(c.x, c.y, c.z, max1(0.0f, m.y - m.x * m.x) / max1(m.z, 1.0f));
}

// The guide plane is guide N = (unit normal or 0 where uncovered, footprint); guide P is the policy's own.
struct SurfaceGuide {
    const float4 *guide_p;
    float phi_x;
    static constexpr bool kMasked = true;
    struct Centre { float4 pp; float den_x; };
    PT_DEV Centre centre(size_t i, float4 gp) const { return {guide_p[i], phi_x * gp.w + 1e-6f}; }
    PT_DEV float weight(const Centre &at, float4 gp, float4, size_t qi, float off) const {
        const float4 pq = guide_p[qi];
        const float ex = pq.x - at.pp.x, ey = pq.y - at.pp.y, ez = pq.z - at.pp.z;
        const float dist = len3(ex, ey, ez);
        const float plane = __builtin_fabsf(gp.x * ex + gp.y * ey + gp.z * ez);
        const float e = max1(plane, dist - kStretch * off * gp.w);
        return __builtin_expf(-e / at.den_x);
    }
    // (rgb, 1): the masked plane bake.hip's k_bake_mask makes
    PT_DEV void finish(size_t, float4 &o) const { o.w = 1.0f; }
};

// The prepass, the passes and `dilate` passes of the gutter fill on stream s. a and b are the ping-pong planes; the result lands in
// `out` whatever the counts are: the last pass of the filter writes there when no gutter pass follows, else the last gutter pass does.
void launch(hipStream_t s, const AtrousArgs &p, uint32_t dilate, const float4 *texels, const float4 *radiance, const float4 *moments,
            float4 *guide_n, float4 *guide_p, float4 *a, float4 *b, float4 *out) {
    hipLaunchKernelGGL(k_bd_prepass, grid(p.W, p.H), block(), 0, s, p.W, p.H, texels, radiance, moments, guide_n, guide_p, a);
    float4 *src = launch_passes(s, p, guide_n, SurfaceGuide{guide_p, p.phi_geo}, a, b, dilate ? nullptr : out);
    float4 *spare = src == a ? b : a;                             // src: the masked plane; spare: free
    for (uint32_t k = 0; k < dilate; k++) {
        float4 *const to = k + 1u == dilate ? out : spare;
        pt_launch_bake_dilate_pass(s, p.W, p.H, src, to);
        spare = src; src = to;
    }
}

}  // namespace

extern "C" {

int ptmi_bake_denoise(ptmi_ctx *c, const ptmi_bake_denoise_params *p, float *dst_rgba, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    const ptmi_bake_denoise_params zero = {};
    const ptmi_bake_denoise_params &q = p ? *p : zero;
    AtrousArgs a;
    int rc = atrous_params(c, q.iterations, q.reserved, " of ptmi_bake_denoise_params", q.phi_color, q.phi_normal, q.phi_position, &a);
    if (rc) return rc;
    if (!c->d_bake_texels) return fail(c, PTMI_E_INVALID, "no bake surface in place (ptmi_upload_bake_surface)");
    const size_t npix = (size_t)c->W * c->H;
    if (dst_rgba && n_floats != npix * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", npix * 4, n_floats);
    if (!c->moments_on || !c->plane[kMoments]) return fail(c, PTMI_E_STATE, "the bake denoiser needs the moments plane (ptmi_set_moments)");
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = make_planes(c, group_set(kByBake) | group_set(kByBakeDenoise), npix, c->plane))) return rc;
    // a pass fills the texels one step (in the maximum norm) further from the covered ones, and none is farther than the longer side
    const uint32_t dilate = std::min(q.dilate, std::max(c->W, c->H));
    launch(c->stream, a, dilate, c->d_bake_texels, c->d_out, plane_as<float4>(c, kMoments), plane_as<float4>(c, kBdGuideN),
           plane_as<float4>(c, kBdGuideP), plane_as<float4>(c, kBakeA), plane_as<float4>(c, kBakeB), plane_as<float4>(c, kBdOut));
    HIP_TRY(c, hipGetLastError());
    return dst_rgba ? read_plane(c, kBdOut, c->plane[kBdOut], dst_rgba, n_floats, 4) : PTMI_OK;
}

void *ptmi_bake_denoised_device_ptr(ptmi_ctx *c) { return c ? c->plane[kBdOut] : nullptr; }

}  // extern "C"
