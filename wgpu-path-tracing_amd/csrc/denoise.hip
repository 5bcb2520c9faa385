// denoise.hip — ptmi_denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) whose colour weight is scaled by the
// per-pixel variance of the running mean (Schied et al. 2017, SVGF, the spatial part only). It reads the output buffer, the NORMAL
// (and ALBEDO) first-hit planes and the sample-moments plane, and writes a context-owned plane; none of its inputs are written.
//
//   prepass   guide = (unit normal or 0 on a miss, depth), grad = max |depth - depth of a 4-neighbour| (neighbours inside the image),
//             cv = (colour, variance of the mean): variance = max(0, E[l^2] - E[l]^2) / max(frames, 1); with demodulation and
//             coverage > 0: colour / max(albedo, 1e-3) per channel, variance / max(l(albedo), 1e-3)^2
//   pass i    5x5 B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16) at offsets of 2^i pixels; w = h h w_n w_z w_l with
//             w_n = max(0, n_p . n_q)^phi_n, w_z = exp(-|z_p - z_q| / (phi_z |offset| grad_p + 1e-6)),
//             w_l = exp(-|l_p - l_q| / (phi_c sqrt(g3x3(var)_p) + 1e-6)); colour = sum w c / sum w, var = sum w^2 var / (sum w)^2.
//             Taps outside the image, with a non-finite value or a zero guide normal are skipped; the centre weighs h0^2. A centre
//             that is non-finite or has a zero normal (a miss) keeps its value. g3x3 is the (1/4, 1/8, 1/16) Gaussian over the
//             finite taps inside the image, divided by the sum of their weights.
//   last pass remodulates with the same clamped albedo and writes (rgb, 0).
// Every expression is written in the order tests/denoise_ref.py restates it; the library builds with -ffp-contract=off, so the only
// differences to a float32 numpy restatement are exp and pow (a few ulp).
// The pass itself is pt_atrous.h's, shared with bake_denoise.hip; what is the camera's own is the prepass and DepthGuide below: w_z,
// a miss written through, and the remodulation.
#include "pt_atrous.h"

namespace {

using namespace pt_atrous;

__global__ __launch_bounds__(DX * DY) void k_dn_prepass(uint32_t W, uint32_t H, const float4 *__restrict__ radiance,
                                                        const float4 *__restrict__ normal, const float4 *__restrict__ albedo,
                                                        const float4 *__restrict__ moments, float4 *__restrict__ guide,
                                                        float *__restrict__ grad, float4 *__restrict__ cv) {
    const uint32_t x = blockIdx.x * DX + threadIdx.x, y = blockIdx.y * DY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 n = normal[i];
    const float len2 = n.x * n.x + n.y * n.y + n.z * n.z;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, n.w);
    if (len2 > 0.0f) {
        const float len = __builtin_sqrtf(len2);
        g.x = n.x / len; g.y = n.y / len; g.z = n.z / len;
    }
    float dz = 0.0f;
    if (x > 0u) dz = max1(dz, __builtin_fabsf(n.w - normal[i - 1].w));
    if (x + 1u < W) dz = max1(dz, __builtin_fabsf(n.w - normal[i + 1].w));
    if (y > 0u) dz = max1(dz, __builtin_fabsf(n.w - normal[i - W].w));
    if (y + 1u < H) dz = max1(dz, __builtin_fabsf(n.w - normal[i + W].w));
    const float4 c = radiance[i], m = moments[i];
    float4 o = make_float4(c.x, c.y, c.z, max1(0.0f, m.y - m.x * m.x) / max1(m.z, 1.0f));
    if (albedo) {
        const float4 a = albedo[i];
        if (a.w > 0.0f) {
            o.x = o.x / max1(a.x, 1e-3f); o.y = o.y / max1(a.y, 1e-3f); o.z = o.z / max1(a.z, 1e-3f);
            const float la = max1(lum(a.x, a.y, a.z), 1e-3f);
            o.w = o.w / (la * la);
        }
    }
    guide[i] = g;
    grad[i] = dz;
    cv[i] = o;
}

// The guide plane is (unit normal or 0 on a miss, depth). A miss carries a value (the sky, the background), so nothing is masked.
struct DepthGuide {
    const float *grad;
    const float4 *albedo;               // NULL: no demodulation
    float phi_z;
    static constexpr bool kMasked = false;
    struct Centre { float gz; };
    PT_DEV Centre centre(size_t i, float4) const { return {grad[i]}; }
    PT_DEV float weight(Centre at, float4 gp, float4 gq, size_t, float off) const {
        return __builtin_expf(-__builtin_fabsf(gp.w - gq.w) / (phi_z * off * at.gz + 1e-6f));
    }
    // remodulates and writes (rgb, 0)
    PT_DEV void finish(size_t i, float4 &o) const {
        if (albedo) {
            const float4 a = albedo[i];
            if (a.w > 0.0f) { o.x = o.x * max1(a.x, 1e-3f); o.y = o.y * max1(a.y, 1e-3f); o.z = o.z * max1(a.z, 1e-3f); }
        }
        o.w = 0.0f;
    }
};

}  // namespace

void pt_launch_denoise(hipStream_t s, const AtrousArgs &a, const float4 *radiance, const float4 *normal, const float4 *albedo,
                       const float4 *moments, float4 *guide, float *grad, float4 *cv, float4 *tmp, float4 *out) {
    hipLaunchKernelGGL(k_dn_prepass, grid(a.W, a.H), block(), 0, s, a.W, a.H, radiance, normal, albedo, moments, guide, grad, cv);
    launch_passes(s, a, guide, DepthGuide{grad, albedo, a.phi_geo}, cv, tmp, out);
}
