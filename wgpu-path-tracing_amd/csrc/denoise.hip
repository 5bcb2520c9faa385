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
#include "pt_device.h"
#include "pt_math.h"

namespace {

constexpr int DX = 64, DY = 4;          // a wave is one 64-pixel row segment: every tap row is one coalesced 1 KiB load

PT_DEV float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV bool finite4(float4 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && __builtin_isfinite(v.w);
}

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

// LAST: the final pass, which remodulates (albedo non-NULL) and writes (rgb, 0); the others write (rgb, variance)
template <bool LAST>
__global__ __launch_bounds__(DX * DY) void k_dn_pass(uint32_t W, uint32_t H, uint32_t step, float phi_c, float phi_n, float phi_z,
                                                     const float4 *__restrict__ guide, const float *__restrict__ grad,
                                                     const float4 *__restrict__ src, const float4 *__restrict__ albedo,
                                                     float4 *__restrict__ dst) {
    const uint32_t x = blockIdx.x * DX + threadIdx.x, y = blockIdx.y * DY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    const float4 cp = src[i];
    const float4 gp = guide[i];
    float4 o = cp;
    if (finite4(cp) && (gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f)) {
        // g3x3(var): the centre is finite, so the weight sum is at least 1/4
        float sv = 0.0f, sk = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = (int)y + dy;
            if (qy < 0 || qy >= (int)H) continue;
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = (int)x + dx;
                if (qx < 0 || qx >= (int)W) continue;
                const float4 q = src[(size_t)qy * W + qx];
                if (!finite4(q)) continue;
                const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                sv = sv + k * q.w;
                sk = sk + k;
            }
        }
        const float lp = lum(cp.x, cp.y, cp.z);
        const float den_l = phi_c * __builtin_sqrtf(sv / sk) + 1e-6f;
        const float gz = grad[i];
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
                const float4 q = src[qi];
                const float4 gq = guide[qi];
                if (!finite4(q) || (gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f)) continue;
                const float wn = __builtin_powf(max1(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z), phi_n);
                const float off = (float)step * __builtin_sqrtf((float)(dx * dx + dy * dy));
                const float wz = __builtin_expf(-__builtin_fabsf(gp.w - gq.w) / (phi_z * off * gz + 1e-6f));
                const float wl = __builtin_expf(-__builtin_fabsf(lp - lum(q.x, q.y, q.z)) / den_l);
                const float w = h[dy + 2] * h[dx + 2] * wn * wz * wl;
                sw = sw + w;
                sr = sr + w * q.x; sg = sg + w * q.y; sb = sb + w * q.z;
                s2 = s2 + w * w * q.w;
            }
        }
        o = make_float4(sr / sw, sg / sw, sb / sw, s2 / (sw * sw));
    }
    if (LAST) {
        if (albedo) {
            const float4 a = albedo[i];
            if (a.w > 0.0f) { o.x = o.x * max1(a.x, 1e-3f); o.y = o.y * max1(a.y, 1e-3f); o.z = o.z * max1(a.z, 1e-3f); }
        }
        o.w = 0.0f;
    }
    dst[i] = o;
}

}  // namespace

void pt_launch_denoise(hipStream_t s, const DenoiseArgs &a, const float4 *radiance, const float4 *normal, const float4 *albedo,
                       const float4 *moments, float4 *guide, float *grad, float4 *cv, float4 *tmp, float4 *out) {
    const dim3 grid((a.W + DX - 1) / DX, (a.H + DY - 1) / DY), block(DX, DY);
    hipLaunchKernelGGL(k_dn_prepass, grid, block, 0, s, a.W, a.H, radiance, normal, albedo, moments, guide, grad, cv);
    const float4 *src = cv;
    float4 *spare = tmp;
    for (uint32_t it = 0; it < a.iterations; it++) {
        const uint32_t step = 1u << it;
        if (it + 1u == a.iterations) {
            hipLaunchKernelGGL(k_dn_pass<true>, grid, block, 0, s, a.W, a.H, step, a.phi_color, a.phi_normal, a.phi_depth, guide, grad,
                               src, albedo, out);
        } else {
            hipLaunchKernelGGL(k_dn_pass<false>, grid, block, 0, s, a.W, a.H, step, a.phi_color, a.phi_normal, a.phi_depth, guide,
                               grad, src, nullptr, spare);
            float4 *const read_next = spare;
            spare = const_cast<float4 *>(src);
            src = read_next;
        }
    }
}
