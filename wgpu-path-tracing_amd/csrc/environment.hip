// environment.hip — the environment map of include/ptmi.h (ptmi_upload_environment): the tables built on the host at upload, their
// installation and removal, and the kernels behind the two device debug calls, which run the pt_env.h functions k_shade runs.
#include "ptmi_ctx.h"
#include "pt_env.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr double kPi = 3.14159265358979323846;

struct EnvTables {
    std::vector<float4> tab;            // (r, g, b, c) per texel
    std::vector<uint2> alias;           // (bits(prob), alias) per entry
    double weight_sum = 0.0;
};

// params resolved: intensity 0 -> 1, the rotation as its remainder by 2 pi (the same azimuths; keeps the kernels' sin / cos in range)
int resolve_params(const ptmi_environment *p, ptmi_environment &out, std::string &err) {
    const ptmi_environment zero = {};
    out = p ? *p : zero;
    if (!std::isfinite(out.intensity) || out.intensity < 0.0f) return fail(err, PTMI_E_INVALID, "intensity %g is negative or not finite", (double)out.intensity);
    if (!std::isfinite(out.rotation)) return fail(err, PTMI_E_INVALID, "rotation is not finite");
    if (out.sample > 1u) return fail(err, PTMI_E_INVALID, "unknown sample %u", out.sample);
    for (uint32_t r : out.reserved) if (r) return fail(err, PTMI_E_INVALID, "a reserved word of ptmi_environment is not zero");
    if (out.intensity == 0.0f) out.intensity = 1.0f;
    if (std::fabs(out.rotation) > (float)kPi) out.rotation = (float)std::remainder((double)out.rotation, 2.0 * kPi);
    return PTMI_OK;
}

// The tables of a map: validation, the weights w_t = lum(rgb_t) (cos theta_top - cos theta_bottom), Vose's alias method over
// p_t = P_t N, and c_t = P_t N / (2 pi^2); all in double, rounded to float once.
int build_tables(const void *texels, uint32_t w, uint32_t h, int fmt, EnvTables &t, std::string &err) {
    size_t bytes = 0;
    char why[128];
    if (!texels || w == 0 || h == 0) return fail(err, PTMI_E_INVALID, "no texels");
    if (pt_atlas_bytes(w, h, fmt, &bytes, why, sizeof why) != PTMI_OK) return fail(err, PTMI_E_INVALID, "%s", why);
    if ((uint64_t)w * h > (1ull << 28)) return fail(err, PTMI_E_INVALID, "environment of %ux%u texels is above 2^28 texels", w, h);
    const size_t n = (size_t)w * h;
    t.tab.resize(n);
    t.alias.resize(n);
    std::vector<double> p(n);
    double sum = 0.0;
    for (uint32_t y = 0; y < h; y++) {
        const double band = std::cos(kPi * y / h) - std::cos(kPi * (y + 1) / h);
        for (uint32_t x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            float rgb[3];
            for (int k = 0; k < 3; k++)
                rgb[k] = fmt == PTMI_ATLAS_RGBA16F ? (float)static_cast<const _Float16 *>(texels)[4 * i + k]
                                                   : static_cast<const float *>(texels)[4 * i + k];
            for (float f : rgb)
                if (!std::isfinite(f) || f < 0.0f)
                    return fail(err, PTMI_E_INVALID, "texel (%u, %u) of the environment is negative or not finite", x, y);
            t.tab[i] = make_float4(rgb[0], rgb[1], rgb[2], 0.0f);
            p[i] = (0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2]) * band;
            sum += p[i];
        }
    }
    t.weight_sum = sum;
    union { float f; uint32_t u; } one, bits;
    one.f = 1.0f;
    for (size_t i = 0; i < n; i++) t.alias[i] = make_uint2(sum > 0.0 ? one.u : 0u, (uint32_t)i);
    if (!(sum > 0.0)) return PTMI_OK;                         // all black: looked up, never sampled
    for (size_t i = 0; i < n; i++) {
        p[i] = p[i] / sum * (double)n;
        t.tab[i].w = (float)(p[i] / (2.0 * kPi * kPi));
    }
    // Vose. The entries of probability zero are paired first, while a donor is certain to exist (the others then hold more than one
    // each on average), so that none of them is left over and given probability 1 by the rounding of the running differences.
    std::vector<uint32_t> zero, small, large;
    for (size_t i = n; i-- > 0;) (p[i] == 0.0 ? zero : p[i] < 1.0 ? small : large).push_back((uint32_t)i);
    auto pair_off = [&](std::vector<uint32_t> &from) {
        while (!from.empty() && !large.empty()) {
            const uint32_t s = from.back(), l = large.back();
            from.pop_back();
            bits.f = (float)p[s];
            t.alias[s] = make_uint2(bits.u, l);
            p[l] = (p[l] + p[s]) - 1.0;
            if (p[l] < 1.0) { large.pop_back(); small.push_back(l); }
        }
    };
    pair_off(zero);
    for (uint32_t s : zero) t.alias[s] = make_uint2(0u, large.empty() ? small.back() : large.back());   // (no donor left: cannot happen)
    pair_off(small);                                          // what is left on either list holds 1 within rounding: prob 1, own alias
    return PTMI_OK;
}

__global__ void k_env_lookup(uint32_t n, DevEnv e, const float *__restrict__ d3, float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const EnvSample s = env_lookup(e, mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]));
    out[i] = make_float4(s.le.x, s.le.y, s.le.z, s.pdf);
}
__global__ void k_env_sample(uint32_t n, DevEnv e, const float4 *__restrict__ r, float *__restrict__ d3, float4 *__restrict__ out,
                             uint32_t *__restrict__ texel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 q = r[i];
    v3 d; uint32_t t;
    const EnvSample s = env_sample(e, q.x, q.y, q.z, q.w, d, t);
    d3[3 * i] = d.x; d3[3 * i + 1] = d.y; d3[3 * i + 2] = d.z;
    out[i] = make_float4(s.le.x, s.le.y, s.le.z, s.pdf);
    texel[i] = t;
}

// the context's DevScene after a change of its environment, on the host and in device memory
int publish(ptmi_ctx *c) {
    c->sc.env.sampled = c->sc.env.tab && c->env_weight_sum > 0.0 && !c->env_lookup_only ? 1u : 0u;
    HIP_TRY(c, hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice));
    return PTMI_OK;
}

}  // namespace

extern "C" {

// Everything is checked, built and on the device before the old map goes: a failed call leaves the context's environment, its
// DevScene and the device copy of that as they were.
int ptmi_upload_environment(ptmi_ctx *c, const void *texels, uint32_t w, uint32_t h, int fmt, const ptmi_environment *params) {
    if (!c) return PTMI_E_INVALID;
    const bool remove = !texels || w == 0 || h == 0;
    EnvTables t;
    ptmi_environment prm{};
    int rc;
    if (!remove && ((rc = resolve_params(params, prm, c->err)) || (rc = build_tables(texels, w, h, fmt, t, c->err)))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    float4 *tab = nullptr;
    uint2 *alias = nullptr;
    if (!remove) {
        hipError_t e = hipMalloc(&tab, t.tab.size() * sizeof(float4));
        if (e == hipSuccess) e = hipMalloc(&alias, t.alias.size() * sizeof(uint2));
        if (e == hipSuccess) e = hipMemcpy(tab, t.tab.data(), t.tab.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(alias, t.alias.data(), t.alias.size() * sizeof(uint2), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = sync_all(c);             // nothing in flight reads the old map any more
        if (e != hipSuccess) {
            dfree(tab); dfree(alias);
            (void)hipGetLastError();
            return fail(c, PTMI_E_HIP, "environment upload failed: %s (the previous environment, if any, is still in place)", hipGetErrorString(e));
        }
    } else HIP_TRY(c, sync_all(c));
    dfree(c->d_env); dfree(c->d_env_alias);
    c->d_env = tab; c->d_env_alias = alias;
    c->env_weight_sum = remove ? 0.0 : t.weight_sum;
    c->env_lookup_only = !remove && prm.sample == 1u;
    c->sc.env = DevEnv{tab, alias, remove ? 0u : w, remove ? 0u : h, 0u, remove ? 0.0f : prm.intensity, remove ? 0.0f : prm.rotation};
    return publish(c);
}

int ptmi_set_environment(ptmi_ctx *c, const ptmi_environment *params) {
    if (!c) return PTMI_E_INVALID;
    if (!c->sc.env.tab) return fail(c, PTMI_E_STATE, "no environment uploaded (ptmi_upload_environment)");
    ptmi_environment prm{};
    const int rc = resolve_params(params, prm, c->err);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    c->env_lookup_only = prm.sample == 1u;
    c->sc.env.intensity = prm.intensity; c->sc.env.rotation = prm.rotation;
    return publish(c);
}

int ptmi_environment_status(ptmi_ctx *c, struct ptmi_environment_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    out->width = c->sc.env.w; out->height = c->sc.env.h; out->sampled = c->sc.env.sampled;
    out->weight_sum = c->env_weight_sum;
    return PTMI_OK;
}

int ptmi_debug_env_table(const void *texels, uint32_t w, uint32_t h, int fmt, float *c_out, float *prob_out, uint32_t *alias_out,
                         double *weight_sum) {
    EnvTables t;
    const int rc = build_tables(texels, w, h, fmt, t, g_create_err);
    if (rc) return rc;
    for (size_t i = 0; i < t.tab.size(); i++) {
        if (c_out) c_out[i] = t.tab[i].w;
        if (prob_out) std::memcpy(&prob_out[i], &t.alias[i].x, 4);
        if (alias_out) alias_out[i] = t.alias[i].y;
    }
    if (weight_sum) *weight_sum = t.weight_sum;
    return PTMI_OK;
}

int ptmi_debug_env_lookup(ptmi_ctx *c, uint32_t n, const float *d3, float *out4) {
    if (!c || !d3 || !out4) return PTMI_E_INVALID;
    if (!c->sc.env.tab) return fail(c, PTMI_E_STATE, "no environment uploaded (ptmi_upload_environment)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> dd; Scratch<float4> dout;
    HIP_TRY(c, hipMalloc(&dd.p, (size_t)n * 12)); HIP_TRY(c, hipMalloc(&dout.p, (size_t)n * 16));
    HIP_TRY(c, hipMemcpy(dd.p, d3, (size_t)n * 12, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_env_lookup, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.env, dd.p, dout.p);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out4, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int ptmi_debug_env_sample(ptmi_ctx *c, uint32_t n, const float *r4, float *d3, float *out4, uint32_t *texel) {
    if (!c || !r4) return PTMI_E_INVALID;
    if (!c->sc.env.tab) return fail(c, PTMI_E_STATE, "no environment uploaded (ptmi_upload_environment)");
    if (!c->sc.env.sampled) return fail(c, PTMI_E_STATE, "the environment is not sampled (all black, or sample = 1)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float4> dr, dout; Scratch<float> dd; Scratch<uint32_t> dt;
    HIP_TRY(c, hipMalloc(&dr.p, (size_t)n * 16)); HIP_TRY(c, hipMalloc(&dout.p, (size_t)n * 16));
    HIP_TRY(c, hipMalloc(&dd.p, (size_t)n * 12)); HIP_TRY(c, hipMalloc(&dt.p, (size_t)n * 4));
    HIP_TRY(c, hipMemcpy(dr.p, r4, (size_t)n * 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_env_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.env, dr.p, dd.p, dout.p, dt.p);
    HIP_TRY(c, sync_all(c));
    if (d3) HIP_TRY(c, hipMemcpy(d3, dd.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (out4) HIP_TRY(c, hipMemcpy(out4, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (texel) HIP_TRY(c, hipMemcpy(texel, dt.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
