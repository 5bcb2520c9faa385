// pt_env.h — the environment map on the device: lookup, density and sampling (include/ptmi.h ptmi_upload_environment).
// Included by shade.hip (both builds) and by environment.hip, whose debug kernels call the same functions the renders run.
//
// The map is equirectangular, row 0 at the +Y pole. One float4 (r, g, b, c) per texel: the radiance and c = P_t N / (2 pi^2), the
// texel's selection probability turned into a density over (u, v), so that the solid-angle density of a direction in texel t is
// c / sin(theta). The alias table holds (bits(prob), alias) per entry. Both are plain global buffers (a 2048 x 1024 map is 50 MB).
//
// Arithmetic: the lookup uses the device's atan2f / acosf, so which texel a direction within rounding of a texel border reads is
// outside the arithmetic contract (like blit). Everything else is float32 in the order written, sin / cos are the contract's sincos1.
#pragma once
#include "pt_device.h"
#include "pt_math.h"

#define PT_TWO_PI 6.28318530718f

struct EnvSample { v3 le; float pdf; };     // radiance (texel x intensity) and solid-angle density

// the texel a unit direction reads
PT_DEV uint32_t env_texel(const DevEnv &e, v3 d) {
    const float phi = atan2f(d.z, d.x) - e.rotation;
    float u = phi / PT_TWO_PI + 0.5f;
    u -= __builtin_floorf(u);                                   // wrapped into [0, 1] (1 only by rounding: clamped below)
    const float v = acosf(min1(max1(d.y, -1.0f), 1.0f)) / PT_PI;
    const uint32_t x = min(f2u(u * (float)e.w), e.w - 1u), y = min(f2u(v * (float)e.h), e.h - 1u);
    return y * e.w + x;
}
PT_DEV v3 env_radiance(const DevEnv &e, float4 t) { return mk3(t.x * e.intensity, t.y * e.intensity, t.z * e.intensity); }
// c / max(sin(theta), eps) from the direction's y: 1 - y^2 in one rounding (near the poles the product's own rounding would be
// a 1e-5 of the difference)
PT_DEV float env_pdf_of(float c, float dy) { return c / max1(sqrt1(max1(0.0f, fma1(-dy, dy, 1.0f))), PT_EPS); }
PT_DEV EnvSample env_lookup(const DevEnv &e, v3 d) {
    const float4 t = e.tab[env_texel(e, d)];
    return EnvSample{env_radiance(e, t), env_pdf_of(t.w, d.y)};
}
// the environment chosen as the light, from four uniforms in [0, 1]: the alias pick, then a uniform point of the texel
PT_DEV EnvSample env_sample(const DevEnv &e, float r1, float r2, float r3, float r4, v3 &d, uint32_t &texel) {
    const uint32_t n = e.w * e.h;
    const uint32_t k = min(f2u(r1 * (float)n), n - 1u);
    const uint2 a = e.alias[k];
    const uint32_t t = r2 < __uint_as_float(a.x) ? k : a.y;
    const uint32_t ty = t / e.w, tx = t - ty * e.w;
    const float u = ((float)tx + r3) / (float)e.w, v = ((float)ty + r4) / (float)e.h;
    const float theta = v * PT_PI, phi = fma1(u - 0.5f, PT_TWO_PI, e.rotation);
    float st, ct, sp, cp;
    sincos1(theta, st, ct);
    sincos1(phi, sp, cp);
    d = mk3(st * cp, ct, st * sp);
    texel = t;
    const float4 q = e.tab[t];
    return EnvSample{env_radiance(e, q), q.w / max1(st, PT_EPS)};
}
