// pt_texel.h — the texel fetch of the atlas (pt.wgsl:112-120), shared by the kernels that read it: `shade` (shade.hip) for the four maps
// of a hit, the alpha-cutout resolve kernels (alpha.hip) for the albedo map's alpha.
#pragma once
#include "pt_device.h"
#include "pt_math.h"

namespace {

PT_DEV v4 atlas_load(const DevScene &sc, uint32_t x, uint32_t y) {
    v4 r; r.x = r.y = r.z = r.w = 0.0f;
    if (sc.atlas_fmt == 0u || x >= sc.atlas_w || y >= sc.atlas_h) return r;      // out of bounds reads zero
    size_t idx = ((size_t)y * sc.atlas_w + x);
    if (sc.atlas_fmt == 1u) {
        const uint2 raw = reinterpret_cast<const uint2 *>(sc.atlas)[idx];        // 4 x f16
        union { uint32_t u; _Float16 h[2]; } a, b;
        a.u = raw.x; b.u = raw.y;
        r.x = (float)a.h[0]; r.y = (float)a.h[1]; r.z = (float)b.h[0]; r.w = (float)b.h[1];
    } else {
        const float4 t = reinterpret_cast<const float4 *>(sc.atlas)[idx];
        r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
    }
    return r;
}

// getTextureColor, pt.wgsl:112-120
PT_DEV v4 texture_color(const DevScene &sc, const ptmi_atlas_rect &tx, float uvx, float uvy, v4 fallback) {
    if (tx.w == 0u || tx.h == 0u) return fallback;
    float fx = uvx - __builtin_truncf(uvx);             // uv % 1.0 (exact)
    float fy = uvy - __builtin_truncf(uvy);
    float ax = (float)tx.x + fx * (float)tx.w;
    float ay = (float)tx.y + fy * (float)tx.h;
    return atlas_load(sc, f2u(ax), f2u(ay));
}

}  // namespace
