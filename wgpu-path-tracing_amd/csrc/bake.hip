// bake.hip — lightmap baking (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake): the surface's records and
// the list of its covered texels, the checks of a bake, the gutter fill and the debug rays' checks (the rays themselves:
// debug_stages.hip's listed-rays routine). The bake's ray generation and folds are with the other pixel sources (pipeline.hip
// BakedPixels); its bounce loop is the plain dispatch's (dispatch.hip).
// No counterpart in the reference, which renders from a camera only.
#include "ptmi_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int BLOCK = 256;

// The gutter fill, one thread per texel, no LDS: a texel reads nine entries that its neighbours in the wave read too, which the caches
// serve; the whole plane is 16 B per texel.
// The masked copy: (rgb of the output, 1) for a covered texel, zeros for every other.
__global__ __launch_bounds__(BLOCK) void k_bake_mask(uint32_t n, const float4 *__restrict__ texels, const float4 *__restrict__ out,
                                                     float4 *__restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const bool covered = __float_as_uint(texels[2 * (size_t)i].w) != 0u;
    const float4 o = out[i];
    dst[i] = covered ? make_float4(o.x, o.y, o.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
// One pass (include/ptmi.h ptmi_bake_dilate): src is the state before the pass, and only dst is written.
__global__ __launch_bounds__(BLOCK) void k_bake_dilate(uint32_t W, uint32_t H, const float4 *__restrict__ src, float4 *__restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= W * H) return;
    const float4 own = src[i];
    if (own.w != 0.0f) { dst[i] = own; return; }
    const uint32_t y = i / W, x = i % W;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint32_t count = 0;
    for (int dy = -1; dy <= 1; dy++) {
        const uint32_t ny = y + (uint32_t)dy;                   // y = 0, dy = -1 wraps and fails the test
        if (ny >= H) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const uint32_t nx = x + (uint32_t)dx;
            if (nx >= W || (dx == 0 && dy == 0)) continue;
            const float4 v = src[(size_t)ny * W + nx];
            if (v.w == 0.0f) continue;
            sx += v.x; sy += v.y; sz += v.z; count++;
        }
    }
    const float k = (float)count;
    dst[i] = count ? make_float4(sx / k, sy / k, sz / k, 2.0f) : own;
}

float dot3_f32(const float *a) { return std::fmaf(a[2], a[2], std::fmaf(a[1], a[1], a[0] * a[0])); }     // pt_math.h dot3(a, a)

// *out = the params with their defaults (NULL: first_frame 0, bias PT_EPS), or PTMI_E_INVALID for a bad bias or reserved word
int resolve_params(ptmi_ctx *c, const ptmi_bake_params *params, ptmi_bake_params *out) {
    ptmi_bake_params bp{0u, 1e-6f, {0u, 0u}};
    if (params) bp = *params;
    if (bp._reserved[0] || bp._reserved[1]) return fail(c, PTMI_E_INVALID, "a reserved word of ptmi_bake_params is not zero");
    if (!std::isfinite(bp.bias) || bp.bias < 0.0f) return fail(c, PTMI_E_INVALID, "bias %g is negative or not finite", (double)bp.bias);
    *out = bp;
    return PTMI_OK;
}

}  // namespace

void pt_launch_bake_dilate_pass(hipStream_t s, uint32_t W, uint32_t H, const float4 *src, float4 *dst) {
    hipLaunchKernelGGL(k_bake_dilate, dim3((W * H + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, W, H, src, dst);
}

float4 *pt_launch_bake_dilate(hipStream_t s, uint32_t W, uint32_t H, uint32_t passes, const float4 *texels, const float4 *out,
                              float4 *a, float4 *b) {
    const uint32_t n = W * H;
    hipLaunchKernelGGL(k_bake_mask, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, n, texels, out, a);
    for (uint32_t k = 0; k < passes; k++) {
        pt_launch_bake_dilate_pass(s, W, H, a, b);
        std::swap(a, b);
    }
    return a;
}

PT_HOST {

void bake_forget(ptmi_ctx *c) {
    dfree(c->d_bake_texels); dfree(c->d_bake_covered);
    c->bake_covered = 0;
}

int bake_check(ptmi_ctx *c, const ptmi_bake_params *params, ptmi_bake_params *out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    ptmi_bake_params bp;
    if ((rc = resolve_params(c, params, &bp))) return rc;
    if (!c->d_bake_texels) return fail(c, PTMI_E_INVALID, "no bake surface in place (ptmi_upload_bake_surface)");
    if ((rc = listed_check(c, "a bake"))) return rc;
    *out = bp;
    return PTMI_OK;
}

int listed_check(ptmi_ctx *c, const char *what) {
    if (c->aov_mask) return fail(c, PTMI_E_INVALID, "%s has no first hit: turn the first-hit planes off (ptmi_set_aovs(0))", what);
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    if (band.y0 != 0u || band.y1 != c->H || band.parts > 1u || band.rows != c->H)
        return fail(c, PTMI_E_INVALID, "%s covers the whole frame: the tile options select rows [%u,%u), part %u of %u", what, band.y0,
                    band.y1, band.part, band.parts);
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

// Everything is checked and the new records are on the device before the old surface goes: a failed call leaves it in place.
int ptmi_upload_bake_surface(ptmi_ctx *c, const ptmi_bake_texel *texels, uint32_t w, uint32_t h) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!texels) {
        HIP_TRY(c, sync_all(c));
        bake_forget(c);
        return PTMI_OK;
    }
    if (c->W == 0 || c->H == 0 || w != c->W || h != c->H)
        return fail(c, PTMI_E_INVALID, "the surface is %ux%u but the output buffer is %ux%u", w, h, c->W, c->H);
    const size_t n = (size_t)w * h;
    std::vector<uint32_t> covered;
    for (size_t i = 0; i < n; i++) {
        const ptmi_bake_texel &t = texels[i];
        if (!t.covered) continue;
        for (float v : t.position)
            if (!std::isfinite(v)) return fail(c, PTMI_E_INVALID, "texel (%zu, %zu): the position is not finite", i % w, i / w);
        for (float v : t.normal)
            if (!std::isfinite(v)) return fail(c, PTMI_E_INVALID, "texel (%zu, %zu): the normal is not finite", i % w, i / w);
        const float l2 = dot3_f32(t.normal);
        if (!(l2 > 0.0f) || !std::isfinite(l2))
            return fail(c, PTMI_E_INVALID, "texel (%zu, %zu): the normal's squared length %g is zero or not finite", i % w, i / w, (double)l2);
        covered.push_back((uint32_t)i);
    }
    float4 *d_tex = nullptr;
    uint32_t *d_cov = nullptr;
    hipError_t e = hipMalloc(&d_tex, n * sizeof(ptmi_bake_texel));
    if (e == hipSuccess) e = hipMalloc(&d_cov, std::max<size_t>(covered.size(), 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_tex, texels, n * sizeof(ptmi_bake_texel), hipMemcpyHostToDevice);
    if (e == hipSuccess && !covered.empty()) e = hipMemcpy(d_cov, covered.data(), covered.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sync_all(c);               // nothing in flight reads the old surface any more
    if (e != hipSuccess) {
        dfree(d_tex); dfree(d_cov);
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "bake surface upload failed: %s (the previous surface, if any, is still in place)", hipGetErrorString(e));
    }
    bake_forget(c);
    c->d_bake_texels = d_tex; c->d_bake_covered = d_cov; c->bake_covered = (uint32_t)covered.size();
    return PTMI_OK;
}

int ptmi_bake_status(ptmi_ctx *c, struct ptmi_bake_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    if (!c->d_bake_texels) return PTMI_OK;
    out->present = 1u; out->width = c->W; out->height = c->H; out->covered = c->bake_covered;
    return PTMI_OK;
}

int ptmi_bake_dilate(ptmi_ctx *c, uint32_t passes, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (!c->d_bake_texels) return fail(c, PTMI_E_INVALID, "no bake surface in place (ptmi_upload_bake_surface)");
    const size_t n = (size_t)c->W * c->H;
    if (n_floats != n * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", n * 4, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = make_planes(c, group_set(kByBake), n, c->plane);
    if (rc) return rc;
    // a pass fills the texels one step (in the maximum norm) further from the covered ones, and none is farther than the longer side
    const uint32_t useful = std::min(passes, std::max(c->W, c->H));
    const float4 *res = pt_launch_bake_dilate(c->stream, c->W, c->H, useful, c->d_bake_texels, c->d_out, plane_as<float4>(c, kBakeA),
                                              plane_as<float4>(c, kBakeB));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, hipMemcpy(dst, res, n * 16, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int ptmi_debug_bake_rays(ptmi_ctx *c, const ptmi_bake_params *params, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                         const uint32_t *frames, float *o3, float *d3, uint32_t *rng) {
    if (!c) return PTMI_E_INVALID;
    if (!xs || !ys || !frames || !o3 || !d3) return fail(c, PTMI_E_INVALID, "NULL argument");
    ptmi_bake_params bp;
    int rc = resolve_params(c, params, &bp);
    if (rc) return rc;
    if (!c->d_bake_texels) return fail(c, PTMI_E_INVALID, "no bake surface in place (ptmi_upload_bake_surface)");
    for (uint32_t i = 0; i < n; i++)
        if (xs[i] >= c->W || ys[i] >= c->H) return fail(c, PTMI_E_INVALID, "texel (%u, %u) outside the %ux%u surface", xs[i], ys[i], c->W, c->H);
    return debug_listed_rays(c, BakeSurface{c->d_bake_texels, bp.bias}, c->W, n, xs, ys, frames, o3, d3, rng);
}

}  // extern "C"
