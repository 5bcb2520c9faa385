// debug_stages.hip — the per-stage entry points of include/ptmi.h (ptmi_debug_*): one stage of the pipeline on the caller's rays, for
// the parity tests. (Those of the traversal image are with the image, scene_image.hip.) debug_listed_rays is the first rays of listed
// pixels from any ray source: ptmi_debug_raygen here, ptmi_debug_bake_rays (bake.hip) and ptmi_debug_probe_rays (probes.hip) are
// their own checks and one call of it.
#include "ptmi_ctx.h"

#include <cstring>
#include <vector>

namespace {

int upload_rays(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *w, float4 *dO, float4 *dD) {
    std::vector<float4> o(n), d(n);
    for (uint32_t i = 0; i < n; i++) {
        o[i] = make_float4(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2], w ? w[i] : 0.0f);
        d[i] = make_float4(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2], 0.0f);
    }
    HIP_TRY(c, hipMemcpyAsync(dO, o.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dD, d.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, sync_all(c));
    return PTMI_OK;
}

// The per-stage entry points run on the context's stream, in the batch arrays of a dispatch: nothing in flight, and room for n paths.
int stage_begin(ptmi_ctx *c, size_t n) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    return ensure_capacity(c, c->lane, n);
}

// origins and directions as the caller's packed triples; rng: the word beside each origin
void unpack3(const std::vector<float4> &o, const std::vector<float4> &d, float *o3, float *d3, uint32_t *rng = nullptr) {
    for (size_t i = 0; i < o.size(); i++) {
        o3[3 * i] = o[i].x; o3[3 * i + 1] = o[i].y; o3[3 * i + 2] = o[i].z;
        d3[3 * i] = d[i].x; d3[3 * i + 1] = d[i].y; d3[3 * i + 2] = d[i].z;
        if (rng) std::memcpy(&rng[i], &o[i].w, 4);
    }
}

}  // namespace

PT_HOST {

int debug_listed_rays(ptmi_ctx *c, const DevRays &rays, uint32_t width, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                      const uint32_t *frames, float *o3, float *d3, uint32_t *rng) {
    if (n == 0) return PTMI_OK;
    const int rc = stage_begin(c, n);
    if (rc) return rc;
    Lane &ln = c->lane;
    uint32_t *dx = ln.queue[0], *dy = ln.queue[1], *df = reinterpret_cast<uint32_t *>(ln.hits);
    HIP_TRY(c, hipMemcpyAsync(dx, xs, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dy, ys, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(df, frames, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    pt_launch_raygen_list(c->stream, rays, width, n, dx, dy, df, ln.paths);
    std::vector<float4> o(n), d(n);
    HIP_TRY(c, hipMemcpyAsync(o.data(), ln.paths.O, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.data(), ln.paths.D, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    unpack3(o, d, o3, d3, rng);
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

// ---- per-stage entry points ------------------------------------------------------
int ptmi_debug_raygen(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                      const uint32_t *frames, float *o3, float *d3, uint32_t *rng) {
    if (!c || !cam || !xs || !ys || !frames || !o3 || !d3) return PTMI_E_INVALID;
    uint32_t proj;
    int rc = pt_check_camera(c, cam, &proj, c->err);
    if (rc) return rc;
    return debug_listed_rays(c, CameraSource{cam, proj}, cam->width, n, xs, ys, frames, o3, d3, rng);
}

int ptmi_debug_center_rays(ptmi_ctx *c, const ptmi_camera *cam, float *o3, float *d3, size_t n_floats_each) {
    if (!c) return PTMI_E_INVALID;
    if (!cam || !o3 || !d3) return fail(c, PTMI_E_INVALID, "NULL argument");
    if (c->W == 0 || c->H == 0) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (cam->width != c->W || cam->height != c->H)
        return fail(c, PTMI_E_INVALID, "camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
    const size_t n = (size_t)c->W * c->H;
    if (n_floats_each != n * 3) return fail(c, PTMI_E_INVALID, "expected %zu floats each, got %zu", n * 3, n_floats_each);
    uint32_t proj;
    int rc = pt_check_camera(c, cam, &proj, c->err);
    if (rc) return rc;
    if ((rc = stage_begin(c, n))) return rc;
    Lane &ln = c->lane;
    const DevBand whole{c->W, c->H, 0u, c->H, 1u, 1u, 0u, c->H};
    pt_launch_center_rays(c->stream, c->n_cu * 8, *cam, proj, whole, ln.paths, &c->d_control[kCwQueue]);
    std::vector<float4> o(n), d(n);
    HIP_TRY(c, hipMemcpyAsync(o.data(), ln.paths.O, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.data(), ln.paths.D, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    unpack3(o, d, o3, d3);
    return PTMI_OK;
}

int ptmi_debug_intersect(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, float *t, uint32_t *tri,
                         float *u, float *v) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!o3 || !d3 || !t || !tri || !u || !v) return fail(c, PTMI_E_INVALID, "NULL argument");
    if (n == 0) return PTMI_OK;
    if ((rc = stage_begin(c, n))) return rc;
    Lane &ln = c->lane;
    rc = upload_rays(c, n, o3, d3, nullptr, ln.paths.O, ln.paths.D);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(&c->d_control[kCwQueue], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg;
    if ((rc = traverse_ready(c, true, cfg))) return rc;
    launch_extend(c, c->stream, cfg, ln.paths, nullptr, &c->d_control[kCwQueue], ln.hits);
    // (u, v) are not part of the hit record: rebuilt exactly as `shade` rebuilds them (into the C stream, unused here)
    pt_launch_hit_uv(c->stream, n, c->sc, ln.paths, ln.hits, ln.paths.C);
    std::vector<float2> h(n), uv(n);
    HIP_TRY(c, hipMemcpyAsync(h.data(), ln.hits, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(uv.data(), ln.paths.C, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipGetLastError());
    for (uint32_t i = 0; i < n; i++) {
        t[i] = h[i].x; u[i] = uv[i].x; v[i] = uv[i].y; std::memcpy(&tri[i], &h[i].y, 4);
    }
    return PTMI_OK;
}

int ptmi_debug_occluded(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *dist, uint8_t *occ) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!o3 || !d3 || !dist || !occ) return fail(c, PTMI_E_INVALID, "NULL argument");
    if (n == 0) return PTMI_OK;
    if ((rc = stage_begin(c, n))) return rc;
    Lane &ln = c->lane;
    {   // every negative distance means "directional light" (ptmi.h). Inside the library -2 is the record of an emissive hit
        // (nothing to trace, traverse.hip ShadowIO::fetch): a caller's -2 must not be read as that, so negatives travel as -1
        std::vector<float> dn(dist, dist + n);
        for (float &x : dn) if (x < 0.0f) x = -1.0f;
        rc = upload_rays(c, n, o3, d3, dn.data(), ln.sh[0].SO, ln.sh[0].SD);
    }
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(&c->d_control[kCwQueue], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg;
    if ((rc = traverse_ready(c, false, cfg))) return rc;
    launch_shadow(c, c->stream, cfg, ln.paths, ln.sh[0], nullptr, &c->d_control[kCwQueue], ln.d_occ);
    HIP_TRY(c, hipMemcpyAsync(occ, ln.d_occ, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int ptmi_debug_math(ptmi_ctx *c, int op, uint32_t n, const float *a, const float *b, const float *cc, float *out) {
    if (!c || !a || !out) return PTMI_E_INVALID;
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> da, db, dc, dout;
    size_t bytes = (size_t)n * 4;
    HIP_TRY(c, hipMalloc(&da.p, bytes)); HIP_TRY(c, hipMalloc(&dout.p, bytes));
    HIP_TRY(c, hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
    if (b) { HIP_TRY(c, hipMalloc(&db.p, bytes)); HIP_TRY(c, hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice)); }
    if (cc) { HIP_TRY(c, hipMalloc(&dc.p, bytes)); HIP_TRY(c, hipMemcpy(dc.p, cc, bytes, hipMemcpyHostToDevice)); }
    pt_launch_math(c->stream, op, n, da.p, db.p, dc.p, dout.p);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int ptmi_debug_exact_math(ptmi_ctx *c, int which, uint64_t *n_different, uint32_t *first_different) {
    if (!c || !n_different || which < 0 || which > 2) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<unsigned long long> d;
    unsigned long long h[2] = {0ull, ~0ull};
    HIP_TRY(c, hipMalloc(&d.p, sizeof h));
    HIP_TRY(c, hipMemcpy(d.p, h, sizeof h, hipMemcpyHostToDevice));
    pt_launch_exact_math(c->stream, which, d.p);
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(h, d.p, sizeof h, hipMemcpyDeviceToHost));
    *n_different = h[0];
    if (first_different) *first_different = (uint32_t)h[1];
    return PTMI_OK;
}

}  // extern "C"
