// medium.hip — the participating medium of include/ptmi.h (ptmi_set_medium): the checks of its fields, its installation and removal,
// and the kernels behind the two device debug calls, which run the pt_medium.h functions k_shade runs.
#include "ptmi_ctx.h"
#include "pt_medium.h"

#include <cmath>
#include <cstring>

namespace {

__global__ void k_medium_step(uint32_t n, DevMedium m, const float *__restrict__ o3, const float *__restrict__ d3,
                              const float *__restrict__ t_hit, const float *__restrict__ r3, uint32_t *__restrict__ scattered,
                              float *__restrict__ x3, float *__restrict__ dir3, float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const v3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
    const MedInterval iv = med_interval(m, o, d, t_hit[i]);
    float s = 0.0f, pdf = 0.0f;
    v3 x = mk3(0.0f, 0.0f, 0.0f), dir = x;
    bool sc = false;
    if (iv.b > iv.a) {                                      // the order and the conditions of k_shade's MED block
        s = med_free_flight(m, r3[3 * i]);
        const float t_sc = iv.a + s;
        sc = t_sc < iv.b;
        if (sc) {
            x = madd3(d, t_sc, o);
            float ct;
            dir = med_sample_phase(m.g, d, r3[3 * i + 1], r3[3 * i + 2], ct);
            pdf = med_phase(m.g, ct);
        }
    }
    scattered[i] = sc ? 1u : 0u;
    x3[3 * i] = x.x; x3[3 * i + 1] = x.y; x3[3 * i + 2] = x.z;
    dir3[3 * i] = dir.x; dir3[3 * i + 1] = dir.y; dir3[3 * i + 2] = dir.z;
    out[i] = make_float4(iv.a, iv.b, s, pdf);
}
__global__ void k_medium_tr(uint32_t n, DevMedium m, const float *__restrict__ o3, const float *__restrict__ wi3,
                            const float *__restrict__ dist, float *__restrict__ tr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tr[i] = med_tr(m, mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), mk3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]), dist[i]);
}

}  // namespace

// the checks of ptmi_set_medium, without a context (ptmi_multi_set_medium runs them once before any device changes)
int pt_check_medium(const ptmi_medium *m, std::string &err) {
    if (!m) return PTMI_OK;
    if (!std::isfinite(m->sigma_t) || !(m->sigma_t > 0.0f)) return fail(err, PTMI_E_INVALID, "sigma_t %g is not finite and > 0", (double)m->sigma_t);
    for (float a : m->albedo)
        if (!(a >= 0.0f && a <= 1.0f)) return fail(err, PTMI_E_INVALID, "albedo %g is outside [0, 1]", (double)a);
    if (!(std::fabs(m->g) <= 0.99f)) return fail(err, PTMI_E_INVALID, "g %g is outside [-0.99, 0.99]", (double)m->g);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(m->box_min[k]) || !std::isfinite(m->box_max[k]) || !(m->box_min[k] <= m->box_max[k]))
            return fail(err, PTMI_E_INVALID, "box axis %d: [%g, %g] is not finite with min <= max", k, (double)m->box_min[k], (double)m->box_max[k]);
    for (uint32_t r : m->reserved) if (r) return fail(err, PTMI_E_INVALID, "a reserved word of ptmi_medium is not zero");
    return PTMI_OK;
}
// a density grid needs sigma_t * |box diagonal| <= PT_MED_MAX_DEPTH (pt_medium.h): the bound on its tracking loops
int pt_check_medium_depth(const ptmi_medium *m, std::string &err) {
    double d2 = 0.0;
    for (int k = 0; k < 3; k++) { const double e = (double)m->box_max[k] - (double)m->box_min[k]; d2 += e * e; }
    const double depth = (double)m->sigma_t * std::sqrt(d2);
    if (!(depth <= PT_MED_MAX_DEPTH))
        return fail(err, PTMI_E_UNSUPPORTED, "sigma_t * |box diagonal| = %g exceeds %g, the limit of a medium with a density grid", depth,
                    PT_MED_MAX_DEPTH);
    return PTMI_OK;
}

extern "C" {

// Checked before anything changes: a failed call leaves the medium, the context's DevScene and the device copy of that as they were.
int ptmi_set_medium(ptmi_ctx *c, const ptmi_medium *m) {
    if (!c) return PTMI_E_INVALID;
    int rc = pt_check_medium(m, c->err);
    if (rc) return rc;
    if (m && c->sc.med.grid && (rc = pt_check_medium_depth(m, c->err))) return rc;     // the grid stays, stretched over the new box
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                // nothing in flight reads the device copy any more
    DevMedium d{};
    if (m) {
        d.sigma_t = m->sigma_t; d.g = m->g;
        for (int k = 0; k < 3; k++) { d.albedo[k] = m->albedo[k]; d.box_min[k] = m->box_min[k]; d.box_max[k] = m->box_max[k]; }
        d.on = 1u;
        d.grid = c->sc.med.grid; d.filter = c->sc.med.filter;
        d.nx = c->sc.med.nx; d.ny = c->sc.med.ny; d.nz = c->sc.med.nz;
    }
    DevScene next = c->sc;
    next.med = d;
    HIP_TRY(c, hipMemcpy(c->d_scene, &next, sizeof(DevScene), hipMemcpyHostToDevice));
    c->sc = next;
    if (m) c->medium = *m;
    else {                                                  // the grid goes with its medium
        std::memset(&c->medium, 0, sizeof c->medium);
        dfree(c->d_med_grid);
        c->med_grid = {};
    }
    return PTMI_OK;
}

int ptmi_get_medium(const ptmi_ctx *c, ptmi_medium *out, uint32_t *present) {
    if (!c) return PTMI_E_INVALID;
    if (out) *out = c->medium;
    if (present) *present = c->sc.med.on;
    return PTMI_OK;
}

int ptmi_debug_medium_step(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *t_hit, const float *r3,
                           uint32_t *scattered, float *x3, float *dir3, float *out4) {
    if (!c || !o3 || !d3 || !t_hit || !r3) return PTMI_E_INVALID;
    if (!c->sc.med.on) return fail(c, PTMI_E_STATE, "no medium in place (ptmi_set_medium)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> dorg, ddir, dt, dr, dx, dd; Scratch<uint32_t> ds; Scratch<float4> dout;
    const size_t n3 = (size_t)n * 12;
    HIP_TRY(c, hipMalloc(&dorg.p, n3)); HIP_TRY(c, hipMalloc(&ddir.p, n3)); HIP_TRY(c, hipMalloc(&dr.p, n3));
    HIP_TRY(c, hipMalloc(&dx.p, n3)); HIP_TRY(c, hipMalloc(&dd.p, n3));
    HIP_TRY(c, hipMalloc(&dt.p, (size_t)n * 4)); HIP_TRY(c, hipMalloc(&ds.p, (size_t)n * 4)); HIP_TRY(c, hipMalloc(&dout.p, (size_t)n * 16));
    HIP_TRY(c, hipMemcpy(dorg.p, o3, n3, hipMemcpyHostToDevice)); HIP_TRY(c, hipMemcpy(ddir.p, d3, n3, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dr.p, r3, n3, hipMemcpyHostToDevice)); HIP_TRY(c, hipMemcpy(dt.p, t_hit, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_medium_step, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.med, dorg.p, ddir.p, dt.p, dr.p, ds.p,
                       dx.p, dd.p, dout.p);
    HIP_TRY(c, sync_all(c));
    if (scattered) HIP_TRY(c, hipMemcpy(scattered, ds.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (x3) HIP_TRY(c, hipMemcpy(x3, dx.p, n3, hipMemcpyDeviceToHost));
    if (dir3) HIP_TRY(c, hipMemcpy(dir3, dd.p, n3, hipMemcpyDeviceToHost));
    if (out4) HIP_TRY(c, hipMemcpy(out4, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int ptmi_debug_medium_tr(ptmi_ctx *c, uint32_t n, const float *o3, const float *wi3, const float *dist, float *tr) {
    if (!c || !o3 || !wi3 || !dist) return PTMI_E_INVALID;
    if (!c->sc.med.on) return fail(c, PTMI_E_STATE, "no medium in place (ptmi_set_medium)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> dorg, dwi, ddist, dtr;
    const size_t n3 = (size_t)n * 12;
    HIP_TRY(c, hipMalloc(&dorg.p, n3)); HIP_TRY(c, hipMalloc(&dwi.p, n3));
    HIP_TRY(c, hipMalloc(&ddist.p, (size_t)n * 4)); HIP_TRY(c, hipMalloc(&dtr.p, (size_t)n * 4));
    HIP_TRY(c, hipMemcpy(dorg.p, o3, n3, hipMemcpyHostToDevice)); HIP_TRY(c, hipMemcpy(dwi.p, wi3, n3, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(ddist.p, dist, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_medium_tr, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.med, dorg.p, dwi.p, ddist.p, dtr.p);
    HIP_TRY(c, sync_all(c));
    if (tr) HIP_TRY(c, hipMemcpy(tr, dtr.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
