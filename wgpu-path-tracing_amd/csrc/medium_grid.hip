// medium_grid.hip — the medium's density grid of include/ptmi.h (ptmi_upload_medium_density): the checks of its arguments, its upload and
// removal, its status, and the kernels behind the two device debug calls, which run the pt_medium.h functions k_shade runs.
#include "ptmi_ctx.h"
#include "pt_medium.h"

#include <cmath>

namespace {

__global__ void k_medium_density(uint32_t n, DevMedium m, const float *__restrict__ p3, float *__restrict__ rho) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rho[i] = med_density(m, mk3(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]));
}
__global__ void k_medium_track(uint32_t n, DevMedium m, uint32_t mode, const float *__restrict__ o3, const float *__restrict__ d3,
                               const float *__restrict__ t_end, const uint32_t *__restrict__ rng_in, uint32_t *__restrict__ scattered,
                               float *__restrict__ t_out, float *__restrict__ value, uint32_t *__restrict__ steps_out,
                               uint32_t *__restrict__ rng_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const v3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
    uint32_t rng = rng_in[i], steps = 0u, sc = 0u;
    float t = 0.0f, v = 0.0f;
    if (mode == 0u) {                                       // the order and the conditions of k_shade's MED block
        const MedInterval iv = med_interval(m, o, d, t_end[i]);
        if (iv.b > iv.a) {
            sc = med_delta_track(m, o, d, iv.a, iv.b, rng, t, steps) == PT_TRACK_SCATTERED ? 1u : 0u;
            if (sc) v = med_density(m, madd3(d, t, o));
        }
    } else {
        v = med_ratio_track(m, o, d, t_end[i], rng, steps, t);
    }
    scattered[i] = sc; t_out[i] = t; value[i] = v; steps_out[i] = steps; rng_out[i] = rng;
}

}  // namespace

int pt_check_medium_density(const float *rho, uint32_t nx, uint32_t ny, uint32_t nz, const ptmi_medium_grid *params,
                            struct ptmi_medium_grid_status *st, std::string &err) {
    if (nx > 1024u || ny > 1024u || nz > 1024u) return fail(err, PTMI_E_INVALID, "a grid of %u x %u x %u has a dimension above 1024", nx, ny, nz);
    if (params) {
        if (params->filter > 1u) return fail(err, PTMI_E_INVALID, "filter %u is neither 0 (nearest) nor 1 (trilinear)", params->filter);
        for (uint32_t r : params->reserved) if (r) return fail(err, PTMI_E_INVALID, "a reserved word of ptmi_medium_grid is not zero");
    }
    const size_t n = (size_t)nx * ny * nz;
    float lo = rho[0], hi = rho[0];
    double sum = 0.0;
    for (size_t i = 0; i < n; i++) {
        const float v = rho[i];
        if (!(v >= 0.0f && v <= 1.0f)) return fail(err, PTMI_E_INVALID, "density %g at entry %zu is not within [0, 1]", (double)v, i);
        lo = std::fmin(lo, v); hi = std::fmax(hi, v);
        sum += v;
    }
    if (st) {
        st->nx = nx; st->ny = ny; st->nz = nz; st->filter = params ? params->filter : 0u;
        st->rho_min = lo; st->rho_max = hi; st->rho_mean = sum / (double)n;
    }
    return PTMI_OK;
}
const ptmi_medium *pt_ctx_medium(const ptmi_ctx *c) { return c->sc.med.on ? &c->medium : nullptr; }
bool pt_ctx_has_medium_grid(const ptmi_ctx *c) { return c->sc.med.grid != nullptr; }

extern "C" {

// Checked before anything changes: a failed call leaves the grid, the context's DevScene and the device copy of that as they were.
int ptmi_upload_medium_density(ptmi_ctx *c, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz, const ptmi_medium_grid *params) {
    if (!c) return PTMI_E_INVALID;
    const bool remove = !rho || nx == 0u || ny == 0u || nz == 0u;
    struct ptmi_medium_grid_status st{};
    if (!remove) {
        if (!c->sc.med.on) return fail(c, PTMI_E_STATE, "no medium in place (ptmi_set_medium)");
        int rc = pt_check_medium_density(rho, nx, ny, nz, params, &st, c->err);
        if (!rc) rc = pt_check_medium_depth(&c->medium, c->err);
        if (rc) return rc;
    } else if (!c->sc.med.grid) {
        return PTMI_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                // nothing in flight reads the grid or the device copy any more
    Scratch<float> fresh;
    DevScene next = c->sc;
    next.med.grid = nullptr; next.med.filter = next.med.nx = next.med.ny = next.med.nz = 0u;
    if (!remove) {
        const size_t bytes = (size_t)nx * ny * nz * sizeof(float);
        HIP_TRY(c, hipMalloc(&fresh.p, bytes));
        HIP_TRY(c, hipMemcpy(fresh.p, rho, bytes, hipMemcpyHostToDevice));
        next.med.grid = fresh.p; next.med.filter = st.filter;
        next.med.nx = nx; next.med.ny = ny; next.med.nz = nz;
    }
    HIP_TRY(c, hipMemcpy(c->d_scene, &next, sizeof(DevScene), hipMemcpyHostToDevice));
    c->sc = next;
    dfree(c->d_med_grid);
    c->d_med_grid = fresh.p; fresh.p = nullptr;
    c->med_grid = st;
    return PTMI_OK;
}

int ptmi_debug_medium_grid_check(const ptmi_medium *medium, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz,
                                 const ptmi_medium_grid *params, struct ptmi_medium_grid_status *out) {
    if (!rho || nx == 0u || ny == 0u || nz == 0u) return fail(g_create_err, PTMI_E_INVALID, "no grid: rho is NULL or a dimension is 0");
    struct ptmi_medium_grid_status st{};
    int rc = medium ? pt_check_medium(medium, g_create_err) : PTMI_OK;
    if (!rc) rc = pt_check_medium_density(rho, nx, ny, nz, params, &st, g_create_err);
    if (!rc && medium) rc = pt_check_medium_depth(medium, g_create_err);
    if (!rc && out) *out = st;
    return rc;
}

int ptmi_medium_grid_status(ptmi_ctx *c, struct ptmi_medium_grid_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->med_grid;
    return PTMI_OK;
}

int ptmi_debug_medium_density(ptmi_ctx *c, uint32_t n, const float *p3, float *rho_out) {
    if (!c || !p3) return PTMI_E_INVALID;
    if (!c->sc.med.grid) return fail(c, PTMI_E_STATE, "no density grid in place (ptmi_upload_medium_density)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> dp, dr;
    HIP_TRY(c, hipMalloc(&dp.p, (size_t)n * 12)); HIP_TRY(c, hipMalloc(&dr.p, (size_t)n * 4));
    HIP_TRY(c, hipMemcpy(dp.p, p3, (size_t)n * 12, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_medium_density, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.med, dp.p, dr.p);
    HIP_TRY(c, sync_all(c));
    if (rho_out) HIP_TRY(c, hipMemcpy(rho_out, dr.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int ptmi_debug_medium_track(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, const float *t_end, const uint32_t *rng_in,
                            uint32_t mode, uint32_t *scattered, float *t_out, float *value_out, uint32_t *steps_out, uint32_t *rng_out) {
    if (!c || !o3 || !d3 || !t_end || !rng_in || mode > 1u) return PTMI_E_INVALID;
    if (!c->sc.med.grid) return fail(c, PTMI_E_STATE, "no density grid in place (ptmi_upload_medium_density)");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Scratch<float> dorg, ddir, dend, dt, dv; Scratch<uint32_t> drin, dsc, dst, drout;
    const size_t n3 = (size_t)n * 12, n1 = (size_t)n * 4;
    HIP_TRY(c, hipMalloc(&dorg.p, n3)); HIP_TRY(c, hipMalloc(&ddir.p, n3)); HIP_TRY(c, hipMalloc(&dend.p, n1));
    HIP_TRY(c, hipMalloc(&dt.p, n1)); HIP_TRY(c, hipMalloc(&dv.p, n1)); HIP_TRY(c, hipMalloc(&drin.p, n1));
    HIP_TRY(c, hipMalloc(&dsc.p, n1)); HIP_TRY(c, hipMalloc(&dst.p, n1)); HIP_TRY(c, hipMalloc(&drout.p, n1));
    HIP_TRY(c, hipMemcpy(dorg.p, o3, n3, hipMemcpyHostToDevice)); HIP_TRY(c, hipMemcpy(ddir.p, d3, n3, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dend.p, t_end, n1, hipMemcpyHostToDevice)); HIP_TRY(c, hipMemcpy(drin.p, rng_in, n1, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_medium_track, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->sc.med, mode, dorg.p, ddir.p, dend.p, drin.p,
                       dsc.p, dt.p, dv.p, dst.p, drout.p);
    HIP_TRY(c, sync_all(c));
    if (scattered) HIP_TRY(c, hipMemcpy(scattered, dsc.p, n1, hipMemcpyDeviceToHost));
    if (t_out) HIP_TRY(c, hipMemcpy(t_out, dt.p, n1, hipMemcpyDeviceToHost));
    if (value_out) HIP_TRY(c, hipMemcpy(value_out, dv.p, n1, hipMemcpyDeviceToHost));
    if (steps_out) HIP_TRY(c, hipMemcpy(steps_out, dst.p, n1, hipMemcpyDeviceToHost));
    if (rng_out) HIP_TRY(c, hipMemcpy(rng_out, drout.p, n1, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
