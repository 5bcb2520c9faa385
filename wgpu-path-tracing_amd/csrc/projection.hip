// projection.hip — camera projections (ptmi_set_projections; the contract is stated in include/ptmi.h): the context's
// switch, and the one check every entry that takes a camera runs before it enqueues anything. The rays themselves are the
// projection's instantiations of camera_dir / camera_ray in pipeline.hip; reproject.hip has the orthographic inverse.
#include "ptmi_ctx.h"

#include <cmath>

int pt_check_camera(const ptmi_ctx *c, const ptmi_camera *cam, uint32_t *kind, std::string &err) {
    *kind = PTMI_PROJ_PERSPECTIVE;
    if (!c->projections_on) return PTMI_OK;                     // the words are padding: not read
    const uint32_t k = ptmi_camera_projection(cam);
    if (k > PTMI_PROJ_EQUIRECT) return pt_host::fail(err, PTMI_E_INVALID, "unknown camera projection %u", k);
    if (k == PTMI_PROJ_ORTHOGRAPHIC) {
        const float ymag = ptmi_camera_ymag(cam);
        if (!std::isfinite(ymag) || !(ymag > 0.0f))
            return pt_host::fail(err, PTMI_E_INVALID, "orthographic camera: ymag %g is not finite and positive", (double)ymag);
    }
    *kind = k;
    return PTMI_OK;
}

extern "C" {

int ptmi_set_projections(ptmi_ctx *c, uint32_t on) {
    if (!c) return PTMI_E_INVALID;
    if (on > 1u) return fail(c, PTMI_E_INVALID, "on = %u is not 0 or 1", on);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    c->projections_on = on != 0;
    return PTMI_OK;
}

int ptmi_get_projections(const ptmi_ctx *c, uint32_t *on) {
    if (!c || !on) return PTMI_E_INVALID;
    *on = c->projections_on ? 1u : 0u;
    return PTMI_OK;
}

}  // extern "C"
