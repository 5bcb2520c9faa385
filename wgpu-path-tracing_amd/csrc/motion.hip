// motion.hip — reprojection across a geometry edit (ptmi_set_motion; the contract is stated in include/ptmi.h).
// The context keeps the vertex positions the history was rendered with (buf[kMotionPrev]: v0, v1, v2 as float4 per triangle) and the
// range of triangles ptmi_update_triangles has rewritten since (the dirty range). ptmi_reproject projects a hit on a triangle of that
// range from where its point was (reproject.hip k_reproject<true>), writes the motion plane, and commits: the previous positions of
// the range become the current ones. Here: the commit kernel, the buffers' lifetime, and the entry points around them.
#include "ptmi_ctx.h"

#include <cstring>
#include <vector>

namespace {

constexpr int TB = 256;

// One thread per triangle of the range: the three position rows of the 128-byte record, 16 bytes each, to the 48-byte entry. The
// record's padding words are not carried (w = 0), so the buffer's bytes depend on the positions alone.
__global__ __launch_bounds__(TB) void k_motion_commit(const ptmi_triangle *__restrict__ tris, uint32_t first, uint32_t count,
                                                       float4 *__restrict__ prev) {
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= count) return;
    const size_t tri = (size_t)first + i;
    const float4 *rec = reinterpret_cast<const float4 *>(tris + tri);
    float4 v0 = rec[0], v1 = rec[1], v2 = rec[2];
    v0.w = v1.w = v2.w = 0.0f;
    float4 *to = prev + 3u * tri;
    to[0] = v0; to[1] = v1; to[2] = v2;
}

}  // namespace

void pt_launch_motion_commit(hipStream_t s, const ptmi_triangle *tris, uint32_t first, uint32_t count, float4 *prev) {
    if (!count) return;
    hipLaunchKernelGGL(k_motion_commit, dim3((count + TB - 1) / TB), dim3(TB), 0, s, tris, first, count, prev);
}

PT_HOST {

int motion_fill(ptmi_ctx *c) {
    c->motion_dirty_first = c->motion_dirty_count = 0u;
    c->motion_epochs = 0u;
    if (!c->buf[kMotionPrev] || !c->sc.n_tris) return PTMI_OK;
    pt_launch_motion_commit(c->stream, c->sc.tris, 0u, c->sc.n_tris, static_cast<float4 *>(c->buf[kMotionPrev]));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

void motion_widen(ptmi_ctx *c, uint32_t first, uint32_t count) {
    if (!c->motion_on || !count) return;
    if (!c->motion_dirty_count) { c->motion_dirty_first = first; c->motion_dirty_count = count; return; }
    const uint32_t lo = first < c->motion_dirty_first ? first : c->motion_dirty_first;
    const uint32_t end_a = first + count, end_b = c->motion_dirty_first + c->motion_dirty_count;
    c->motion_dirty_first = lo; c->motion_dirty_count = (end_a > end_b ? end_a : end_b) - lo;
}

int motion_commit(ptmi_ctx *c) {
    if (c->motion_dirty_count && c->buf[kMotionPrev]) {
        pt_launch_motion_commit(c->stream, c->sc.tris, c->motion_dirty_first, c->motion_dirty_count, static_cast<float4 *>(c->buf[kMotionPrev]));
        HIP_TRY(c, hipGetLastError());
    }
    c->motion_dirty_first = c->motion_dirty_count = 0u;
    c->motion_epochs++;
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

// Both buffers exist before anything of the context changes, so a failed call leaves the previous state in place.
int ptmi_set_motion(ptmi_ctx *c, uint32_t on) {
    if (!c) return PTMI_E_INVALID;
    if (on > 1u) return fail(c, PTMI_E_INVALID, "on = %u is not 0 or 1", on);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                     // nothing in flight reads or writes a buffer that goes
    if (!on) {
        dfree(c->buf[kMotionPrev]); dfree(c->plane[kMotion]);
        c->motion_on = false;
        c->motion_dirty_first = c->motion_dirty_count = 0u; c->motion_epochs = 0u;
        return PTMI_OK;
    }
    void *prev = nullptr;
    if (c->have_scene && !c->buf[kMotionPrev]) {
        const size_t bytes = motion_prev_bytes(c->sc.n_tris);
        hipError_t e = hipMalloc(&prev, bytes);
        if (e == hipSuccess && !c->sc.n_tris) e = hipMemset(prev, 0, bytes);
        if (e != hipSuccess) {
            dfree(prev);
            (void)hipGetLastError();
            return fail(c, PTMI_E_HIP, "allocation of %zu bytes of previous positions failed: %s (motion is as it was)", bytes, hipGetErrorString(e));
        }
    }
    const int rc = make_planes(c, bit(kMotion), (size_t)c->W * c->H, c->plane);     // a plane already on keeps its contents
    if (rc) { dfree(prev); return rc; }
    if (prev) c->buf[kMotionPrev] = prev;
    c->motion_on = true;
    const int rf = motion_fill(c);               // previous := current, whether the buffer is new or not
    if (rf) return rf;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_get_motion(const ptmi_ctx *c, uint32_t *on) {
    if (!c || !on) return PTMI_E_INVALID;
    *on = c->motion_on ? 1u : 0u;
    return PTMI_OK;
}

int ptmi_motion_commit(ptmi_ctx *c) {
    if (!c) return PTMI_E_INVALID;
    if (!c->motion_on) return fail(c, PTMI_E_STATE, "motion is off (ptmi_set_motion)");
    HIP_TRY(c, hipSetDevice(c->device));
    return motion_commit(c);
}

int ptmi_motion_status(ptmi_ctx *c, struct ptmi_motion_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    unsigned long long h[2];
    HIP_TRY(c, hipMemcpy(h, &c->d_counters[kCtRpMoved], sizeof h, hipMemcpyDeviceToHost));
    out->on = c->motion_on ? 1u : 0u; out->epochs = c->motion_epochs;
    out->dirty_first = c->motion_dirty_first; out->dirty_count = c->motion_dirty_count;
    out->moved = h[0]; out->moved_carried = h[kCtRpMovedCarried - kCtRpMoved];
    return PTMI_OK;
}

int ptmi_read_motion(ptmi_ctx *c, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!c->motion_on) return fail(c, PTMI_E_STATE, "motion is off (ptmi_set_motion)");
    if (!c->plane[kMotion]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    const size_t want = (size_t)c->W * c->H * 4;
    if (n_floats != want) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", want, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, hipMemcpy(dst, c->plane[kMotion], want * sizeof(float), hipMemcpyDeviceToHost));
    return PTMI_OK;
}

void *ptmi_motion_device_ptr(ptmi_ctx *c) { return c && c->motion_on ? c->plane[kMotion] : nullptr; }

int ptmi_debug_motion_prev(ptmi_ctx *c, uint32_t first, uint32_t count, float *v9) {
    if (!c) return PTMI_E_INVALID;
    if (!c->motion_on) return fail(c, PTMI_E_STATE, "motion is off (ptmi_set_motion)");
    if (!c->have_scene || !c->buf[kMotionPrev]) return fail(c, PTMI_E_STATE, "no scene uploaded (ptmi_upload_scene)");
    if ((uint64_t)first + count > c->sc.n_tris)
        return fail(c, PTMI_E_INVALID, "triangles [%u, +%u) reach beyond the %u uploaded", first, count, c->sc.n_tris);
    if (!count) return PTMI_OK;
    if (!v9) return fail(c, PTMI_E_INVALID, "v9 is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    std::vector<float4> h((size_t)count * 3u);
    HIP_TRY(c, hipMemcpy(h.data(), static_cast<const float4 *>(c->buf[kMotionPrev]) + 3u * (size_t)first, h.size() * sizeof(float4),
                         hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); i++) { v9[3 * i] = h[i].x; v9[3 * i + 1] = h[i].y; v9[3 * i + 2] = h[i].z; }
    return PTMI_OK;
}

}  // extern "C"
