// scene_pose.hip — what the three pose sources share on the host (scene_transform.hip: triangle groups; scene_skin.hip: the skin;
// scene_morph.hip: the morph; DESIGN.md §17 "The shared pose sequence"): the check-then-write sequence of a refusable pose and the
// snapshot of a rest pose. ptmi_ctx.h has the contract of both; pt_transform.h has what their kernels share on the device.
#include "ptmi_ctx.h"
#include "pt_transform.h"

namespace {

// a thread per float4 of the rest rows [first, first + count): row e is triangle list[e], or triangle e where there is no list
__global__ void __launch_bounds__(TB) k_pose_snapshot(uint32_t first, uint32_t count, const uint32_t *__restrict__ list,
                                                      const float4 *__restrict__ live, float4 *__restrict__ rest) {
    const size_t i = (size_t)blockIdx.x * TB + threadIdx.x;
    if (i >= (size_t)count * kRestQ) return;
    const size_t e = first + i / kRestQ, q = i % kRestQ;
    rest[e * kRestQ + q] = live[(list ? (size_t)list[e] : e) * kLiveQ + q];
}

}  // namespace

PT_HOST {

int pose_snapshot(ptmi_ctx *c, uint32_t first, uint32_t count, const void *list, void *rest) {
    if (!count) return PTMI_OK;
    const size_t threads = (size_t)count * kRestQ;
    k_pose_snapshot<<<dim3((unsigned)((threads + TB - 1) / TB)), TB, 0, c->stream>>>(
        first, count, static_cast<const uint32_t *>(list), reinterpret_cast<const float4 *>(c->sc.tris), static_cast<float4 *>(rest));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int pose_refusable(ptmi_ctx *c, std::chrono::steady_clock::time_point t0, const PoseCall &p) {
    int rc = refit_begin(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                                        // nothing in flight reads the scene any more
    if (p.moves) {
        if ((rc = p.stage())) return rc;
        // the check pass: nothing of the scene is written before it has found nothing
        if ((rc = p.pass(false))) return rc;
        uint32_t bad = kNone;
        HIP_TRY(c, hipMemcpyAsync(&bad, p.check_word, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (bad != kNone) {
            *p.first_bad = bad;
            return fail(c, PTMI_E_INVALID, "triangle %u: a %s vertex is not finite%s (nothing was changed)", bad, p.how,
                        c->sc.own ? ", or an edge is too long for float32 arithmetic" : "");
        }
    }
    if (!p.refit) {                                                 // no live record is written: the pass, and nothing of the refit
        if (p.moves && (rc = p.pass(true))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return PTMI_OK;
    }
    if ((rc = refit_ready(c))) return rc;                           // the plan, at the first edit after an upload
    if (p.moves) {
        if ((rc = p.pass(true))) return rc;
        motion_widen(c, p.lo, p.hi - p.lo + 1u);                    // while motion is on: from the lowest to the highest triangle moved
    }
    return refit_written(c, t0);
}

}  // namespace pt_host
