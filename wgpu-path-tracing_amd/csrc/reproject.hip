// reproject.hip — ptmi_reproject, step 4: the planes of the camera `to` from the snapshot of the planes of the camera `from`
// (the temporal half of Schied et al. 2017; denoise.hip is the spatial half). The contract is stated in include/ptmi.h and restated
// in numpy by tests/reproject_ref.py; every expression here is written in that order. The library builds with -ffp-contract=off, so
// the only operations are float32 + - *, the correctly rounded / and sqrt, floor, comparisons and one tan1: the model agrees bit for bit.
//
// One thread per pixel of the context's rows. The centre ray of the pixel under `to` and its closest hit (t, tri) are given (the
// centre-ray kernel of pipeline.hip, then `extend`); the hit point is projected into `from`, and the four snapshot pixels around it
// that show the same surface (depth within the tolerance, same material when ids are compared) and hold samples are blended.
//
// k_reproject<true, *> is the pass while ptmi_set_motion is on: a hit on a triangle that moved since the history was rendered is projected
// from where its point was then (the hit's barycentrics on the previous positions), and every pixel writes the motion plane. The moved
// test starts with the dirty range, two kernel arguments, so a wave whose hits all lie outside it reads nothing more than
// k_reproject<false, *>, which is the kernel of a context with motion off, unchanged.
//
// ORTHO is the projection of `from` (ptmi_set_projections): an orthographic camera's image coordinates are the point's right / up
// components over the half extents, with no perspective divide, and its depth is zf, the t along a ray that starts on the camera
// plane. k_reproject<*, false> is the pinhole's kernel, unchanged. The camera `to` enters through its centre rays alone.
//
// k_hit_uv writes the barycentrics that pass reads (ReprojectArgs::uv); ptmi_debug_intersect reports them too.
#include "pt_device.h"
#include "pt_math.h"
#include "pt_hit.h"

namespace {

constexpr int RX = 64, RY = 4;          // like denoise.hip: a wave is one 64-pixel row segment

PT_DEV bool finite3(float4 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }
PT_DEV float dot_plain(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

enum { CARRIED = 0, DISOCCLUDED = 1, MISSED = 2 };

PT_DEV bool same_bits3(float4 p, const float *q) {
    return __float_as_uint(p.x) == __float_as_uint(q[0]) && __float_as_uint(p.y) == __float_as_uint(q[1]) &&
           __float_as_uint(p.z) == __float_as_uint(q[2]);
}

template <bool MOTION, bool ORTHO> __global__ __launch_bounds__(RX * RY) void k_reproject(ReprojectArgs a) {
    const DevBand &band = a.band;
    const uint32_t W = band.width, H = band.height;
    const uint32_t x = blockIdx.x * RX + threadIdx.x, l = blockIdx.y * RY + threadIdx.y;
    const bool in = x < W && l < band.rows;          // every lane stays for the wave reduction at the end
    int outcome = -1;
    float count = 0.0f;
    bool moved = false;
    if (in) {
        const uint32_t p = l * W + x;
        const size_t oi = (size_t)band.row_of(l) * W + x;
        const float2 hit = a.hits[p];
        const uint32_t tri = __float_as_uint(hit.y);
        float4 o_out = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o_mom = o_out, o_nrm = o_out, o_alb = o_out;
        uint2 o_ids = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        float m_x = 0.0f, m_y = 0.0f, m_z = 0.0f;                // the motion plane's x, y, z (MOTION only)
        outcome = MISSED;
        if (tri != 0xFFFFFFFFu) {
            outcome = DISOCCLUDED;
            const float t = hit.x;
            const uint32_t mat = tri < a.n_tris ? a.tris[tri].material_index : 0xFFFFFFFFu;
            o_ids = make_uint2(tri, mat);
            const float4 o = a.O[p], d = a.D[p];
            const ptmi_camera &cam = a.from;
            float Px = o.x + t * d.x, Py = o.y + t * d.y, Pz = o.z + t * d.z;
            if (MOTION && tri >= a.dirty_first && tri < a.dirty_end && tri < a.n_tris) {
                // MOVED: in the dirty range, and a previous position differs in its bits from the current one
                const float4 p0 = a.prev[3u * (size_t)tri], p1 = a.prev[3u * (size_t)tri + 1u], p2 = a.prev[3u * (size_t)tri + 2u];
                const ptmi_triangle &T = a.tris[tri];
                moved = !(same_bits3(p0, T.v0) && same_bits3(p1, T.v1) && same_bits3(p2, T.v2));
                if (moved) {
                    const float2 uv = a.uv[p];
                    Px = (p0.x + uv.x * (p1.x - p0.x)) + uv.y * (p2.x - p0.x);
                    Py = (p0.y + uv.x * (p1.y - p0.y)) + uv.y * (p2.y - p0.y);
                    Pz = (p0.z + uv.x * (p1.z - p0.z)) + uv.y * (p2.z - p0.z);
                }
            }
            const float vx = Px - cam.position[0], vy = Py - cam.position[1], vz = Pz - cam.position[2];
            const float zf = dot_plain(vx, vy, vz, cam.forward[0], cam.forward[1], cam.forward[2]);
            const float dist = ORTHO ? zf : sqrt1(dot_plain(vx, vy, vz, vx, vy, vz));
            const float th = ORTHO ? __uint_as_float(cam._p3[1]) : tan1(cam.fov * 0.5f);      // orthographic: ymag, the half-height
            if (zf > 0.0f) {
                const float sx = dot_plain(vx, vy, vz, cam.right[0], cam.right[1], cam.right[2]) / (ORTHO ? th * cam.aspect : zf * th * cam.aspect);
                const float sy = dot_plain(vx, vy, vz, cam.up[0], cam.up[1], cam.up[2]) / (ORTHO ? th : zf * th);
                const float fx = (sx + 1.0f) * 0.5f * (float)W - 0.5f;
                const float fy = (sy + 1.0f) * 0.5f * (float)H - 0.5f;
                if (__builtin_isfinite(fx) && __builtin_isfinite(fy)) {
                    if (MOTION) { m_x = fx - (float)x; m_y = fy - (float)band.row_of(l); m_z = dist; }
                    const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
                    const float ax = fx - x0, ay = fy - y0;
                    const float tol = a.depth_tolerance * dist;
                    float sw = 0.0f, nmin = __builtin_inff();
                    float s_out[3] = {0.0f, 0.0f, 0.0f}, s_mom[2] = {0.0f, 0.0f}, s_alb[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s_nrm[3] = {0.0f, 0.0f, 0.0f};
                    bool any = false;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = k & 1, j = k >> 1;
                        const float qxf = x0 + (float)i, qyf = y0 + (float)j;
                        if (!(qxf >= 0.0f && qxf < (float)W && qyf >= 0.0f && qyf < (float)H)) continue;
                        const uint32_t qx = (uint32_t)qxf, qy = (uint32_t)qyf;
                        if (!band.has_row(qy)) continue;
                        const size_t qi = (size_t)qy * W + qx;
                        const float4 qm = a.h_mom[qi], qn = a.h_normal[qi];
                        if (!(qm.z >= 1.0f) || !(qn.w > 0.0f)) continue;
                        if (!(__builtin_fabsf(qn.w - dist) <= tol)) continue;
                        const float4 qo = a.h_out[qi];
                        if (!finite3(qo) || !finite3(qm) || !finite3(qn) || !__builtin_isfinite(qn.w)) continue;
                        float4 qa = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if (a.h_albedo) {
                            qa = a.h_albedo[qi];
                            if (!finite3(qa) || !__builtin_isfinite(qa.w)) continue;
                        }
                        if (a.match_ids && a.h_ids[qi].y != mat) continue;
                        const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        any = true;
                        sw = sw + w;
                        s_out[0] = s_out[0] + w * qo.x; s_out[1] = s_out[1] + w * qo.y; s_out[2] = s_out[2] + w * qo.z;
                        s_mom[0] = s_mom[0] + w * qm.x; s_mom[1] = s_mom[1] + w * qm.y;
                        s_alb[0] = s_alb[0] + w * qa.x; s_alb[1] = s_alb[1] + w * qa.y; s_alb[2] = s_alb[2] + w * qa.z; s_alb[3] = s_alb[3] + w * qa.w;
                        s_nrm[0] = s_nrm[0] + w * qn.x; s_nrm[1] = s_nrm[1] + w * qn.y; s_nrm[2] = s_nrm[2] + w * qn.z;
                        nmin = qm.z < nmin ? qm.z : nmin;
                    }
                    if (any && sw > 0.0f) {
                        outcome = CARRIED;
                        const float cap = (float)a.max_history;
                        count = nmin < cap ? nmin : cap;
                        o_out = make_float4(s_out[0] / sw, s_out[1] / sw, s_out[2] / sw, 0.0f);
                        o_mom = make_float4(s_mom[0] / sw, s_mom[1] / sw, count, 0.0f);
                        o_alb = make_float4(s_alb[0] / sw, s_alb[1] / sw, s_alb[2] / sw, s_alb[3] / sw);
                        o_nrm = make_float4(s_nrm[0] / sw, s_nrm[1] / sw, s_nrm[2] / sw, t);
                    }
                }
            }
        }
        a.out[oi] = o_out;
        a.mom[oi] = o_mom;
        a.normal[oi] = o_nrm;
        if (a.albedo) a.albedo[oi] = o_alb;
        if (a.ids) a.ids[oi] = o_ids;
        if (MOTION) a.motion[oi] = make_float4(m_x, m_y, m_z, (float)outcome);
    }
    // the counters: per wave, then one atomic each from its first lane (integers: order-free)
    const unsigned long long n_carried = __popcll(__ballot(outcome == CARRIED)), n_dis = __popcll(__ballot(outcome == DISOCCLUDED)),
                             n_missed = __popcll(__ballot(outcome == MISSED));
    uint32_t samples = (uint32_t)count;              // at most 2^24 each, 64 lanes
    for (int off = 32; off > 0; off >>= 1) samples += __shfl_down(samples, off);
    if ((threadIdx.x & 63u) == 0u) {
        if (n_carried) atomicAdd(&a.status[kCtRpCarried], n_carried);
        if (n_dis) atomicAdd(&a.status[kCtRpDisoccluded], n_dis);
        if (n_missed) atomicAdd(&a.status[kCtRpMissed], n_missed);
        if (samples) atomicAdd(&a.status[kCtRpSamples], (unsigned long long)samples);
    }
    if (MOTION) {
        const unsigned long long n_moved = __popcll(__ballot(moved)), n_moved_carried = __popcll(__ballot(moved && outcome == CARRIED));
        if ((threadIdx.x & 63u) == 0u) {
            if (n_moved) atomicAdd(&a.status[kCtRpMoved], n_moved);
            if (n_moved_carried) atomicAdd(&a.status[kCtRpMovedCarried], n_moved_carried);
        }
    }
}

// (u, v) of every hit, which the 8-byte hit record does not carry (pt_hit.h); a miss gets (0, 0)
__global__ void k_hit_uv(uint32_t n, DevScene sc, DevPaths P, const float2 *__restrict__ hits, float2 *__restrict__ uv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 h = hits[i];
    float u = 0.0f, v = 0.0f;
    if (!(h.x < 0.0f)) (void)tri_hit(sc.tris[__float_as_uint(h.y)], xyz(P.O[i]), xyz(P.D[i]), u, v);
    uv[i] = make_float2(u, v);
}

}  // namespace

void pt_launch_hit_uv(hipStream_t s, uint32_t n, const DevScene &sc, DevPaths p, const float2 *hits, float2 *uv) {
    hipLaunchKernelGGL(k_hit_uv, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, p, hits, uv);
}

void pt_launch_reproject(hipStream_t s, const ReprojectArgs &a) {
    const dim3 grid((a.band.width + RX - 1) / RX, (a.band.rows + RY - 1) / RY), block(RX, RY);
    const bool ortho = a.from_proj == PTMI_PROJ_ORTHOGRAPHIC;
    auto *const k = a.motion ? (ortho ? k_reproject<true, true> : k_reproject<true, false>)
                             : (ortho ? k_reproject<false, true> : k_reproject<false, false>);
    hipLaunchKernelGGL(k, grid, block, 0, s, a);
}
