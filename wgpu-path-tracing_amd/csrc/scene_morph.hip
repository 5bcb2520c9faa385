// scene_morph.hip — morphed triangles posed on the device (include/ptmi.h: ptmi_set_morph, ptmi_pose_morph).
//
// The caller lists the morphed triangles once (ascending indices) with a sparse table of deltas in compressed-row form: entry e of the
// list has the records [rows[e], rows[e + 1]), one per target that displaces it, 96 bytes each (ptmi_morph_delta: dv0, dv1, dv2, dn0,
// dn1, dn2 with the target in the first float4's fourth word). The context keeps, per entry, the index (buf[kMorphList]), the row
// bounds (buf[kMorphRows]), the REST POSE (buf[kMorphRest], 96 bytes) and where the result goes (buf[kMorphSkinRow]); per record, the
// record (buf[kMorphDeltas]) and, beside it, its target word alone (buf[kMorphTargets]), so that a record of weight zero costs a
// 4-byte load and not a 96-byte one. ptmi_pose_morph sends one weight per target: every entry becomes its rest record plus the
// weighted records of its row, and the refit of ptmi_update_triangles follows (scene_update.hip refit_written).
//
// All-or-nothing by a CHECK PASS followed by a WRITE PASS (scene_pose.hip pose_refusable; the check word is word 0 of
// buf[kMorphWeights]). This file's own: the list and the rows, the sum, where an entry's result goes, and k_morph, one kernel template
// for both passes.
//
// Layout: as k_skin's (pt_transform.h Octet): eight lanes per entry, lane q < 6 owns float4 q of the rest record and of every delta
// record of the row. ROWS DIFFER IN LENGTH, so the row loop's trip count differs between the octets of a wave: the loop therefore
// contains NO cross-lane operation (every lane reads the row bounds, the target words and the weights it needs itself; the eight lanes
// of an octet read the same words, which the memory system serves as one), and the only cross-lane steps, the __shfl and the ballot of
// check_tail, stand behind it where every lane of the wave arrives. The weights sit in LDS (at most kMaxTargets = 8 192 of them, 32 KB).
//
// Morph and skin compose in glTF's order: an entry whose triangle the skin lists too writes its six float4 to that triangle's row of
// buf[kSkinRest] instead of the live record, and ptmi_pose_skin carries it on. The entry -> row map is made on the host from the two
// ascending lists (morph_relink) by whichever of ptmi_set_skin / ptmi_set_morph ran last.
#include "ptmi_ctx.h"
#include "pt_dev_scratch.h"
#include "pt_transform.h"   // the octet layout, the check tail and the constants, shared with scene_transform.hip and scene_skin.hip

#include <algorithm>
#include <chrono>
#include <cmath>

namespace {

constexpr uint32_t kMaxTargets = 8192u;      // the weights of a pose a block keeps in LDS
static_assert(sizeof(ptmi_morph_delta) == 96 && sizeof(ptmi_morph_delta) == kRestQ * sizeof(float4), "a delta record is 6 float4");
static_assert(offsetof(ptmi_morph_delta, target) == 12, "the target is the fourth word of a delta record");
static_assert(sizeof(struct ptmi_morph_status) == 48, "ptmi_morph_status is 48 bytes");
static_assert(kMaxTargets * sizeof(float) == 32u * 1024u, "the weights take 32 KB of LDS at most");

// The list entries [0, n_listed). WRITE: the six float4 of every entry go to its live record, or to row skin_row[entry] of skin_rest
// where that is not kNone. Otherwise nothing is written: the three vertices are checked and the smallest offending triangle goes to
// *first_bad. The row loop has no cross-lane operation (see above); no lane returns early, and the round loop's bounds are the same for
// a whole block, so every lane of a wave reaches check_tail.
template <bool WRITE>
__global__ void __launch_bounds__(TB) k_morph(uint32_t n_listed, const uint32_t *__restrict__ list, const uint32_t *__restrict__ rows,
                                              const uint32_t *__restrict__ targets, const float4 *__restrict__ deltas,
                                              const float4 *__restrict__ rest, const uint32_t *__restrict__ skin_row,
                                              const float *__restrict__ weights, uint32_t n_targets, float4 *live, float4 *skin_rest,
                                              uint32_t own, uint32_t *first_bad) {
    extern __shared__ float s_weights[];
    for (uint32_t i = threadIdx.x; i < n_targets; i += TB) s_weights[i] = weights[i];
    __syncthreads();
    const Octet o = octet_here();
    uint32_t worst = kNone;                                              // the smallest offending list entry this lane has seen
    for (uint32_t base = blockIdx.x * kOctets; base < n_listed; base += octet_stride()) {
        const uint32_t entry = base + o.slot;
        const bool listed = entry < n_listed;
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t r0 = 0u, r1 = 0u;
        if (listed) {
            r0 = rows[entry]; r1 = rows[entry + 1u];
            if (o.l8 < 6u) p = rest[(size_t)entry * kRestQ + o.l8];
        }
        bool applied = false;
        for (uint32_t r = r0; r < r1; r++) {                             // (no cross-lane operation in here)
#ifdef PT_MORPH_LOAD_FIRST                                               // the measurement's other form: the record is loaded before its weight is known
            float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (o.l8 < 6u) d = deltas[(size_t)r * kRestQ + o.l8];
            const float w = s_weights[targets[r]];
            if (w == 0.0f) continue;
            applied = true;
#else
            const float w = s_weights[targets[r]];
            if (w == 0.0f) continue;                                     // either sign: skipped, not loaded, not added
            applied = true;
            float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (o.l8 < 6u) d = deltas[(size_t)r * kRestQ + o.l8];
#endif
            p.x = p.x + w * d.x; p.y = p.y + w * d.y; p.z = p.z + w * d.z;   // the product rounded, then the sum (-ffp-contract=off)
        }
        float4 res = p;                                                  // (the fourth word keeps its bits: nothing was added to it)
        if (applied && o.l8 >= 3u && o.l8 < 6u) {                        // the normal tail of transform_row
            const float l2 = (p.x * p.x + p.y * p.y) + p.z * p.z;
            if (l2 > 0.0f) {
                const float len = __builtin_sqrtf(l2);
                res.x = p.x / len; res.y = p.y / len; res.z = p.z / len;
            }
        }
        if (WRITE) {
            if (listed && o.l8 < 6u) {
                const uint32_t row = skin_row[entry];
                if (row == kNone) live[(size_t)list[entry] * kLiveQ + o.l8] = res;
                else skin_rest[(size_t)row * kRestQ + o.l8] = res;
            }
        } else {
            worst = check_tail(o, res, listed, own, base, worst);
        }
    }
    if (!WRITE && o.lane == 0u && worst != kNone) atomicMin(first_bad, list[worst]);   // (the list ascends: the smallest entry is the smallest triangle)
}

uint32_t *head_of(ptmi_ctx *c) { return static_cast<uint32_t *>(c->buf[kMorphWeights]); }

template <bool WRITE>
int run_pass(ptmi_ctx *c) {
    const uint32_t n = c->morph.n_morphed, nt = c->morph.n_targets;
    k_morph<WRITE><<<pose_blocks(n, c->n_cu), TB, (size_t)nt * sizeof(float), c->stream>>>(
        n, static_cast<const uint32_t *>(c->buf[kMorphList]), static_cast<const uint32_t *>(c->buf[kMorphRows]),
        static_cast<const uint32_t *>(c->buf[kMorphTargets]), static_cast<const float4 *>(c->buf[kMorphDeltas]),
        static_cast<const float4 *>(c->buf[kMorphRest]), static_cast<const uint32_t *>(c->buf[kMorphSkinRow]),
        reinterpret_cast<const float *>(reinterpret_cast<const char *>(c->buf[kMorphWeights]) + kPoseHeadBytes), nt,
        reinterpret_cast<float4 *>(const_cast<ptmi_triangle *>(c->sc.tris)), static_cast<float4 *>(c->buf[kSkinRest]), c->sc.own, head_of(c));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

// entry -> the row of the skin's rest pose that lists the same triangle (kNone: none), from the two ascending lists; *lo / *hi: the
// lowest and the highest morphed triangle outside the skin (lo > hi: there is none). Returns how many entries are in the skin.
uint32_t link_lists(const std::vector<uint32_t> &morph, const std::vector<uint32_t> &skin, std::vector<uint32_t> &map, uint32_t *lo, uint32_t *hi) {
    map.assign(morph.size(), kNone);
    *lo = kNone; *hi = 0u;
    uint32_t in_skin = 0u;
    size_t s = 0;
    for (size_t e = 0; e < morph.size(); e++) {
        while (s < skin.size() && skin[s] < morph[e]) s++;
        if (s < skin.size() && skin[s] == morph[e]) { map[e] = (uint32_t)s; in_skin++; }
        else { *lo = std::min(*lo, morph[e]); *hi = std::max(*hi, morph[e]); }
    }
    return in_skin;
}

}  // namespace

int pt_check_morph(const ptmi_ctx *c, const uint32_t *triangle, const uint32_t *row_start, const ptmi_morph_delta *deltas, uint32_t n,
                   uint32_t n_targets, std::string &err) {
    if (!c->have_scene) return fail(err, PTMI_E_INVALID, "no scene is loaded (ptmi_upload_scene)");
    if (!triangle || n == 0u) return PTMI_OK;                       // a removal
    if (n_targets == 0u) return fail(err, PTMI_E_INVALID, "n_targets is 0");
    if (n_targets > kMaxTargets) return fail(err, PTMI_E_UNSUPPORTED, "%u targets: at most %u", n_targets, kMaxTargets);
    if (!row_start && deltas) return fail(err, PTMI_E_INVALID, "row_start is NULL");
    if (row_start && row_start[0] != 0u) return fail(err, PTMI_E_INVALID, "row_start[0] is %u: the rows start at 0", row_start[0]);
    for (uint32_t i = 0; i < n; i++) {
        if (triangle[i] >= c->sc.n_tris) return fail(err, PTMI_E_INVALID, "entry %u names triangle %u of %u", i, triangle[i], c->sc.n_tris);
        if (i && triangle[i] <= triangle[i - 1]) return fail(err, PTMI_E_INVALID, "entry %u: the list is not strictly ascending", i);
        if (row_start && row_start[i + 1] < row_start[i]) return fail(err, PTMI_E_INVALID, "row_start[%u] is below row_start[%u]", i + 1u, i);
    }
    if (!row_start || row_start[n] == 0u) return PTMI_OK;           // every row is empty
    if (!deltas) return fail(err, PTMI_E_INVALID, "deltas is NULL");
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t r = row_start[i]; r < row_start[i + 1]; r++) {
            const ptmi_morph_delta &d = deltas[r];
            if (d.target >= n_targets) return fail(err, PTMI_E_INVALID, "entry %u record %u names target %u of %u", i, r, d.target, n_targets);
            if (r > row_start[i] && d.target <= deltas[r - 1].target)
                return fail(err, PTMI_E_INVALID, "entry %u record %u: the targets of a row are not strictly ascending", i, r);
            if (d.reserved0 || d.reserved1 || d.reserved2 || d.reserved3 || d.reserved4)
                return fail(err, PTMI_E_INVALID, "entry %u record %u: ptmi_morph_delta.reserved must be 0", i, r);
            for (const float *v : {d.dv0, d.dv1, d.dv2, d.dn0, d.dn1, d.dn2})
                for (int k = 0; k < 3; k++)
                    if (!std::isfinite(v[k])) return fail(err, PTMI_E_INVALID, "entry %u record %u: a delta is not finite", i, r);
        }
    return PTMI_OK;
}

int pt_check_morph_pose(const ptmi_ctx *c, const float *weights, uint32_t n_targets, std::string &err) {
    if (!c->morph.present) return fail(err, PTMI_E_STATE, "no morph is in place (ptmi_set_morph)");
    if (!weights) return fail(err, PTMI_E_INVALID, "weights is NULL");
    if (n_targets != c->morph.n_targets) return fail(err, PTMI_E_INVALID, "%u weights: the morph was set with %u targets", n_targets, c->morph.n_targets);
    for (uint32_t i = 0; i < n_targets; i++)
        if (!std::isfinite(weights[i])) return fail(err, PTMI_E_INVALID, "weight %u is not finite", i);
    return PTMI_OK;
}

PT_HOST {

void morph_forget(ptmi_ctx *c) {
    for (SceneBuf k : {kMorphList, kMorphRows, kMorphTargets, kMorphDeltas, kMorphRest, kMorphSkinRow, kMorphWeights}) dfree(c->buf[k]);
    c->morph_list.clear();
    c->morph_lo = c->morph_hi = 0u;
    c->morph = {};
}

int morph_rebase(ptmi_ctx *c, uint32_t first, uint32_t count) {
    if (!c->morph.present) return PTMI_OK;
    const auto &l = c->morph_list;
    const uint32_t e0 = (uint32_t)(std::lower_bound(l.begin(), l.end(), first) - l.begin());
    const uint64_t end = (uint64_t)first + count;
    const uint32_t e1 = end > kNone ? (uint32_t)l.size() : (uint32_t)(std::lower_bound(l.begin(), l.end(), (uint32_t)end) - l.begin());
    return pose_snapshot(c, e0, e1 - e0, c->buf[kMorphList], c->buf[kMorphRest]);
}

int morph_relink(ptmi_ctx *c) {
    if (!c->morph.present) return PTMI_OK;
    std::vector<uint32_t> map;
    uint32_t lo, hi;
    const uint32_t in_skin = link_lists(c->morph_list, c->skin_list, map, &lo, &hi);
    HIP_TRY(c, hipMemcpy(c->buf[kMorphSkinRow], map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->morph.n_in_skin = in_skin; c->morph.skin_stale = 0u;
    c->morph_lo = lo; c->morph_hi = hi;
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

// The new buffers exist and are filled before anything of the context changes, so a failed call keeps the previous morph.
int ptmi_set_morph(ptmi_ctx *c, const uint32_t *triangle, const uint32_t *row_start, const ptmi_morph_delta *deltas, uint32_t n,
                   uint32_t n_targets) {
    if (!c) return PTMI_E_INVALID;
    const int rc = pt_check_morph(c, triangle, row_start, deltas, n, n_targets, c->err);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    if (!triangle || n == 0u) { morph_forget(c); return PTMI_OK; }
    const std::vector<uint32_t> rows_h = row_start ? std::vector<uint32_t>(row_start, row_start + n + 1u) : std::vector<uint32_t>(n + 1u, 0u);
    const uint32_t nr = rows_h[n];
    std::vector<uint32_t> targets_h(nr), listed(triangle, triangle + n), map;
    for (uint32_t r = 0; r < nr; r++) targets_h[r] = deltas[r].target;
    uint32_t lo, hi;
    const uint32_t in_skin = link_lists(listed, c->skin_list, map, &lo, &hi);
    const size_t rec = (size_t)n * kRestQ * sizeof(float4), drec = (size_t)nr * sizeof(ptmi_morph_delta);
    DevScratch fresh;                                               // freed on every way out but the last
    uint32_t *list = fresh.get<uint32_t>(n), *rows = fresh.get<uint32_t>((size_t)n + 1u), *tg = fresh.get<uint32_t>(std::max(nr, 1u));
    uint32_t *srow = fresh.get<uint32_t>(n);
    char *dl = fresh.get<char>(std::max(drec, sizeof(ptmi_morph_delta))), *rest = fresh.get<char>(rec);
    char *wts = fresh.get<char>(kPoseHeadBytes + (size_t)n_targets * sizeof(float));
    hipError_t e = fresh.error;
    int rs = PTMI_OK;
    if (hip_ok(e) && hip_ok(e = hipMemcpy(list, triangle, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        hip_ok(e = hipMemcpy(rows, rows_h.data(), ((size_t)n + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        hip_ok(e = hipMemcpy(srow, map.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
        (!nr || (hip_ok(e = hipMemcpy(tg, targets_h.data(), (size_t)nr * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
                 hip_ok(e = hipMemcpy(dl, deltas, drec, hipMemcpyHostToDevice)))) &&
        !(rs = pose_snapshot(c, 0u, n, list, rest)))
        e = hipStreamSynchronize(c->stream);
    if (rs) return rs;
    if (!hip_ok(e)) {
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "the morph could not be made: %s (the previous morph, if any, is still in place)", hipGetErrorString(e));
    }
    morph_forget(c);
    c->buf[kMorphList] = fresh.keep(list); c->buf[kMorphRows] = fresh.keep(rows); c->buf[kMorphTargets] = fresh.keep(tg);
    c->buf[kMorphDeltas] = fresh.keep(dl); c->buf[kMorphRest] = fresh.keep(rest); c->buf[kMorphSkinRow] = fresh.keep(srow);
    c->buf[kMorphWeights] = fresh.keep(wts);
    c->morph_list = listed;
    c->morph_lo = lo; c->morph_hi = hi;
    c->morph.present = 1u; c->morph.n_targets = n_targets; c->morph.n_morphed = n; c->morph.n_records = nr; c->morph.n_in_skin = in_skin;
    c->morph.first_bad = kNone;
    return PTMI_OK;
}

int ptmi_pose_morph(ptmi_ctx *c, const float *weights, uint32_t n_targets) {
    if (!c) return PTMI_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = pt_check_morph_pose(c, weights, n_targets, c->err);
    if (rc) return rc;
    uint32_t *head = head_of(c);
    auto stage = [&]() -> int {
        HIP_TRY(c, hipMemsetAsync(head, 0xFF, kPoseHeadBytes, c->stream));  // "none" in the check word
        HIP_TRY(c, hipMemcpy(reinterpret_cast<char *>(head) + kPoseHeadBytes, weights, (size_t)n_targets * sizeof(float), hipMemcpyHostToDevice));
        return PTMI_OK;
    };
    auto pass = [&](bool write) { return write ? run_pass<true>(c) : run_pass<false>(c); };
    PoseCall p{stage, pass};
    p.check_word = head; p.first_bad = &c->morph.first_bad; p.how = "morphed";
    p.refit = c->morph.n_in_skin < c->morph.n_morphed;             // an entry goes to a live record
    if (p.refit) { p.lo = c->morph_lo; p.hi = c->morph_hi; }       // from the lowest to the highest triangle whose live record is written
    if ((rc = pose_refusable(c, t0, p))) return rc;
    uint32_t active = 0u;
    for (uint32_t i = 0; i < n_targets; i++) active += weights[i] != 0.0f;
    c->morph.poses++; c->morph.active_targets = active; c->morph.first_bad = kNone;
    if (c->morph.n_in_skin) c->morph.skin_stale = 1u;              // until the next ptmi_pose_skin carries those rows to the live records
    c->morph.pose_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PTMI_OK;
}

int ptmi_morph_status(ptmi_ctx *c, struct ptmi_morph_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->morph;
    return PTMI_OK;
}

}  // extern "C"
