// dispatch.hip — the wavefront dispatch loop behind ptmi_dispatch and ptmi_dispatch_adaptive, ptmi_reproject, and what they leave for
// later calls to pick up: event pairs that become the timing statistics, and the dispatches in flight that ptmi_throttle bounds.
//
// Replaces the reference's dispatch (src/renderer/renderer.ts: updateCamera + dispatch :403-431).
#include "ptmi_ctx.h"
#include "scene/frame_scissor.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

namespace {

constexpr size_t kMaxPendingEvents = 4096;        // a caller that never synchronises (a preview loop) must not grow the list without bound
constexpr size_t kMaxDispatchesInFlight = 256;     // a caller that never throttles or synchronises still cannot queue without bound

// the statistics an event pair of each kind adds to: its time, and where there is one its launch count
const struct { double ptmi_stats::*ms; uint64_t ptmi_stats::*launches; } kEventStat[kEventKinds] = {
    {&ptmi_stats::gpu_ms, nullptr},                                  // kDispatch
    {&ptmi_stats::extend_ms, &ptmi_stats::extend_launches},          // kExtend
    {&ptmi_stats::shade_ms, &ptmi_stats::shade_launches},            // kShade
    {&ptmi_stats::shadow_ms, &ptmi_stats::shadow_launches},          // kShadow
    {&ptmi_stats::raygen_ms, nullptr},                               // kRaygen
    {&ptmi_stats::compact_ms, nullptr},                              // kCompact
    {&ptmi_stats::accumulate_ms, nullptr},                           // kAccumulate
};

hipEvent_t get_event(ptmi_ctx *c) {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}

}  // namespace

PT_HOST {

// resolve finished event pairs into the statistics (stream must be synchronised)
void drain_events(ptmi_ctx *c) {
    for (auto &p : c->pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->st.*kEventStat[p.kind].ms += ms;
            if (kEventStat[p.kind].launches) (c->st.*kEventStat[p.kind].launches)++;
        }
        c->event_pool.push_back(p.a); c->event_pool.push_back(p.b);
    }
    c->pending.clear();
}

// wait for everything in flight, then resolve its event pairs: what a call does before it reads what dispatches wrote
hipError_t quiesce(ptmi_ctx *c) {
    const hipError_t e = sync_all(c);
    if (e == hipSuccess) drain_events(c);
    return e;
}

}  // namespace pt_host

namespace {

// without a synchronisation: resolve the pairs at the front of the list whose closing event has completed
void drain_completed_events(ptmi_ctx *c) {
    size_t n = 0;
    while (n < c->pending.size() && hipEventQuery(c->pending[n].b) == hipSuccess) n++;
    if (n == 0) return;
    std::vector<EventPair> rest(c->pending.begin() + n, c->pending.end());
    c->pending.resize(n);
    drain_events(c);
    c->pending = std::move(rest);
}

// drop the finished dispatches from the front of the list, then wait for the oldest ones until at most `max` are left
hipError_t throttle(ptmi_ctx *c, size_t max) {
    while (!c->in_flight.empty() && hipEventQuery(c->in_flight.front()) == hipSuccess) {
        c->event_pool.push_back(c->in_flight.front()); c->in_flight.pop_front();
    }
    (void)hipGetLastError();                          // hipErrorNotReady of the query is not an error
    while (c->in_flight.size() > max) {
        hipError_t e = hipEventSynchronize(c->in_flight.front());
        if (e != hipSuccess) return e;
        c->event_pool.push_back(c->in_flight.front()); c->in_flight.pop_front();
    }
    return hipSuccess;
}

struct Timed {
    ptmi_ctx *c; hipEvent_t a = nullptr, b = nullptr; EventKind kind; bool on;
    hipStream_t st;
    Timed(ptmi_ctx *c_, EventKind kind_, bool on_, hipStream_t st_ = nullptr) : c(c_), kind(kind_), on(on_), st(st_ ? st_ : c_->stream) {
        if (on) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, st); }
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(b, st);
        c->pending.push_back({a, b, kind});
        if (c->pending.size() > kMaxPendingEvents) drain_completed_events(c);
    }
};

// The frame scissor of a dispatch: the part of the band whose pixels have a camera ray that can meet the scene's root
// box. A path of any other pixel misses at bounce 0 and ends with radiance 0, so while nothing can see a miss — no environment, no
// medium, no first-hit or moments plane, no alpha table — a plain dispatch traces the pixels inside only (ScissoredPixels) and folds
// zeros for the rest. Leaves the verdict in c->scissor; true: applied, with the band-local rows [l0, l1) and the columns [x0, x1).
struct ScissorRect { uint32_t l0, l1, x0, x1; };
bool frame_scissor(ptmi_ctx *c, const ptmi_camera *cam, uint32_t proj, const DevBand &band, bool plain, ScissorRect &r) {
    struct ptmi_scissor_status &st = c->scissor;
    st.x0 = 0u; st.x1 = c->W; st.y0 = 0u; st.y1 = c->H; st.applied = 0u;
    const auto no = [&](uint32_t reason) { st.reason = reason; return false; };
    if (!c->scissor_on) return no(PTMI_SCISSOR_OFF);
    if (!plain) return no(PTMI_SCISSOR_NOT_PLAIN);
    if (c->sc.env.tab) return no(PTMI_SCISSOR_ENVIRONMENT);
    if (c->sc.med.on) return no(PTMI_SCISSOR_MEDIUM);
    if (c->aov_mask) return no(PTMI_SCISSOR_AOV);
    if (c->plane[kMoments]) return no(PTMI_SCISSOR_MOMENTS);
    if (alpha_active(c)) return no(PTMI_SCISSOR_ALPHA);
    if (proj != PTMI_PROJ_PERSPECTIVE) return no(PTMI_SCISSOR_PROJECTION);
    if (c->sc.root_ref == PT_REF_NONE) return no(PTMI_SCISSOR_NO_PROMISE);
    // the box a ray has to meet before it meets anything: the walked tree's (padded) root and the uploaded tree's, which irregular rays walk
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        lo[k] = std::min(c->sc.root_min[k], c->sc.ref_root_min[k]);
        hi[k] = std::max(c->sc.root_max[k], c->sc.ref_root_max[k]);
    }
    ptmi_camera pin = *cam;
    ptmi_camera_set_projection(&pin, PTMI_PROJ_PERSPECTIVE, 0.0f);      // (the words are unread while the context's switch is off)
    const int why = pt_frame_scissor(&pin, lo, hi, &st.x0, &st.x1, &st.y0, &st.y1);
    if (why != PT_SCISSOR_RECT) return no(why == PT_SCISSOR_PROJECTION ? PTMI_SCISSOR_PROJECTION : PTMI_SCISSOR_NO_PROMISE);
    // row_of is increasing: the band's rows inside [y0, y1) are one range of local rows
    r.l0 = 0u;
    while (r.l0 < band.rows && band.row_of(r.l0) < st.y0) r.l0++;
    r.l1 = r.l0;
    while (r.l1 < band.rows && band.row_of(r.l1) < st.y1) r.l1++;
    r.x0 = st.x0; r.x1 = st.x1;
    if (r.l0 == 0u && r.l1 == band.rows && r.x0 == 0u && r.x1 == band.width) return no(PTMI_SCISSOR_NOTHING);
    st.reason = PTMI_SCISSOR_APPLIED; st.applied = 1u;
    return true;
}

#ifndef PT_REPACK
#define PT_REPACK 1          /* A/B switch: 0 leaves the path state at the path id for every bounce (no tail arrays in use) */
#endif

// ptmi_dispatch (ap NULL: n_frames frames of every pixel of the band, from cam->frame_index) and ptmi_dispatch_adaptive (ap: `rounds`
// rounds of ap->step frames for the listed pixels, each from its own count). Both run the same bounce loop per batch; they differ in
// the raygen in front of it and the folds behind it.
// map (with ap; ptmi_multi_dispatch_adaptive): the round selects from the whole-frame flag map and never restarts (pt_adaptive_flags
// has); count_call = false: a further round of one call, which ptmi_stats.dispatches has already counted.
// listed (ptmi_dispatch_bake and ptmi_dispatch_probes, which have checked it: bake_check, probes_check; no camera, no ap): n_frames
// frames of every texel of listed->list, from listed->first_frame: listed->rays is the batch's ray source and the list is the batch's
// pixels (a bake: the surface and its covered texels; probes: the probe records and the texels of the enabled probes' tiles; with
// listed->depth_max > 0 shade(0) leaves its first-hit records as it does for the first-hit planes, for the depth plane's fold).
int dispatch(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n_frames, const ptmi_adaptive_params *ap, uint32_t rounds,
             const DevFlagMap *map = nullptr, bool count_call = true, const ListedRays *listed = nullptr) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    uint32_t proj = PTMI_PROJ_PERSPECTIVE;
    if (!listed) {
        if (!cam) return fail(c, PTMI_E_INVALID, "camera is NULL");
        if (cam->width != c->W || cam->height != c->H)
            return fail(c, PTMI_E_INVALID, "camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
        if ((rc = pt_check_camera(c, cam, &proj, c->err))) return rc;
    }
    if (n_frames == 0 || (ap && rounds == 0) || (listed && listed->count == 0u)) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (ap && (rc = make_planes(c, group_set(kByAdaptive), (size_t)c->W * c->H, c->plane))) return rc;
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    if (band.y0 >= band.y1) return fail(c, PTMI_E_INVALID, "tile rows [%u,%u) outside the %u-row frame", band.y0, band.y1, c->H);
    if (band.rows == 0) return PTMI_OK;                         // more parts than strips: nothing to render here
    const uint64_t npix = listed ? listed->count : (uint64_t)band.rows * band.width;
    const uint32_t first_frame = listed ? listed->first_frame : cam->frame_index;
    uint32_t F = c->opt.frames_per_batch;
    // ~128 Mi paths, ~23 GB of state: the last bounces' small queues cost a fixed time per batch, so fewer, larger batches
    // (measured at 1080p, Msamples/s: 32 frames 8 920, 64 frames 9 150 - 9 275, 128 frames 9 270 - 9 310, when that time was ~3 ms.
    // About 1.2 ms of it, 0.15 ms per launch of `shade`, were the per-wave atomics of its statistics, which the compaction now sums:
    // a launch of `shade` on a queue of no segments takes ~0.05 ms, not ~0.2; profiles/README.md, "Shade's statistics in the compaction")
    const bool auto_F = F == 0;
    const bool depth = listed && listed->depth_max > 0.0f;      // a probe dispatch that folds the depth plane: it keeps the first-hit records
    Lane &ln = c->lane;
    if (auto_F) {
        F = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, (128ull << 20) / npix));
        // ... but never more than the device has room for: several contexts may share one device (ranks rehearsed on one GPU, a
        // Node host beside another process), and eight ranks of one node each size their batch by what THEIR device has free.
        // Room = free memory + what this context already holds, less a tenth for the rest (spill areas, blit staging).
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t held = (uint64_t)ln.cap * bytes_per_path(ln.aov != nullptr, ln.paths.W != nullptr, ln.alpha.RO != nullptr);
            const uint64_t room = (uint64_t)((double)(free_b + held) * 0.9);
            F = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(F, room / (npix * bytes_per_path(c->aov_mask != 0 || depth, c->sc.env.sampled != 0, alpha_active(c)))));
        }
    }
    F = std::min(F, n_frames);
    const bool env_w = c->sc.env.sampled != 0;                  // a sampled environment is one more light, and bounce rays carry its weight
    const bool nee = c->opt.do_mis && (c->sc.n_lights > 0 || env_w);
    // overlap: `shadow` of bounce b on a side stream, beside extend / shade of bounce b + 1. It is then the only kernel that
    // adds to L (emissive hits leave a record too, ShadeParams::emit_records), bounce after bounce on one stream, so every
    // path's sum is formed in the same order as without it. Record buffers alternate by bounce parity; shade(b) waits for
    // shadow(b - 2), the end of the batch for the last one.
    // While an alpha cutoff table is active (alpha.hip) the shadow stage is `extend` plus a resolve loop on the bounce loop's stream,
    // sharing its scratch arrays with the path loop: the one-stream schedule, whatever the option says.
    const bool alpha = alpha_active(c);
    const bool side = nee && c->opt.overlap != 0 && !alpha;
    if (npix * F > 0xFFFFFF00ull) return fail(c, PTMI_E_UNSUPPORTED, "batch of %llu paths exceeds 2^32", (unsigned long long)(npix * F));
    TraverseConfig cfg, cfg_shadow;
    if ((rc = traverse_pick(c, true, cfg)) || (rc = traverse_pick(c, false, cfg_shadow))) return rc;      // refused before anything is made
    for (;;) {
        rc = ensure_capacity(c, ln, (size_t)(npix * F), depth);
        if (rc == PTMI_OK) break;
        // out of device memory with a batch size the library chose: halve it and try again (hipMemGetInfo is a snapshot; another
        // context may have allocated since). A size the caller asked for fails loudly.
        if (!auto_F || !c->alloc_oom || F <= 1) return rc;
        F = (F + 1) / 2;
    }
    if ((rc = traverse_arm(c, true, kSpillMain, cfg, true)) || (rc = traverse_arm(c, false, side ? kSpillSide : kSpillAfterExtend, cfg_shadow, true)))
        return rc;
    c->st.traversal_used = pt_variant(cfg.variant).where == PT_FROM_MEMORY ? PTMI_TRAVERSAL_GLOBAL : PTMI_TRAVERSAL_LDS;
    c->st.frames_per_batch_used = F;
    c->st.radiance_stride_bytes = (walks_memory_quantised(cfg) || walks_memory_quantised(cfg_shadow)) ? 16u : 12u;
    c->st.shade_tables = PT_SHADE_LDS_BUDGET | ((uint32_t)pt_shade_stage(c->sc.n_mats, c->sc.n_lights) << 28);
    // (the batch size and the capacity above are the whole band's, scissor or not: frames_per_batch_used and the memory stay what they were)
    ScissorRect sr{};
    const bool scissored = frame_scissor(c, cam, proj, band, !ap && !listed, sr);
    const uint64_t skipped_px = scissored ? npix - (uint64_t)(sr.l1 - sr.l0) * (sr.x1 - sr.x0) : 0u;
    const int blocks = c->n_cu * 8;
#ifndef PT_SHADE_WGS_PER_CU
#define PT_SHADE_WGS_PER_CU 16
#endif
    // 256-thread workgroups of the grid-stride shade kernel. Config 1, five interleaved runs each (Msamples/s): 8 per CU 9 247,
    // 16: 9 362, 32: 9 303, 64: 8 929 (run-to-run +-130); config 3 +-0.
    const int shade_blocks = c->n_cu * PT_SHADE_WGS_PER_CU;
    const uint32_t maxb = c->opt.max_bounces;
    const bool t1 = c->opt.timing >= 1, t2 = c->opt.timing >= 2, t3 = c->opt.timing >= 3;
    {
        Timed td(c, kDispatch, t1);
        const hipStream_t ms = c->stream;                                         // the bounce loop's stream
        const hipStream_t ss = side ? ln.side : ms;                               // ... and the shadow kernels'
        const int tiles = (int)(ln.cap / pt_compact_tile_slots() + 1);
        ln.paths.l_stride = c->st.radiance_stride_bytes / 4u;
        DevPaths bp = ln.paths;
        if (!env_w) bp.W = nullptr;                             // (the arrays of an earlier, sampled environment may still be there)
        // Once per batch, after the compaction of the first bounce that plays roulette, the survivors' O / D / C are gathered into the
        // tail arrays at their queue positions: from then on a few percent of the paths are alive, and state left at the path id costs
        // them a line per lane in each stream. From the next bounce on, extend and shade find the state at the slot the queue names
        // and shade writes it back there; the radiance and the records keep the path id (ln.pid).
        const uint32_t rb = PT_REPACK ? pt_repack_bounce() : 0xFFFFFFFEu;
        DevPaths tp = ln.tail;
        tp.L = bp.L; tp.l_stride = bp.l_stride;
        if (!env_w) tp.W = nullptr;
        float4 *const aov_rec = c->aov_mask || depth ? ln.aov : nullptr;      // written by shade(0), read by the folds after the last bounce
        float4 *const mom = plane_as<float4>(c, kMoments);
        unsigned long long *const ct = c->d_counters;
        uint32_t *const qlen = &c->d_control[kCwQueue], *const slen = &c->d_control[kCwShadow];    // queue lengths by bounce; shadow, by parity
        if (ap && !map && first_frame == 0u) { pt_launch_adaptive_restart(ms, blocks, band, mom); c->ad_rounds = 0; }
        const DevRays rays = listed ? listed->rays : DevRays{CameraSource{cam, proj}};
        // a batch: fb frames of every pixel (listed: listed texel) from frame0 on, or (ap) of every listed pixel from its own count on
        auto batch = [&](uint32_t frame0, uint32_t fb) -> int {
            const DevPixels px = ap     ? DevPixels{ListedPixels{band, c->ad.list, &c->d_control[kCwAdActive], mom, &ct[kCtAdTraced]}}
                                 : listed ? DevPixels{BakedPixels{band, listed->list, listed->count, frame0}}
                                 : scissored ? DevPixels{ScissoredPixels{band, sr.l0, sr.l1, sr.x0, sr.x1, frame0, ct}}
                                          : DevPixels{DensePixels{band, frame0}};
            { Timed t(c, kRaygen, t3, ms); pt_launch_raygen(ms, blocks, rays, px, fb, bp, &qlen[0]); }
            int cur = 0;
            for (uint32_t b = 0; b < maxb; b++) {
                const bool tail = b > rb;                                   // the state is in the tail arrays
                const uint32_t *q = b == 0 || b == rb + 1 ? nullptr : ln.queue[cur];   // bounce 0 / after the repack: slot i holds path / state i
                const DevPaths sp = tail ? tp : bp;
                const int par = side ? (int)(b & 1u) : 0;
                const ShadeParams shp{b, maxb, c->opt.do_mis, ln.counts, side ? 1u : 0u, tail ? ln.pid : nullptr};
                { Timed t(c, kExtend, t2, ms); launch_extend(c, ms, cfg, sp, q, &qlen[b], ln.hits);
                  if (alpha) alpha_resolve_paths(c, ms, cfg, sp, q, &qlen[b], ln.hits, nullptr); }
                const bool last = b + 1 == maxb;
                if (side && b >= 2) HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[par], 0));      // its records are read
                { Timed t(c, kShade, t3, ms);
                  (c->opt.perf_mode ? pt_launch_shade_fast : pt_launch_shade)(
                      ms, shade_blocks, c->sc, sp, q, &qlen[b], ln.hits, ln.sh[par], ln.alive, ln.shadowm, shp,
                      b == 0 ? aov_rec : nullptr); }
                { Timed t(c, kCompact, t3, ms);
                  pt_launch_compact(ms, tiles, q, &qlen[b], ln.alive, nee ? ln.shadowm : nullptr, ln.counts,
                                    ln.word_off, ln.queue[cur ^ 1], &qlen[b + 1], ln.sq[par], &slen[par],
                                    ct, b, last ? 0 : 1);
                  if (b == rb && !last) pt_launch_repack(ms, blocks, &qlen[b + 1], ln.queue[cur ^ 1], bp, tp, ln.pid); }
                if (side) {
                    HIP_TRY(c, hipEventRecord(ln.ev_ready, ms));
                    HIP_TRY(c, hipStreamWaitEvent(ss, ln.ev_ready, 0));
                    { Timed t(c, kShadow, t3, ss); launch_shadow(c, ss, cfg_shadow, bp, ln.sh[par], ln.sq[par], &slen[par], nullptr); }
                    HIP_TRY(c, hipEventRecord(ln.ev_shadow[par], ss));
                } else if (nee) {
                    Timed t(c, kShadow, t3, ms);
                    if (alpha) alpha_shadow_stage(c, ms, cfg, bp, ln.sh[0], ln.sq[0], &slen[0], ln.hits, nullptr, nullptr);   // (shade is done with the hits)
                    else launch_shadow(c, ms, cfg_shadow, bp, ln.sh[0], ln.sq[0], &slen[0], nullptr);
                }
                cur ^= 1;
            }
            // all additions to L are in before it is folded
            if (side) {
                HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[(maxb - 1) & 1u], 0));
                if (maxb >= 2) HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[maxb & 1u], 0));
            }
            Timed t(c, kAccumulate, t3, ms);
            pt_launch_accumulate(ms, blocks, px, fb, bp.L, bp.l_stride, c->d_out);
            if (depth) pt_launch_accumulate_probe_depth(ms, blocks, px, fb, aov_rec, listed->depth_max, plane_as<float4>(c, kProbeDepth));
            if (c->aov_mask)
                pt_launch_accumulate_aov(ms, blocks, px, fb, aov_rec, c->sc.tris, c->sc.n_tris, plane_as<float4>(c, kAovAlbedo),
                                         plane_as<float4>(c, kAovNormal), plane_as<uint2>(c, kAovId));
            // the moments fold goes last: it moves mom.z on, where the other two read the listed pixels' counts. An adaptive dispatch
            // always has the plane (it is refused without); a plain one folds it only while it is on.
            if (ap || mom) pt_launch_accumulate_moments(ms, blocks, px, fb, bp.L, bp.l_stride, mom);
            return PTMI_OK;
        };
        if (ap) {
            for (uint32_t r = 0; r < rounds; r++) {
                pt_launch_adaptive_list(ms, blocks, band, *ap, mom, map, c->ad);
                for (uint32_t f0 = 0; f0 < n_frames; f0 += F)
                    if ((rc = batch(0u, std::min(F, n_frames - f0)))) return rc;
            }
            c->ad_rounds += rounds;
        } else {
            for (uint32_t f0 = 0; f0 < n_frames; f0 += F)
                if ((rc = batch(first_frame + f0, std::min(F, n_frames - f0)))) return rc;
        }
    }
    HIP_TRY(c, hipGetLastError());
    {   // the end of this dispatch on the context's stream (the fold of its last batch): what ptmi_throttle waits for
        hipEvent_t done = get_event(c);
        HIP_TRY(c, hipEventRecord(done, c->stream));
        c->in_flight.push_back(done);
        if (c->in_flight.size() > kMaxDispatchesInFlight) HIP_TRY(c, throttle(c, kMaxDispatchesInFlight));
    }
    if (!ap) { c->st.paths += npix * n_frames; c->st.frames += n_frames; }      // adaptive: counted on the device (kCtAdTraced)
    c->scissor.skipped += skipped_px * n_frames;
    if (count_call) c->st.dispatches += 1;
    return PTMI_OK;
}

}  // namespace

int pt_adaptive_check(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *params, ptmi_adaptive_params *out) {
    if (!c) return PTMI_E_INVALID;
    if (!params) return fail(c, PTMI_E_INVALID, "params is NULL");
    ptmi_adaptive_params ap = *params;
    if (!(ap.threshold > 0.0f)) return fail(c, PTMI_E_INVALID, "threshold %g is not > 0", (double)ap.threshold);
    if (!(ap.floor >= 0.0f) || std::isinf(ap.floor)) return fail(c, PTMI_E_INVALID, "floor %g is negative or not finite", (double)ap.floor);
    if (ap.reserved[0] || ap.reserved[1]) return fail(c, PTMI_E_INVALID, "a reserved word of ptmi_adaptive_params is not zero");
    if (ap.neighbourhood > 1u) return fail(c, PTMI_E_INVALID, "neighbourhood %u is not 0 or 1", ap.neighbourhood);
    if (ap.floor == 0.0f) ap.floor = 1.0f;
    if (ap.min_frames == 0u) ap.min_frames = 16u;
    if (ap.max_frames == 0u) ap.max_frames = 4096u;
    if (ap.step == 0u) ap.step = 16u;
    if (ap.max_frames > (1u << 24)) return fail(c, PTMI_E_INVALID, "max_frames %u above 2^24", ap.max_frames);
    if (ap.min_frames > ap.max_frames) return fail(c, PTMI_E_INVALID, "min_frames %u above max_frames %u", ap.min_frames, ap.max_frames);
    if (ap.step > (1u << 16)) return fail(c, PTMI_E_INVALID, "step %u above 2^16", ap.step);
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!c->moments_on || !c->plane[kMoments]) return fail(c, PTMI_E_STATE, "adaptive sampling needs the moments plane (ptmi_set_moments)");
    if (!cam) return fail(c, PTMI_E_INVALID, "camera is NULL");
    if (cam->width != c->W || cam->height != c->H)
        return fail(c, PTMI_E_INVALID, "camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
    uint32_t proj;
    if ((rc = pt_check_camera(c, cam, &proj, c->err))) return rc;
    *out = ap;
    return PTMI_OK;
}

int pt_adaptive_flags(ptmi_ctx *c, const ptmi_adaptive_params *ap, bool restart, uint8_t **share_out) {
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = make_planes(c, group_set(kByAdaptive), (size_t)c->W * c->H, c->plane);
    if (rc) return rc;
    *share_out = plane_as<uint8_t>(c, kAdFlags);
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    if (band.y0 >= band.y1 || band.rows == 0) return PTMI_OK;           // more parts than strips: no pixel of this context's
    float4 *const mom = plane_as<float4>(c, kMoments);
    if (restart) { pt_launch_adaptive_restart(c->stream, c->n_cu * 8, band, mom); c->ad_rounds = 0; }
    pt_launch_adaptive_flags(c->stream, c->n_cu * 8, band, *ap, mom, *share_out);
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int pt_adaptive_round(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *ap, const uint8_t *map, uint32_t share_px,
                      bool count_call) {
    const DevFlagMap fm{map, share_px, c->W, std::max(1u, c->opt.tile_strip), std::max(1u, c->opt.tile_parts)};
    return dispatch(c, cam, ap->step, ap, 1, &fm, count_call);
}

extern "C" {

int ptmi_dispatch(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n_frames) { return dispatch(c, cam, n_frames, nullptr, 0); }

int ptmi_dispatch_adaptive(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *params, uint32_t rounds) {
    ptmi_adaptive_params ap;
    const int rc = pt_adaptive_check(c, cam, params, &ap);
    if (rc) return rc;
    return dispatch(c, cam, ap.step, &ap, rounds);
}

int ptmi_dispatch_bake(ptmi_ctx *c, const ptmi_bake_params *params, uint32_t n_frames) {
    ptmi_bake_params bp;
    const int rc = bake_check(c, params, &bp);
    if (rc) return rc;
    const ListedRays listed{BakeSurface{c->d_bake_texels, bp.bias}, c->d_bake_covered, c->bake_covered, bp.first_frame};
    return dispatch(c, nullptr, n_frames, nullptr, 0, nullptr, true, &listed);
}

int ptmi_dispatch_probes(ptmi_ctx *c, const ptmi_probe_params *params, uint32_t n_frames) {
    ListedRays listed;
    const int rc = probes_check(c, params, &listed);
    if (rc) return rc;
    return dispatch(c, nullptr, n_frames, nullptr, 0, nullptr, true, &listed);
}

int ptmi_scissor_status(ptmi_ctx *c, struct ptmi_scissor_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->scissor;
    return PTMI_OK;
}

int ptmi_adaptive_status(ptmi_ctx *c, struct ptmi_adaptive_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    if (!c->moments_on) return fail(c, PTMI_E_STATE, "the moments plane is off (ptmi_set_moments)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    HIP_TRY(c, hipSetDevice(c->device));
    std::memset(out, 0, sizeof *out);
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    const unsigned long long preset[3] = {0ull, ~0ull, 0ull};
    unsigned long long sum_min_max[3] = {0ull, 0ull, 0ull};
    uint32_t active = 0u;
    HIP_TRY(c, quiesce(c));
    if (band.y0 < band.y1 && band.rows) {
        HIP_TRY(c, hipMemcpyAsync(&c->d_counters[kCtAdSum], preset, sizeof preset, hipMemcpyHostToDevice, c->stream));
        pt_launch_adaptive_status(c->stream, c->n_cu * 8, band, plane_as<float4>(c, kMoments), c->ad);
        HIP_TRY(c, hipMemcpyAsync(sum_min_max, &c->d_counters[kCtAdSum], sizeof sum_min_max, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(&active, &c->d_control[kCwAdActive], sizeof active, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->active = active;
    out->samples = sum_min_max[0];
    out->min_count = sum_min_max[1] == ~0ull ? 0u : (uint32_t)sum_min_max[1];
    out->max_count = (uint32_t)sum_min_max[2];
    out->rounds = c->ad_rounds;
    return PTMI_OK;
}

// The snapshot is a copy of whole planes (rows of other contexts travel along and are never read); the centre rays and their hits use
// the batch arrays of a dispatch, like the per-stage entry points. Everything that can fail comes before the first write.
int ptmi_reproject(ptmi_ctx *c, const ptmi_camera *from, const ptmi_camera *to, const ptmi_reproject_params *params) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!from || !to) return fail(c, PTMI_E_INVALID, "a camera is NULL");
    for (const ptmi_camera *cam : {from, to})
        if (cam->width != c->W || cam->height != c->H)
            return fail(c, PTMI_E_INVALID, "a camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
    uint32_t from_proj, to_proj;
    if ((rc = pt_check_camera(c, from, &from_proj, c->err)) || (rc = pt_check_camera(c, to, &to_proj, c->err))) return rc;
    if (from_proj == PTMI_PROJ_EQUIRECT || to_proj == PTMI_PROJ_EQUIRECT)
        return fail(c, PTMI_E_INVALID, "reprojection %s an equirectangular camera is not supported", from_proj == PTMI_PROJ_EQUIRECT ? "from" : "to");
    const ptmi_reproject_params zero = {};
    const ptmi_reproject_params &q = params ? *params : zero;
    if (!std::isfinite(q.depth_tolerance) || q.depth_tolerance < 0.0f)
        return fail(c, PTMI_E_INVALID, "depth_tolerance %g is negative or not finite", (double)q.depth_tolerance);
    if (q.max_history > (1u << 24)) return fail(c, PTMI_E_INVALID, "max_history %u above 2^24", q.max_history);
    if (q.match_ids > 2u) return fail(c, PTMI_E_INVALID, "unknown match_ids %u", q.match_ids);
    for (uint32_t r : q.reserved) if (r) return fail(c, PTMI_E_INVALID, "a reserved word of ptmi_reproject_params is not zero");
    if (!(c->aov_mask & PTMI_AOV_NORMAL) || !c->plane[kAovNormal])
        return fail(c, PTMI_E_STATE, "reprojection needs the NORMAL plane (ptmi_set_aovs)");
    if (!c->moments_on || !c->plane[kMoments]) return fail(c, PTMI_E_STATE, "reprojection needs the moments plane (ptmi_set_moments)");
    const bool have_albedo = (c->aov_mask & PTMI_AOV_ALBEDO) && c->plane[kAovAlbedo];
    const bool have_ids = (c->aov_mask & PTMI_AOV_ID) && c->plane[kAovId];
    if (q.match_ids == 2u && !have_ids) return fail(c, PTMI_E_STATE, "match_ids = 2 needs the ID plane (ptmi_set_aovs)");
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    if (band.y0 >= band.y1) return fail(c, PTMI_E_INVALID, "tile rows [%u,%u) outside the %u-row frame", band.y0, band.y1, c->H);
    if ((band.rows + 3u) / 4u > 65535u) return fail(c, PTMI_E_UNSUPPORTED, "more than 262140 rows");
    TraverseConfig cfg;
    if ((rc = traverse_pick(c, true, cfg))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->W * c->H;
    const uint32_t history = bit(kRpOut) | bit(kRpMoments) | bit(kRpNormal) | (have_albedo ? bit(kRpAlbedo) : 0u) | (have_ids ? bit(kRpId) : 0u);
    if ((rc = make_planes(c, history, npix, c->plane))) return rc;
    Lane &ln = c->lane;
    if (band.rows && (rc = ensure_capacity(c, ln, (size_t)band.rows * band.width))) return rc;
    if ((rc = traverse_arm(c, true, kSpillMain, cfg, false))) return rc;      // (the statistics keep the variants of the last dispatch)
    const hipStream_t s = c->stream;
    static_assert(kCtRpMovedCarried == kCtRpCarried + 5, "the four words of the status and the two of the motion status, zeroed as one");
    HIP_TRY(c, hipMemsetAsync(&c->d_counters[kCtRpCarried], 0, 6 * sizeof(unsigned long long), s));
    if (band.rows == 0) return PTMI_OK;                         // more parts than strips: no pixel of this context's
    const struct { FramePlane to; const void *from; bool on; } copies[] = {
        {kRpOut, c->d_out, true}, {kRpMoments, c->plane[kMoments], true}, {kRpNormal, c->plane[kAovNormal], true},
        {kRpAlbedo, c->plane[kAovAlbedo], have_albedo}, {kRpId, c->plane[kAovId], have_ids}};
    for (const auto &cp : copies)
        if (cp.on) HIP_TRY(c, hipMemcpyAsync(c->plane[cp.to], cp.from, plane_bytes(cp.to, npix), hipMemcpyDeviceToDevice, s));
    const int blocks = c->n_cu * 8;
    pt_launch_center_rays(s, blocks, *to, to_proj, band, ln.paths, &c->d_control[kCwQueue]);
    launch_extend(c, s, cfg, ln.paths, nullptr, &c->d_control[kCwQueue], ln.hits);
    // the first surface that is there, as the first-hit planes recorded it: without this every pixel seen through a hole is disoccluded
    if (alpha_active(c)) alpha_resolve_paths(c, s, cfg, ln.paths, nullptr, &c->d_control[kCwQueue], ln.hits, nullptr);
    ReprojectArgs a{};
    a.from = *from; a.from_proj = from_proj; a.band = band;
    a.max_history = q.max_history ? q.max_history : 32u;
    a.depth_tolerance = q.depth_tolerance > 0.0f ? q.depth_tolerance : 0.02f;
    a.match_ids = q.match_ids == 2u || (q.match_ids == 0u && have_ids) ? 1u : 0u;
    a.O = ln.paths.O; a.D = ln.paths.D; a.hits = ln.hits;
    a.tris = c->sc.tris; a.n_tris = c->sc.n_tris;
    a.h_out = plane_as<float4>(c, kRpOut); a.h_mom = plane_as<float4>(c, kRpMoments); a.h_normal = plane_as<float4>(c, kRpNormal);
    a.h_albedo = have_albedo ? plane_as<float4>(c, kRpAlbedo) : nullptr; a.h_ids = have_ids ? plane_as<uint2>(c, kRpId) : nullptr;
    a.out = c->d_out; a.mom = plane_as<float4>(c, kMoments); a.normal = plane_as<float4>(c, kAovNormal);
    a.albedo = have_albedo ? plane_as<float4>(c, kAovAlbedo) : nullptr; a.ids = have_ids ? plane_as<uint2>(c, kAovId) : nullptr;
    a.status = c->d_counters;
    const bool motion = c->motion_on && c->plane[kMotion] && c->buf[kMotionPrev];
    if (motion) {
        // (u, v) of the resolved hits on the centre rays, as ptmi_debug_intersect reports them, into the batch's C array
        pt_launch_hit_uv(s, band.rows * band.width, c->sc, ln.paths, ln.hits, ln.paths.C);
        a.prev = static_cast<const float4 *>(c->buf[kMotionPrev]); a.uv = ln.paths.C;
        a.dirty_first = c->motion_dirty_first; a.dirty_end = c->motion_dirty_first + c->motion_dirty_count;
        a.motion = plane_as<float4>(c, kMotion);
    }
    pt_launch_reproject(s, a);
    HIP_TRY(c, hipGetLastError());
    if (motion) return motion_commit(c);         // the history now holds the current geometry
    return PTMI_OK;
}

int ptmi_reproject_status(ptmi_ctx *c, struct ptmi_reproject_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    unsigned long long h[4];
    HIP_TRY(c, hipMemcpy(h, &c->d_counters[kCtRpCarried], sizeof h, hipMemcpyDeviceToHost));
    const auto word = [&](CounterWord w) { return h[w - kCtRpCarried]; };
    out->carried = word(kCtRpCarried); out->disoccluded = word(kCtRpDisoccluded);
    out->missed = word(kCtRpMissed); out->samples = word(kCtRpSamples);
    return PTMI_OK;
}

int ptmi_throttle(ptmi_ctx *c, uint32_t max_in_flight, uint32_t *in_flight) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, throttle(c, max_in_flight));
    if (in_flight) *in_flight = (uint32_t)c->in_flight.size();
    return PTMI_OK;
}

int ptmi_synchronize(ptmi_ctx *c) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, throttle(c, 0));
    return PTMI_OK;
}

}  // extern "C"
