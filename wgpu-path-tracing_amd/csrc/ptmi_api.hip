// ptmi_api.hip — the C ABI of include/ptmi.h: the context and its options, the frame planes and the batch arrays, output, atlas, AOV
// and moments planes, denoising, blit and statistics. (Upload: scene_image.hip; dispatch: dispatch.hip; ptmi_debug_*: debug_stages.hip.)
//
// Replaces the host side of the reference's compute pass (src/renderer/renderer.ts: createBuffers :242-355, createBindGroups :368-381).
#include "ptmi_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

void vfail(std::string &err, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    err = buf;
}

// what an element of each of the lane's arrays takes, in bytes: a path of the batch in the per-path arrays, then a word per 64 paths,
// then a compaction tile
constexpr size_t kLaneBytes[kLaneBufs] = {
    16, 16, 8, 16,                                 // kPathO .. kPathL
    8,                                             // kHits
    16 + 16 + sizeof(rgb_sc), 4, 16 + 16 + sizeof(rgb_sc), 4,      // kShadow0, kShadowIdx0, kShadow1, kShadowIdx1
    16, 16, 8, 4,                                  // kTailO .. kPid
    4, 4,                                          // kQueue0, kQueue1
    1,                                             // kOcc
    32,                                            // kAovRec
    4, 4,                                          // kPathW, kTailW
    16, 16, 4, 4, 8,                               // kAlphaO, kAlphaD, kAlphaList0, kAlphaList1, kAlphaHits
    8, 8, 4,                                       // kAliveMask, kShadowMask, kShadeCounts: per 64 paths
    4 * 4,                                         // kTileSums: four totals per tile
};
// elements of array k in a batch of `cap` paths
size_t lane_elements(int k, size_t cap) {
    return k < kLanePerPath ? cap : k == kTileSums ? cap / pt_compact_tile_slots() + 2 : cap / 64 + 1;
}
// bytes of device memory a path of a batch takes in ensure_capacity: the per-path arrays and one byte for the three arrays of words
// (20 B per 64 paths; the tile totals are 16 B per 65 536). The automatic batch size and its out-of-memory retry (ptmi_dispatch)
// rely on it.
// the arrays that exist only while something is on: the first-hit records (aov), the environment's weights (env_w), the alpha resolve
// loops' arrays (alpha)
constexpr bool lane_buf_wanted(int k, bool aov, bool env_w, bool alpha) {
    return k == kAovRec ? aov : k == kPathW || k == kTailW ? env_w : k >= kAlphaO && k <= kAlphaHits ? alpha : true;
}
constexpr size_t lane_bytes_per_path(bool aov, bool env_w, bool alpha) {
    size_t n = 1;
    for (int k = 0; k < kLanePerPath; k++) if (lane_buf_wanted(k, aov, env_w, alpha)) n += kLaneBytes[k];
    return n;
}
static_assert(lane_bytes_per_path(false, false, false) == 214 && lane_bytes_per_path(true, false, false) == 246 &&
              lane_bytes_per_path(false, true, false) == 222 && lane_bytes_per_path(false, false, true) == 262,
              "the automatic frames_per_batch moves with these");

}  // namespace

PT_HOST {
// the typed members that kernels receive, as views of Lane::buf
void lane_views(Lane &ln) {
    auto at = [&](int k, auto *&p) { view(p, ln.buf[k]); };
    at(kPathO, ln.paths.O); at(kPathD, ln.paths.D); at(kPathC, ln.paths.C); at(kPathL, ln.paths.L);
    at(kHits, ln.hits);
    for (int k = 0; k < 2; k++) {
        DevShadow &sh = ln.sh[k];
        at(k ? kShadow1 : kShadow0, sh.SO); at(k ? kShadowIdx1 : kShadowIdx0, ln.sq[k]); at(k ? kQueue1 : kQueue0, ln.queue[k]);
        sh.SD = sh.SO ? sh.SO + ln.cap : nullptr; sh.SC = sh.SO ? reinterpret_cast<rgb_sc *>(sh.SO + 2 * ln.cap) : nullptr;
        sh.cap = (uint32_t)ln.cap;
    }
    at(kTailO, ln.tail.O); at(kTailD, ln.tail.D); at(kTailC, ln.tail.C); at(kPid, ln.pid);
    at(kOcc, ln.d_occ); at(kAovRec, ln.aov);
    at(kPathW, ln.paths.W); at(kTailW, ln.tail.W);
    at(kAlphaO, ln.alpha.RO); at(kAlphaD, ln.alpha.RD); at(kAlphaList0, ln.alpha.list[0]); at(kAlphaList1, ln.alpha.list[1]);
    at(kAlphaHits, ln.alpha.hits);
    at(kAliveMask, ln.alive); at(kShadowMask, ln.shadowm); at(kShadeCounts, ln.counts); at(kTileSums, ln.word_off);
}
}  // namespace pt_host

namespace {

void free_batch(Lane &ln) {
    for (void *&p : ln.buf) dfree(p);
    ln.cap = 0;
    lane_views(ln);
}

// ptmi_stats.bvh_depth: levels of the uploaded tree, or of the hierarchy rebuilt over its leaves where that is deeper
uint32_t stats_depth(const ptmi_ctx *c) { return c->img.leaves_used == 2u ? c->img.ref_depth : std::max(c->img.depth, c->img.ref_depth); }

constexpr uint32_t kAovAll = PTMI_AOV_ALBEDO | PTMI_AOV_NORMAL | PTMI_AOV_ID;

// One row per FramePlane: its size for px pixels, whether it is zero-filled when made, and when it is made: with the frame (ptmi_resize
// and the call that turns it on), or by the first call that needs it since the last resize.
template <size_t K> size_t per_pixel(size_t px) { return px * K; }
size_t ballot_bytes(size_t px) { return (px / 64 + 1) * 8; }
size_t tile_sum_bytes(size_t px) { return (size_t)pt_adaptive_tiles((uint32_t)px) * 4; }
const struct { const char *name; size_t (*bytes)(size_t px); bool zeroed; PlaneGroup group; } kFrame[kFramePlanes] = {
    {"output", per_pixel<PTMI_OUTPUT_STRIDE>, true, kWithFrame},
    {"albedo", per_pixel<16>, true, kWithFrame}, {"normal", per_pixel<16>, true, kWithFrame}, {"id", per_pixel<8>, true, kWithFrame},
    {"moments", per_pixel<16>, true, kWithFrame},
    {"denoiser guide", per_pixel<16>, false, kByDenoise}, {"denoiser gradient", per_pixel<4>, false, kByDenoise},
    {"denoiser ping", per_pixel<16>, false, kByDenoise}, {"denoiser pong", per_pixel<16>, false, kByDenoise},
    {"denoised", per_pixel<16>, false, kByDenoise},
    {"adaptive ballot", ballot_bytes, false, kByAdaptive}, {"adaptive list", per_pixel<4>, false, kByAdaptive},
    {"adaptive tile sums", tile_sum_bytes, false, kByAdaptive}, {"adaptive flag share", per_pixel<1>, false, kByAdaptive},
    {"output history", per_pixel<PTMI_OUTPUT_STRIDE>, false, kByReproject}, {"moments history", per_pixel<16>, false, kByReproject},
    {"normal history", per_pixel<16>, false, kByReproject}, {"albedo history", per_pixel<16>, false, kByReproject},
    {"id history", per_pixel<8>, false, kByReproject},
    {"float canvas", per_pixel<16>, false, kByBlit}, {"8-bit canvas", per_pixel<4>, false, kByBlit},
    {"motion", per_pixel<16>, true, kWithFrame},
    {"dilate ping", per_pixel<16>, false, kByBake}, {"dilate pong", per_pixel<16>, false, kByBake},
    {"probe depth", per_pixel<16>, true, kWithFrame},
    {"lightmap guide (normal)", per_pixel<16>, false, kByBakeDenoise}, {"lightmap guide (position)", per_pixel<16>, false, kByBakeDenoise},
    {"denoised lightmap", per_pixel<16>, false, kByBakeDenoise},
};
// sets of planes: a bit per FramePlane
constexpr uint32_t kAllPlanes = (1u << kFramePlanes) - 1u;
static_assert(PTMI_AOV_ALBEDO << kAovAlbedo == bit(kAovAlbedo) && PTMI_AOV_NORMAL << kAovAlbedo == bit(kAovNormal) &&
              PTMI_AOV_ID << kAovAlbedo == bit(kAovId), "an AOV mask, shifted, is its set of planes");
// the planes that exist whenever the output buffer does: the output, the AOV planes of the mask, the moments, the motion and the probe
// depth plane while on
uint32_t frame_set(const ptmi_ctx *c) {
    return bit(kOut) | c->aov_mask << kAovAlbedo | (c->moments_on ? bit(kMoments) : 0u) | (c->motion_on ? bit(kMotion) : 0u) |
           (c->probe_depth_on ? bit(kProbeDepth) : 0u);
}
// which: one PTMI_AOV_* bit (else kFramePlanes)
FramePlane aov_plane_of(uint32_t which) {
    return which == PTMI_AOV_ALBEDO ? kAovAlbedo : which == PTMI_AOV_NORMAL ? kAovNormal : which == PTMI_AOV_ID ? kAovId : kFramePlanes;
}
void view_planes(ptmi_ctx *c) {
    view(c->ad.ballot, c->plane[kAdBallot]); view(c->ad.list, c->plane[kAdList]); view(c->ad.tile_sums, c->plane[kAdTileSums]);
}

// Frees the context's planes of `set` (the caller has synchronised where one may be in use).
void drop_planes(ptmi_ctx *c, uint32_t set) {
    for (int k = 0; k < kFramePlanes; k++) if (set & 1u << k) dfree(c->plane[k]);
    view_planes(c);
}

// a fresh moments plane (ptmi_resize, ptmi_set_moments): no round has listed anything in it
int reset_adaptive_rounds(ptmi_ctx *c) {
    static_assert(kCwAdActive == kCwAdPixels + 1, "the round's two words, zeroed as one");
    HIP_TRY(c, hipMemset(&c->d_control[kCwAdPixels], 0, 2 * sizeof(uint32_t)));
    c->ad_rounds = 0;
    return PTMI_OK;
}

}  // namespace

PT_HOST {

thread_local std::string g_create_err;

int fail(std::string &err, int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfail(err, fmt, ap); va_end(ap);
    return code;
}
int fail(const ptmi_ctx *c, int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfail(c ? c->err : g_create_err, fmt, ap); va_end(ap);
    return code;
}

int read_plane(ptmi_ctx *c, FramePlane k, const void *src, void *dst, size_t n, size_t unit) {
    const size_t bytes = kFrame[k].bytes((size_t)c->W * c->H);
    if (n * unit != bytes) return fail(c, PTMI_E_INVALID, "expected %zu %s, got %zu", bytes / unit, unit == 4 ? "floats" : "bytes", n);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

int atrous_params(ptmi_ctx *c, uint32_t iterations, const uint32_t (&reserved)[3], const char *of, float phi_color, float phi_normal,
                  float phi_geo, AtrousArgs *out) {
    if (iterations > 10u) return fail(c, PTMI_E_INVALID, "iterations = %u is above 10", iterations);
    if (reserved[0] || reserved[1] || reserved[2]) return fail(c, PTMI_E_INVALID, "a reserved word%s is not zero", of);
    for (float f : {phi_color, phi_normal, phi_geo})
        if (!std::isfinite(f) || f < 0.0f) return fail(c, PTMI_E_INVALID, "phi %g is negative or not finite", (double)f);
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    *out = AtrousArgs{c->W, c->H, iterations ? iterations : 5u, phi_color > 0.0f ? phi_color : 4.0f,
                      phi_normal > 0.0f ? phi_normal : 128.0f, phi_geo > 0.0f ? phi_geo : 1.0f};
    return PTMI_OK;
}

void default_options(ptmi_options &o) {
    std::memset(&o, 0, sizeof o);
    o.max_bounces = 8; o.do_mis = 1; o.cull = 1; o.traversal = PTMI_TRAVERSAL_AUTO; o.overlap = 2;
}

// everything the library has in flight, on every stream it owns
hipError_t sync_all(ptmi_ctx *c) {
    hipError_t e = c->stream ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (e == hipSuccess && c->lane.side) e = hipStreamSynchronize(c->lane.side);
    if (e == hipSuccess && c->stream) e = hipStreamSynchronize(c->stream);      // the accumulate that waited for the side stream
    return e;
}

size_t bytes_per_path(bool aov, bool env_w, bool alpha) { return lane_bytes_per_path(aov, env_w, alpha); }

int ensure_capacity(ptmi_ctx *c, Lane &ln, size_t n, bool first_hit) {
    const bool aov = c->aov_mask != 0 || first_hit, env_w = c->sc.env.sampled != 0, alpha = alpha_active(c);
    if (n <= ln.cap && (!aov || ln.aov) && (!env_w || ln.paths.W) && (!alpha || ln.alpha.RO)) return PTMI_OK;
    HIP_TRY(c, sync_all(c));
    free_batch(ln);
    const size_t cap = (n + 1023) & ~(size_t)1023;
    c->alloc_oom = false;
    hipError_t e = hipSuccess;
    size_t bytes = 0;
    for (int k = 0; k < kLaneBufs && e == hipSuccess; k++)
        if (lane_buf_wanted(k, aov, env_w, alpha)) e = hipMalloc(&ln.buf[k], bytes = lane_elements(k, cap) * kLaneBytes[k]);
    if (e != hipSuccess) {
        // a failed allocation leaves the lane empty (not half-built) and the runtime's sticky error cleared; ptmi_dispatch retries
        // with a smaller batch when it chose the size itself
        c->alloc_oom = e == hipErrorOutOfMemory;
        free_batch(ln);
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "hipMalloc of %zu bytes for a batch of %zu paths failed: %s", bytes, cap, hipGetErrorString(e));
    }
    ln.cap = cap;
    lane_views(ln);
    return PTMI_OK;
}

size_t plane_bytes(FramePlane k, size_t px) { return kFrame[k].bytes(px); }
uint32_t group_set(PlaneGroup g) {
    uint32_t set = 0;
    for (int k = 0; k < kFramePlanes; k++) if (kFrame[k].group == g) set |= 1u << k;
    return set;
}

// Makes every plane of `set` that `into` (the context's table, or an empty one for fresh planes) lacks, for px pixels, all or nothing:
// on failure what was made is freed, the runtime's sticky error cleared, and `into` and the context are as they were. Nothing is freed
// or overwritten, so nothing in flight is disturbed. Before ptmi_resize (px = 0) there is nothing to make.
int make_planes(ptmi_ctx *c, uint32_t set, size_t px, void **into) {
    void *n[kFramePlanes] = {};
    for (int k = 0; k < kFramePlanes && px; k++) {
        if (!(set & 1u << k) || into[k]) continue;
        const size_t bytes = kFrame[k].bytes(px);
        hipError_t e = hipMalloc(&n[k], bytes);
        if (e == hipSuccess && kFrame[k].zeroed) e = hipMemset(n[k], 0, bytes);
        if (e != hipSuccess) {
            for (void *&p : n) dfree(p);
            (void)hipGetLastError();
            return fail(c, PTMI_E_HIP, "allocation of the %zu-byte %s plane failed: %s (the planes are as they were)", bytes, kFrame[k].name,
                        hipGetErrorString(e));
        }
    }
    for (int k = 0; k < kFramePlanes; k++) if (n[k]) into[k] = n[k];
    view_planes(c);
    return PTMI_OK;
}

int check_ready(ptmi_ctx *c, bool need_output) {
    if (!c) return PTMI_E_INVALID;
    if (!c->have_scene) return fail(c, PTMI_E_STATE, "no scene uploaded (ptmi_upload_scene)");
    if (need_output && (!c->d_out || c->W == 0 || c->H == 0)) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return PTMI_OK;
}

}  // namespace pt_host

// rows of a context: all of [y0, y1), or its strips part, part + parts, ... (the last strip may be short)
DevBand pt_band_of(const ptmi_options &opt, uint32_t W, uint32_t H) {
    DevBand band{W, H, opt.tile_y0, opt.tile_y1 ? std::min(opt.tile_y1, H) : H,
                 std::max(1u, opt.tile_strip), std::max(1u, opt.tile_parts), opt.tile_part, 0u};
    if (band.y0 >= band.y1) return band;
    const uint32_t range = band.y1 - band.y0;
    if (band.parts <= 1u) band.rows = range;
    else
        for (uint32_t s0 = band.part * band.strip; s0 < range; s0 += band.parts * band.strip)
            band.rows += std::min(band.strip, range - s0);
    return band;
}
hipStream_t pt_ctx_stream(ptmi_ctx *c) { return c->stream; }
int pt_ctx_device(const ptmi_ctx *c) { return c->device; }
int pt_ctx_cus(const ptmi_ctx *c) { return c->n_cu; }

extern "C" {

int ptmi_abi_version(void) { return PTMI_ABI_VERSION; }

const char *ptmi_last_error(const ptmi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int ptmi_create(int device_ordinal, ptmi_ctx **out) {
    if (!out) return fail(nullptr, PTMI_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, PTMI_E_NODEVICE, "no HIP device available (%s); this library has no CPU backend",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_ordinal < 0 || device_ordinal >= n)
        return fail(nullptr, PTMI_E_INVALID, "device ordinal %d out of range (%d devices)", device_ordinal, n);
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PTMI_E_NODEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only",
                    device_ordinal, prop.gcnArchName);
    ptmi_ctx *c = new ptmi_ctx();
    c->device = device_ordinal;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    default_options(c->opt);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c; return fail(nullptr, PTMI_E_HIP, "hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    {
        // The shadow stream has a priority level of its own — HIGH — because a priority level has hardware queues of its own. At the
        // caller's (normal) priority the runtime multiplexes it with every other normal-priority stream of the process onto a few
        // hardware queues, and what it gets depends on what was created before: the first context of a process is fine, a context made
        // after another one was destroyed got its shadow stream onto that one's old main queue and ran 6 - 9 % slower, at the
        // one-stream rate (tools/two_contexts.py b, profiles/r03_queues/). At high or at low priority that case is gone; in the ordinary
        // case the three are level (config 1: normal 9 966, high 9 970, low 9 939; config 3: 5 027 / 5 037 / 5 031, interleaved;
        // round 2 had measured low 0.8 - 1.3 % behind normal). -DPT_SIDE_NORMAL_PRIORITY / -DPT_SIDE_LOW_PRIORITY build the others.
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        bool ok = true;
        Lane &ln = c->lane;
#if defined(PT_SIDE_LOW_PRIORITY)
        ok = ok && hipStreamCreateWithPriority(&ln.side, hipStreamNonBlocking, lo) == hipSuccess;
#elif defined(PT_SIDE_NORMAL_PRIORITY)
        ok = ok && hipStreamCreateWithFlags(&ln.side, hipStreamNonBlocking) == hipSuccess;
#else
        ok = ok && hipStreamCreateWithPriority(&ln.side, hipStreamNonBlocking, hi) == hipSuccess;
#endif
        for (hipEvent_t *e : {&ln.ev_ready, &ln.ev_shadow[0], &ln.ev_shadow[1]})
            ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        if (!ok) { ptmi_destroy(c); return fail(nullptr, PTMI_E_HIP, "stream / event creation failed"); }
    }
    if (hipMalloc(&c->d_counters, kCounterWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->d_control, kControlWords * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->d_scene, sizeof(DevScene)) != hipSuccess || hipMemset(c->d_scene, 0, sizeof(DevScene)) != hipSuccess ||
        hipMemset(c->d_counters, 0, kCounterWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->d_control, 0, kControlWords * sizeof(uint32_t)) != hipSuccess) {
        ptmi_destroy(c); return fail(nullptr, PTMI_E_HIP, "device allocation failed");
    }
    c->ad.control = c->d_control; c->ad.counters = c->d_counters;
    if (const char *e = std::getenv("PTMI_SCISSOR")) c->scissor_on = std::strcmp(e, "0") != 0;     // A/B runs and tests: 0 switches it off
    *out = c;
    return PTMI_OK;
}

int ptmi_destroy(ptmi_ctx *c) {
    if (!c) return PTMI_E_INVALID;
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    drain_events(c);
    for (hipEvent_t e : c->in_flight) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    {
        Lane &ln = c->lane;
        free_batch(ln);
        dfree(ln.d_spill); dfree(ln.d_spill_side);
        for (hipEvent_t e : {ln.ev_ready, ln.ev_shadow[0], ln.ev_shadow[1]}) if (e) (void)hipEventDestroy(e);
        if (ln.side) (void)hipStreamDestroy(ln.side);
    }
    for (void *&p : c->buf) dfree(p);
    dfree(c->d_atlas); dfree(c->d_env); dfree(c->d_env_alias); dfree(c->d_med_grid);
    bake_forget(c);
    probes_forget(c);
    drop_planes(c, kAllPlanes);
    dfree(c->d_counters); dfree(c->d_control); dfree(c->d_scene);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return PTMI_OK;
}

}  // extern "C"

int pt_atlas_bytes(uint32_t w, uint32_t h, int fmt, size_t *bytes, char *why, size_t why_len) {
    *bytes = 0;
    if (fmt != PTMI_ATLAS_RGBA16F && fmt != PTMI_ATLAS_RGBA32F) {
        snprintf(why, why_len, "unknown atlas format %d", fmt);
        return PTMI_E_INVALID;
    }
    const size_t texel = fmt == PTMI_ATLAS_RGBA16F ? 8 : 16;
    if ((size_t)w > SIZE_MAX / texel / h) {
        snprintf(why, why_len, "atlas of %ux%u texels does not fit in size_t", w, h);
        return PTMI_E_INVALID;
    }
    *bytes = (size_t)w * h * texel;
    return PTMI_OK;
}

extern "C" {

// Everything is checked and the new texels are on the device before the old atlas goes: a failed call leaves the context's
// atlas, its DevScene and the device copy of that as they were.
int ptmi_upload_atlas(ptmi_ctx *c, const void *texels, uint32_t w, uint32_t h, int fmt) {
    if (!c) return PTMI_E_INVALID;
    const bool remove = !texels || w == 0 || h == 0;
    size_t bytes = 0;
    if (!remove) {
        char why[128];
        if (pt_atlas_bytes(w, h, fmt, &bytes, why, sizeof why) != PTMI_OK) return fail(c, PTMI_E_INVALID, "%s", why);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    void *fresh = nullptr;
    if (!remove) {
        HIP_TRY(c, hipMalloc(&fresh, bytes));
        const hipError_t e = hipMemcpy(fresh, texels, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            dfree(fresh);
            return fail(c, PTMI_E_HIP, "atlas upload failed: %s (the previous atlas, if any, is still in place)", hipGetErrorString(e));
        }
    }
    const hipError_t e = sync_all(c);                 // nothing in flight reads the old atlas any more
    if (e != hipSuccess) {
        dfree(fresh);
        return fail(c, PTMI_E_HIP, "sync_all failed: %s", hipGetErrorString(e));
    }
    dfree(c->d_atlas);
    c->d_atlas = fresh;
    c->sc.atlas = fresh;
    c->sc.atlas_w = remove ? 0u : w; c->sc.atlas_h = remove ? 0u : h; c->sc.atlas_fmt = remove ? 0u : (uint32_t)fmt;
    HIP_TRY(c, hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice));
    return PTMI_OK;
}

// The planes of the new size are made before anything of the old size goes, so a failed call leaves the context as it was; for the
// length of the call both exist, at most 104 B per pixel of the new size (output, three AOV planes, moments, motion, probe depth), small
// beside a batch.
int ptmi_resize(ptmi_ctx *c, uint32_t w, uint32_t h) {
    if (!c) return PTMI_E_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 28)) return fail(c, PTMI_E_INVALID, "bad size %ux%u", w, h);
    HIP_TRY(c, hipSetDevice(c->device));
    void *fresh[kFramePlanes] = {};
    const int rc = make_planes(c, frame_set(c), (size_t)w * h, fresh);
    if (rc) return rc;
    const hipError_t e = sync_all(c);                 // nothing in flight uses the old planes any more
    if (e != hipSuccess) {
        for (void *&p : fresh) dfree(p);
        return fail(c, PTMI_E_HIP, "sync_all failed: %s", hipGetErrorString(e));
    }
    drop_planes(c, kAllPlanes);                       // the denoisers', the adaptive, the history, the blit and the dilate planes come back at their first use
    if (w != c->W || h != c->H) { bake_forget(c); probes_forget(c); }      // a bake surface and a probe atlas are of one size
    std::copy(fresh, fresh + kFramePlanes, c->plane);
    c->W = w; c->H = h;
    c->d_out = plane_as<float4>(c, kOut);
    return reset_adaptive_rounds(c);
}

int ptmi_set_options(ptmi_ctx *c, const ptmi_options *o) {
    if (!c || !o) return PTMI_E_INVALID;
    if (o->max_bounces < 1 || o->max_bounces > kMaxBounces) return fail(c, PTMI_E_INVALID, "max_bounces %u not in 1..64", o->max_bounces);
    if (o->traversal > PTMI_TRAVERSAL_GLOBAL_EXACT) return fail(c, PTMI_E_INVALID, "unknown traversal mode %u", o->traversal);
    if (o->tile_y1 != 0 && o->tile_y0 >= o->tile_y1) return fail(c, PTMI_E_INVALID, "empty tile rows [%u,%u)", o->tile_y0, o->tile_y1);
    if (o->tile_parts > 1 && o->tile_part >= o->tile_parts)
        return fail(c, PTMI_E_INVALID, "tile_part %u is not below tile_parts %u", o->tile_part, o->tile_parts);
    if (o->perf_mode > 1) return fail(c, PTMI_E_INVALID, "unknown perf_mode %u", o->perf_mode);
    if (o->overlap > 2) return fail(c, PTMI_E_INVALID, "unknown overlap %u", o->overlap);
    if (o->reserved_a || o->reserved_b[0] || o->reserved_b[1] || o->reserved_b[2] || o->reserved_b[3] || o->reserved[0])
        return fail(c, PTMI_E_INVALID, "a reserved option word is not zero (ABI <= 3's ray_sort / worklist / tails / state / pipeline are gone: "
                    "start from ptmi_get_options)");
    if (o->leaves > 2) return fail(c, PTMI_E_INVALID, "unknown leaves %u", o->leaves);
    if (o->leaf_tris > PT_LEAF_MAX_TRIS) return fail(c, PTMI_E_INVALID, "leaf_tris %u above %u", o->leaf_tris, PT_LEAF_MAX_TRIS);
    if (o->tree_builder > 2) return fail(c, PTMI_E_INVALID, "unknown tree_builder %u", o->tree_builder);
    c->opt = *o;
    return PTMI_OK;
}
int ptmi_get_options(const ptmi_ctx *c, ptmi_options *o) {
    if (!c || !o) return PTMI_E_INVALID;
    *o = c->opt; return PTMI_OK;
}

}  // extern "C"

extern "C" {

int ptmi_read_output(ptmi_ctx *c, float *dst, size_t n_floats) {
    if (!c || !dst) return PTMI_E_INVALID;
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return read_plane(c, kOut, c->d_out, dst, n_floats, 4);
}

int ptmi_write_output(ptmi_ctx *c, const float *src, size_t n_floats) {
    if (!c || !src) return PTMI_E_INVALID;
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (n_floats != (size_t)c->W * c->H * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", (size_t)c->W * c->H * 4, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(c->d_out, src, n_floats * 4, hipMemcpyHostToDevice));
    return PTMI_OK;
}

void *ptmi_output_device_ptr(ptmi_ctx *c) { return c ? c->d_out : nullptr; }

int ptmi_bind_output_device(ptmi_ctx *c, void *p, size_t bytes) {
    if (!c) return PTMI_E_INVALID;
    if (c->W == 0) return fail(c, PTMI_E_STATE, "call ptmi_resize first");
    if (!p) { c->d_out = plane_as<float4>(c, kOut); return PTMI_OK; }
    if (bytes < (size_t)c->W * c->H * PTMI_OUTPUT_STRIDE) return fail(c, PTMI_E_INVALID, "buffer of %zu bytes is too small", bytes);
    if (reinterpret_cast<uintptr_t>(p) & 15u) return fail(c, PTMI_E_INVALID, "buffer must be 16-byte aligned");
    c->d_out = static_cast<float4 *>(p);
    return PTMI_OK;
}

int ptmi_set_stream(ptmi_ctx *c, void *s) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, quiesce(c));
    c->stream = s ? static_cast<hipStream_t>(s) : c->own_stream;
    return PTMI_OK;
}

namespace {
// ptmi_blit's contract for any W x H float4 plane of the context; the staging planes are kept between calls
int blit_from(ptmi_ctx *c, const float4 *src, float *dst_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes) {
    if (!dst_f32 && !dst_rgba8) return PTMI_OK;
    const size_t n = (size_t)c->W * c->H;
    if (dst_f32 && n_floats != n * 4) return fail(c, PTMI_E_INVALID, "float canvas: expected %zu floats, got %zu", n * 4, n_floats);
    if (dst_rgba8 && n_bytes != n * 4) return fail(c, PTMI_E_INVALID, "8-bit canvas: expected %zu bytes, got %zu", n * 4, n_bytes);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = make_planes(c, (dst_f32 ? bit(kBlitF32) : 0u) | (dst_rgba8 ? bit(kBlitU8) : 0u), n, c->plane);
    if (rc) return rc;
    pt_launch_blit(c->stream, c->n_cu * 8, c->W, c->H, src, dst_f32 ? plane_as<float4>(c, kBlitF32) : nullptr,
                   dst_rgba8 ? plane_as<uint32_t>(c, kBlitU8) : nullptr);
    if (dst_f32 && (rc = read_plane(c, kBlitF32, c->plane[kBlitF32], dst_f32, n_floats, 4))) return rc;
    if (dst_rgba8 && (rc = read_plane(c, kBlitU8, c->plane[kBlitU8], dst_rgba8, n_bytes, 1))) return rc;
    return PTMI_OK;
}
}  // namespace

int ptmi_blit(ptmi_ctx *c, float *dst_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes) {
    if (!c) return PTMI_E_INVALID;
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return blit_from(c, c->d_out, dst_f32, n_floats, dst_rgba8, n_bytes);
}

int ptmi_get_size(const ptmi_ctx *c, uint32_t *w, uint32_t *h) {
    if (!c || !w || !h) return PTMI_E_INVALID;
    *w = c->W; *h = c->H;
    return PTMI_OK;
}

int ptmi_set_aovs(ptmi_ctx *c, uint32_t mask) {
    if (!c) return PTMI_E_INVALID;
    if (mask & ~kAovAll) return fail(c, PTMI_E_INVALID, "unknown AOV bits 0x%x", mask & ~kAovAll);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                     // nothing in flight writes a plane or a record that goes
    const int rc = make_planes(c, mask << kAovAlbedo, (size_t)c->W * c->H, c->plane);    // planes already on keep their contents
    if (rc) return rc;
    drop_planes(c, (kAovAll & ~mask) << kAovAlbedo);
    c->aov_mask = mask;
    if (!mask) { dfree(c->lane.buf[kAovRec]); lane_views(c->lane); }      // the records live only while a plane is on (ensure_capacity makes them;
                                                                          // a probe dispatch that folds the depth plane makes its own again)
    return PTMI_OK;
}

int ptmi_get_aovs(const ptmi_ctx *c, uint32_t *mask) {
    if (!c || !mask) return PTMI_E_INVALID;
    *mask = c->aov_mask;
    return PTMI_OK;
}

int ptmi_read_aov(ptmi_ctx *c, uint32_t which, void *dst, size_t n_bytes) {
    if (!c) return PTMI_E_INVALID;
    const FramePlane k = aov_plane_of(which);
    if (k == kFramePlanes) return fail(c, PTMI_E_INVALID, "which = 0x%x is not one PTMI_AOV_* plane", which);
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!(c->aov_mask & which)) return fail(c, PTMI_E_STATE, "AOV plane 0x%x is off (ptmi_set_aovs)", which);
    if (!c->plane[k]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return read_plane(c, k, c->plane[k], dst, n_bytes, 1);
}

void *ptmi_aov_device_ptr(ptmi_ctx *c, uint32_t which) {
    if (!c) return nullptr;
    const FramePlane k = aov_plane_of(which);
    return k != kFramePlanes && (c->aov_mask & which) ? c->plane[k] : nullptr;
}

int ptmi_set_moments(ptmi_ctx *c, uint32_t on) {
    if (!c) return PTMI_E_INVALID;
    if (on > 1u) return fail(c, PTMI_E_INVALID, "on = %u is not 0 or 1", on);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                     // nothing in flight writes a plane that goes
    if (on) {
        const int rc = make_planes(c, bit(kMoments), (size_t)c->W * c->H, c->plane);
        if (rc) return rc;
    } else drop_planes(c, bit(kMoments));
    if ((on != 0) != c->moments_on) { const int rc = reset_adaptive_rounds(c); if (rc) return rc; }
    c->moments_on = on != 0;
    return PTMI_OK;
}

int ptmi_get_moments(const ptmi_ctx *c, uint32_t *on) {
    if (!c || !on) return PTMI_E_INVALID;
    *on = c->moments_on ? 1u : 0u;
    return PTMI_OK;
}

int ptmi_read_moments(ptmi_ctx *c, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!c->moments_on) return fail(c, PTMI_E_STATE, "the moments plane is off (ptmi_set_moments)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return read_plane(c, kMoments, c->plane[kMoments], dst, n_floats, 4);
}

int ptmi_write_moments(ptmi_ctx *c, const float *src, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!src) return fail(c, PTMI_E_INVALID, "src is NULL");
    if (!c->moments_on) return fail(c, PTMI_E_STATE, "the moments plane is off (ptmi_set_moments)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (n_floats != (size_t)c->W * c->H * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", (size_t)c->W * c->H * 4, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(c->plane[kMoments], src, n_floats * 4, hipMemcpyHostToDevice));
    return PTMI_OK;
}

void *ptmi_moments_device_ptr(ptmi_ctx *c) { return c && c->moments_on ? c->plane[kMoments] : nullptr; }

// (the fold and the reduction of the plane: dispatch.hip, probes.hip)
int ptmi_set_probe_depth(ptmi_ctx *c, const ptmi_probe_depth_params *params) {
    if (!c) return PTMI_E_INVALID;
    if (params) {
        if (!std::isfinite(params->max_distance) || !(params->max_distance > 0.0f))
            return fail(c, PTMI_E_INVALID, "max_distance %g is not finite and > 0", (double)params->max_distance);
        for (uint32_t r : params->_reserved) if (r) return fail(c, PTMI_E_INVALID, "a reserved word of ptmi_probe_depth_params is not zero");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));                     // nothing in flight writes a plane or a record that goes
    if (params) {
        const int rc = make_planes(c, bit(kProbeDepth), (size_t)c->W * c->H, c->plane);      // a plane already on keeps its contents
        if (rc) return rc;
        c->probe_depth = *params;
    } else {
        drop_planes(c, bit(kProbeDepth));
        c->probe_depth = {};
        if (!c->aov_mask) { dfree(c->lane.buf[kAovRec]); lane_views(c->lane); }      // the records a probe dispatch kept for the fold
    }
    c->probe_depth_on = params != nullptr;
    return PTMI_OK;
}

int ptmi_get_probe_depth(ptmi_ctx *c, uint32_t *on, ptmi_probe_depth_params *out) {
    if (!c || !on) return PTMI_E_INVALID;
    *on = c->probe_depth_on ? 1u : 0u;
    if (out) *out = c->probe_depth;
    return PTMI_OK;
}

int ptmi_read_probe_depth(ptmi_ctx *c, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!c->probe_depth_on) return fail(c, PTMI_E_STATE, "the probe depth plane is off (ptmi_set_probe_depth)");
    if (!c->plane[kProbeDepth]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return read_plane(c, kProbeDepth, c->plane[kProbeDepth], dst, n_floats, 4);
}

int ptmi_write_probe_depth(ptmi_ctx *c, const float *src, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!src) return fail(c, PTMI_E_INVALID, "src is NULL");
    if (!c->probe_depth_on) return fail(c, PTMI_E_STATE, "the probe depth plane is off (ptmi_set_probe_depth)");
    if (!c->plane[kProbeDepth]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (n_floats != (size_t)c->W * c->H * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", (size_t)c->W * c->H * 4, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipMemcpy(c->plane[kProbeDepth], src, n_floats * 4, hipMemcpyHostToDevice));
    return PTMI_OK;
}

void *ptmi_probe_depth_device_ptr(ptmi_ctx *c) { return c && c->probe_depth_on ? c->plane[kProbeDepth] : nullptr; }

int ptmi_denoise(ptmi_ctx *c, const ptmi_denoise_params *p, float *dst_rgba, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    const ptmi_denoise_params zero = {};
    const ptmi_denoise_params &q = p ? *p : zero;
    // (an unknown demodulate is refused after iterations above 10 and before everything else)
    if (q.iterations <= 10u && q.demodulate > 2u) return fail(c, PTMI_E_INVALID, "unknown demodulate %u", q.demodulate);
    AtrousArgs da;
    int rc = atrous_params(c, q.iterations, q.reserved, "", q.phi_color, q.phi_normal, q.phi_depth, &da);
    if (rc) return rc;
    const size_t npix = (size_t)c->W * c->H;
    if (dst_rgba && n_floats != npix * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", npix * 4, n_floats);
    if (!(c->aov_mask & PTMI_AOV_NORMAL) || !c->plane[kAovNormal])
        return fail(c, PTMI_E_STATE, "the denoiser needs the NORMAL plane (ptmi_set_aovs)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "the denoiser needs the moments plane (ptmi_set_moments)");
    const bool have_albedo = (c->aov_mask & PTMI_AOV_ALBEDO) && c->plane[kAovAlbedo];
    if (q.demodulate == 2u && !have_albedo) return fail(c, PTMI_E_STATE, "demodulate = 2 needs the ALBEDO plane (ptmi_set_aovs)");
    const bool demod = q.demodulate == 2u || (q.demodulate == 0u && have_albedo);
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = make_planes(c, group_set(kByDenoise), npix, c->plane))) return rc;
    pt_launch_denoise(c->stream, da, c->d_out, plane_as<float4>(c, kAovNormal), demod ? plane_as<float4>(c, kAovAlbedo) : nullptr,
                      plane_as<float4>(c, kMoments), plane_as<float4>(c, kDnGuide), plane_as<float>(c, kDnGrad), plane_as<float4>(c, kDnA),
                      plane_as<float4>(c, kDnB), plane_as<float4>(c, kDnOut));
    HIP_TRY(c, hipGetLastError());
    return dst_rgba ? read_plane(c, kDnOut, c->plane[kDnOut], dst_rgba, n_floats, 4) : PTMI_OK;
}

void *ptmi_denoised_device_ptr(ptmi_ctx *c) { return c ? c->plane[kDnOut] : nullptr; }

int ptmi_blit_denoised(ptmi_ctx *c, float *dst_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes) {
    if (!c) return PTMI_E_INVALID;
    if (!c->plane[kDnOut]) return fail(c, PTMI_E_STATE, "nothing denoised since the last resize (ptmi_denoise)");
    return blit_from(c, plane_as<float4>(c, kDnOut), dst_f32, n_floats, dst_rgba8, n_bytes);
}

int ptmi_get_stats(ptmi_ctx *c, ptmi_stats *out) {
    if (!c || !out) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    unsigned long long h[kCtDispatchEnd];
    HIP_TRY(c, hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    c->st.segments = h[kCtSegments];
    c->st.shadow_rays = h[kCtShadowRays] - h[kCtEmitRecords]; c->st.shadow_traced = h[kCtShadowTraced] - h[kCtEmitRecords];
    for (int i = 0; i < kMaxBounces; i++) c->st.segments_by_bounce[i] = h[kCtByBounce + i];
    c->st.verify_failed = h[kCtVerifyFailed];
    c->st.bvh_depth = stats_depth(c);
    *out = c->st;
    out->paths += h[kCtAdTraced];                     // the samples adaptive dispatches traced: in the returned copy only
    return PTMI_OK;
}

int ptmi_reset_stats(ptmi_ctx *c) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    HIP_TRY(c, hipMemset(c->d_counters, 0, kCtDispatchEnd * sizeof(unsigned long long)));      // not the status words of the last calls
    const ptmi_stats old = c->st;
    std::memset(&c->st, 0, sizeof c->st);
    c->scissor.skipped = 0;
    c->st.bvh_depth = stats_depth(c);
    c->st.upload_ms = old.upload_ms; c->st.upload_tree_ms = old.upload_tree_ms; c->st.upload_copy_ms = old.upload_copy_ms;
    c->st.leaves_used = old.leaves_used; c->st.leaf_tris_used = old.leaf_tris_used; c->st.tree_builder_used = old.tree_builder_used;
    return PTMI_OK;
}

}  // extern "C"
