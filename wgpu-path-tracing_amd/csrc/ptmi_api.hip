// ptmi_api.hip — the C ABI of include/ptmi.h: context, resource upload, the wavefront
// dispatch loop and the per-stage debug entry points.
//
// Replaces the host side of the reference's compute pass (src/renderer/renderer.ts:
// createBuffers :242-355, createBindGroups :368-381, updateCamera + dispatch :403-431).
#include "ptmi.h"
#include "pt_device.h"
#include "fast_tree.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <typeinfo>
#include <utility>
#include <vector>

namespace {

thread_local std::string g_create_err;

// The device buffers of an uploaded scene, one entry each (the atlas is ptmi_upload_atlas's). The walked image's entries are absent when
// the kernels walk the tree as uploaded: DevScene then points at the reference entries.
enum SceneBuf {
    kTris, kMats, kLights,
    kRefWnodes, kRefTripos,            // the tree as uploaded; triangle images in original order
    kWnodes, kTripos,                  // the walked image: a hierarchy rebuilt over the reference's leaves (nodes only), or own leaves
    kQnodes, kLeafStream,              // its quantised nodes; the leaf stream (the reference's leaves only)
    kLeafbox,                          // own leaves: per original triangle, the box of the reference leaf that lists it
    kWnodes16, kRefWnodes16, kQnodes16,    // own leaves, small scenes: the two hierarchies and the quantised nodes with 16-bit references
    kShadeTab,                         // the shade tables: materials, lights and the lights' triangles in one blob (pt_device.h)
    kSceneBufs
};

// The per-pixel buffers that follow the output size, one entry each (kFrame below: what each takes and when it is made).
enum FramePlane {
    kOut,                                          // the context's own output buffer (binding 0)
    kAovAlbedo, kAovNormal, kAovId,                // first-hit planes (ptmi_set_aovs), in the order of the PTMI_AOV_* bits
    kMoments,                                      // sample moments (ptmi_set_moments)
    kDnGuide, kDnGrad, kDnA, kDnB, kDnOut,         // the denoiser's: guide (unit normal, depth), depth gradient, two ping-pong colour +
                                                   // variance planes, the result
    kAdBallot, kAdList, kAdTileSums,               // adaptive sampling: ballot words, pixel list, tile totals
    kRpOut, kRpMoments, kRpNormal, kRpAlbedo, kRpId,   // reprojection: the snapshot of the output, moments and first-hit planes
    kBlitF32, kBlitU8,                             // canvas staging of ptmi_blit
    kFramePlanes
};

// The per-path arrays of a batch, one entry each (kLaneBytes below: what each takes per path), in the order they are allocated.
enum LaneBuf {
    kPathO, kPathD, kPathC, kPathL,                // path state; L has room for either stride
    kHits,
    kShadow0, kShadowIdx0, kShadow1, kShadowIdx1,  // shadow records (SO, SD, SC in one block) and their index arrays, by bounce parity
    kTailO, kTailD, kTailC, kPid,                  // state by queue slot after the repack, and the path id of each such slot
    kQueue0, kQueue1,
    kOcc,                                          // occlusion bytes (ptmi_debug_occluded)
    kAovRec,                                       // first-hit records of bounce 0 (k_shade<true>); only while AOV planes are on
    kLaneBufs
};

struct EventPair { hipEvent_t a, b; int kind; };   // kind: 0 dispatch, 1 extend, 2 shade, 3 shadow, 4 raygen, 5 compaction, 6 accumulate
constexpr size_t kMaxPendingEvents = 4096;        // a caller that never synchronises (a preview loop) must not grow the list without bound

}  // namespace

// The buffers of the wavefront batch in flight, and the second stream that lets `shadow` run beside the next bounce.
struct Lane {
    size_t cap = 0;
    void *buf[kLaneBufs] = {};                         // indexed by LaneBuf; the typed members below are views of it (lane_views)
    DevPaths paths{};
    float2 *hits = nullptr;
    DevShadow sh[2]{};                                 // shadow records, double-buffered by bounce parity (overlap)
    uint32_t *queue[2] = {nullptr, nullptr}, *sq[2] = {nullptr, nullptr};
    DevPaths tail{};                                   // O / D / C by queue slot from the bounce after the repack (L unused)
    uint32_t *pid = nullptr;                           // ... and the path id of each such slot
    uint64_t *alive = nullptr, *shadowm = nullptr;
    size_t mask_words = 0;
    uint32_t *word_off = nullptr, *counts = nullptr;
    uint32_t *d_spill = nullptr;          // node-stack overflow of the global traversal variant (128 MiB on 256 CUs; first use)
    uint32_t *d_spill_side = nullptr;     // ... of the `shadow` kernel when it runs beside `extend`
    uint8_t *d_occ = nullptr;
    hipStream_t side = nullptr;           // `shadow` of bounce b beside the kernels of bounce b + 1
    hipEvent_t ev_ready = nullptr, ev_shadow[2] = {nullptr, nullptr};
    float4 *aov = nullptr;                // first-hit records of bounce 0, 32 B per path (k_shade<true>); only while AOV planes are on
};

struct ptmi_ctx {
    int device = 0, n_cu = 256;
    hipStream_t own_stream = nullptr, stream = nullptr;
    Lane lane;
    mutable std::string err;
    bool alloc_oom = false;                            // the last failed batch allocation ran out of device memory
    ptmi_options opt{};

    // scene (bindings 1, 2, 4, 5, 6)
    void *buf[kSceneBufs] = {};                        // indexed by SceneBuf (absent: NULL)
    void *d_atlas = nullptr;
    DevScene *d_scene = nullptr;                       // sc in device memory (DevScene::self), rewritten whenever sc changes
    DevScene sc{};
    bool have_scene = false;
    ptmi_image_info img{};                   // what the last upload put on the device (ptmi_debug_read_image)

    // output (binding 0)
    uint32_t W = 0, H = 0;
    void *plane[kFramePlanes] = {};                    // indexed by FramePlane, W x H pixels each (absent: NULL)
    float4 *d_out = nullptr;                           // what dispatches write: plane[kOut] or the caller's buffer (ptmi_bind_output_device)
    uint32_t aov_mask = 0;                             // ptmi_set_aovs: a plane is present while its bit is set and the output buffer exists
    bool moments_on = false;                           // ptmi_set_moments: likewise
    // adaptive sampling (ptmi_dispatch_adaptive): ballot, list and tile_sums are views of the planes; the control words and counters
    // live for the context's life
    DevAdaptive ad{};
    uint32_t ad_rounds = 0;                            // rounds since the last restart
    unsigned long long *d_reproject = nullptr;         // ptmi_reproject_status: the four counters of the last ptmi_reproject (made by the first)

    unsigned long long *d_stats = nullptr;

    // statistics
    ptmi_stats st{};
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> event_pool;
    std::deque<hipEvent_t> in_flight;                  // one event per ptmi_dispatch, recorded behind its last kernel (ptmi_throttle)
};

namespace {

constexpr int kStatsWords = 8 + 64;
constexpr int kShadowCount = 72;          // slot of the shadow-queue length in ctx->counts (80 words)
constexpr size_t kLdsMax = 160 * 1024;
void vfail(std::string &err, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    err = buf;
}
int fail(std::string &err, int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfail(err, fmt, ap); va_end(ap);
    return code;
}
int fail(const ptmi_ctx *c, int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfail(c ? c->err : g_create_err, fmt, ap); va_end(ap);
    return code;
}
#define HIP_TRY(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail((c), PTMI_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

template <class T> void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }
// device scratch of one call (the ptmi_debug_*math entry points), freed on every way out of it
template <class T> struct Scratch { T *p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } };
template <class T> void view(T *&p, void *b) { p = static_cast<T *>(b); }      // a typed member that stands for an entry of a buffer table

void default_options(ptmi_options &o) {
    std::memset(&o, 0, sizeof o);
    o.max_bounces = 8; o.do_mis = 1; o.cull = 1; o.traversal = PTMI_TRAVERSAL_AUTO; o.overlap = 2;
}

hipEvent_t get_event(ptmi_ctx *c) {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}

// resolve finished event pairs into the statistics (stream must be synchronised)
void drain_events(ptmi_ctx *c) {
    for (auto &p : c->pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            switch (p.kind) {
            case 0: c->st.gpu_ms += ms; break;
            case 1: c->st.extend_ms += ms; c->st.extend_launches++; break;
            case 2: c->st.shade_ms += ms; c->st.shade_launches++; break;
            case 3: c->st.shadow_ms += ms; c->st.shadow_launches++; break;
            case 4: c->st.raygen_ms += ms; break;
            case 5: c->st.compact_ms += ms; break;
            case 6: c->st.accumulate_ms += ms; break;
            }
        }
        c->event_pool.push_back(p.a); c->event_pool.push_back(p.b);
    }
    c->pending.clear();
}

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

constexpr size_t kMaxDispatchesInFlight = 256;     // a caller that never throttles or synchronises still cannot queue without bound

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
    ptmi_ctx *c; hipEvent_t a = nullptr, b = nullptr; int kind; bool on;
    hipStream_t st;
    Timed(ptmi_ctx *c_, int kind_, bool on_, hipStream_t st_ = nullptr) : c(c_), kind(kind_), on(on_), st(st_ ? st_ : c_->stream) {
        if (on) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, st); }
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(b, st);
        c->pending.push_back({a, b, kind});
        if (c->pending.size() > kMaxPendingEvents) drain_completed_events(c);
    }
};

// what a path of a batch takes in each of the lane's per-path arrays, in bytes
constexpr size_t kLaneBytes[kLaneBufs] = {
    16, 16, 8, 16,                                 // kPathO .. kPathL
    8,                                             // kHits
    16 + 16 + sizeof(rgb_sc), 4, 16 + 16 + sizeof(rgb_sc), 4,      // kShadow0, kShadowIdx0, kShadow1, kShadowIdx1
    16, 16, 8, 4,                                  // kTailO .. kPid
    4, 4,                                          // kQueue0, kQueue1
    1,                                             // kOcc
    32,                                            // kAovRec
};
// bytes of device memory a path of a batch takes in ensure_capacity: the per-path arrays and one byte for the two masks (2 x 8 B per 64
// paths). The automatic batch size and its out-of-memory retry (ptmi_dispatch) rely on it.
constexpr size_t bytes_per_path(bool aov) {
    size_t n = 1;
    for (int k = 0; k < kLaneBufs; k++) if (k != kAovRec || aov) n += kLaneBytes[k];
    return n;
}
static_assert(bytes_per_path(false) == 214 && bytes_per_path(true) == 246, "the automatic frames_per_batch moves with these");

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
}

void free_batch(Lane &ln) {
    for (void *&p : ln.buf) dfree(p);
    dfree(ln.alive); dfree(ln.shadowm); dfree(ln.word_off);
    ln.cap = 0;
    lane_views(ln);
}

// everything the library has in flight, on every stream it owns
hipError_t sync_all(ptmi_ctx *c) {
    hipError_t e = c->stream ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (e == hipSuccess && c->lane.side) e = hipStreamSynchronize(c->lane.side);
    if (e == hipSuccess && c->stream) e = hipStreamSynchronize(c->stream);      // the accumulate that waited for the side stream
    return e;
}

#ifndef PT_REPACK
#define PT_REPACK 1          /* A/B switch: 0 leaves the path state at the path id for every bounce (no tail arrays in use) */
#endif

int ensure_capacity(ptmi_ctx *c, Lane &ln, size_t n) {
    const bool aov = c->aov_mask != 0;
    if (n <= ln.cap && (!aov || ln.aov)) return PTMI_OK;
    HIP_TRY(c, sync_all(c));
    free_batch(ln);
    const size_t cap = (n + 1023) & ~(size_t)1023;
    const size_t words = cap / 64 + 1;
    const size_t tiles = cap / pt_compact_tile_slots() + 2;
    c->alloc_oom = false;
    hipError_t e = hipSuccess;
    size_t bytes = 0;
    for (int k = 0; k < kLaneBufs && e == hipSuccess; k++)
        if (k != kAovRec || aov) e = hipMalloc(&ln.buf[k], bytes = cap * kLaneBytes[k]);
    if (e == hipSuccess) e = hipMalloc(&ln.alive, bytes = words * 8);
    if (e == hipSuccess) e = hipMalloc(&ln.shadowm, bytes = words * 8);
    if (e == hipSuccess) e = hipMalloc(&ln.word_off, bytes = 2 * tiles * 4);
    if (e != hipSuccess) {
        // a failed allocation leaves the lane empty (not half-built) and the runtime's sticky error cleared; ptmi_dispatch retries
        // with a smaller batch when it chose the size itself
        c->alloc_oom = e == hipErrorOutOfMemory;
        free_batch(ln);
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "hipMalloc of %zu bytes for a batch of %zu paths failed: %s", bytes, cap, hipGetErrorString(e));
    }
    ln.mask_words = words;
    ln.cap = cap;
    lane_views(ln);
    return PTMI_OK;
}

// ---- scene validation and the traversal image ---------------------------------
// One scene buffer as a preparation leaves it: absent, host bytes (a vector moved in, or the caller's blob), or a buffer on `device` that
// the install takes over or copies.
struct HeldBuf {
    bool present = false;
    std::shared_ptr<const void> keep;        // the vector `host` points into (none: the caller's blob)
    const std::type_info *type = nullptr;    // ... and its type
    const void *host = nullptr;
    void *dev = nullptr;
    int device = -1;
    size_t bytes = 0;
};

// The scene's buffers, and one header for the image the kernels walk.
struct Built {
    HeldBuf buf[kSceneBufs];
    ptmi_image_info img{};                   // the walked image (ptmi_debug_read_image); ref_depth: levels of the tree as uploaded
    uint32_t ref_root_ref = PT_REF_NONE;     // the root of the tree as uploaded
    float ref_root_min[3] = {0, 0, 0}, ref_root_max[3] = {0, 0, 0};
    uint32_t root_ref16 = PT_REF_NONE, ref_root_ref16 = PT_REF_NONE;     // the roots of kWnodes16 / kRefWnodes16
    uint32_t q_top = 0;                      // quantised nodes numbered breadth-first at the front (LDS-resident in the kernel)
    float tri_safe_dsum = 0.0f;              // DevScene::tri_safe_dsum
    uint32_t tree_builder_used = 0;          // ptmi_stats.tree_builder_used
    double tree_ms = 0.0;                    // time spent building and quantising the walked hierarchy

    Built() { img.leaves_used = 1; img.root_ref = PT_REF_NONE; }
    Built(const Built &) = delete;
    Built &operator=(const Built &) = delete;
    ~Built() { for (HeldBuf &e : buf) if (e.dev) (void)hipFree(e.dev); }

    template <class T> void hold(int k, std::vector<T> &&v) {
        auto p = std::make_shared<const std::vector<T>>(std::move(v));
        buf[k].present = true; buf[k].host = p->data(); buf[k].bytes = p->size() * sizeof(T); buf[k].keep = std::move(p);
        buf[k].type = &typeid(std::vector<T>);
    }
    void view(int k, const void *host, size_t bytes) { buf[k].present = true; buf[k].host = host; buf[k].bytes = bytes; }
    void on_device(int k, void *dev, size_t bytes, int device) {
        buf[k].present = true; buf[k].dev = dev; buf[k].bytes = bytes; buf[k].device = device;
    }
    template <class T> const std::vector<T> &vec(int k) const {       // an entry held on the host as a vector of T (else empty)
        static const std::vector<T> none;
        const HeldBuf &e = buf[k];
        return e.type && *e.type == typeid(std::vector<T>) ? *static_cast<const std::vector<T> *>(e.keep.get()) : none;
    }
};

// kWnodes / kTripos as the kernels walk them, in a preparation's table or a context's: the reference's entry when no other image was built
bool present(const HeldBuf &e) { return e.present; }
bool present(const void *d) { return d != nullptr; }
template <class E> const E &walked(const E *buf, SceneBuf k) { return present(buf[k]) ? buf[k] : buf[k == kWnodes ? kRefWnodes : kRefTripos]; }

// a copy of a wide-node image whose child references fit 16 bits: an internal node's index, or 0x8000 | (count - 1) << 12 | first
// triangle. false: some reference does not fit (more than 32 767 nodes, a leaf beyond triangle 4 095 or of more than 8 triangles)
bool compact_ref(uint32_t r, uint32_t &o) {
    if (r & PT_REF_LEAF) {
        const uint32_t first = r & PT_LEAF_OFF_MASK, cnt = ((r >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u;
        if (first > 0xFFFu || cnt > 8u) return false;
        o = 0x8000u | ((cnt - 1u) << 12) | first;
    } else {
        if (r > 0x7FFFu) return false;
        o = r;
    }
    return true;
}
bool compact_refs(const std::vector<float4> &w, uint32_t root, std::vector<float4> &out, uint32_t &root16) {
    auto conv = compact_ref;
    out = w;
    if (root == PT_REF_NONE || !conv(root, root16)) return false;
    for (size_t i = 0; i < w.size() / 4; i++) {
        uint32_t l, r, l16, r16;
        std::memcpy(&l, &w[i * 4 + 3].x, 4); std::memcpy(&r, &w[i * 4 + 3].y, 4);
        if (!conv(l, l16) || !conv(r, r16)) return false;
        std::memcpy(&out[i * 4 + 3].x, &l16, 4); std::memcpy(&out[i * 4 + 3].y, &r16, 4);
    }
    return true;
}

#ifndef PT_LEAVES_DEFAULT
#define PT_LEAVES_DEFAULT 2            /* what ptmi_options.leaves = 0 means (measured: profiles/README.md) */
#endif
#ifndef PT_LEAF_TRIS_DEFAULT
#define PT_LEAF_TRIS_DEFAULT 2         /* ... and ptmi_options.leaf_tris = 0 */
#endif

uint32_t leaf_ref(const ptmi_bvh_node &n) {
    return PT_REF_LEAF | ((n.triangle_count - 1u) << PT_LEAF_OFF_BITS) | n.triangle_offset;
}

// The own tree on `device` (own_tree_gpu.hip) from a device copy of the triangles, made first and kept as b's kTris for the upload to
// take over. false: not built (the caller builds on the host).
bool own_tree_on_device(hipStream_t stream, int device, const ptmi_triangle *tris, uint32_t nt, const std::vector<uint32_t> &which,
                        const std::vector<float4> &leafbox, uint32_t k_max, uint32_t limit, Built &b, PtOwnTreeGpu &g) {
    const size_t bytes = (size_t)nt * sizeof(ptmi_triangle);
    void *d_tris = nullptr;
    if (hipMalloc(&d_tris, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMemcpy(d_tris, tris, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_tris); (void)hipGetLastError(); return false; }
    b.on_device(kTris, d_tris, bytes, device);
    return pt_build_own_tree_gpu(static_cast<const ptmi_triangle *>(d_tris), which, leafbox, k_max, limit, stream, g);
}

// Own leaves, after whichever builder ran (on_device: g on `device`, else t): the walked image and its header, the quantised nodes (the
// device builder made its own) and, for scenes of up to 4 096 triangles, both hierarchies and the quantised nodes once more with 16-bit
// child references (the device builder only runs on larger scenes).
void own_image(Built &b, bool on_device, int device, PtOwnTreeGpu &g, PtOwnTree &t, uint32_t nt, const std::vector<float4> &ref_wnodes,
               std::vector<float4> &&leafbox) {
    ptmi_image_info &h = b.img;
    const PtOwnTreeHeader &o = on_device ? static_cast<const PtOwnTreeHeader &>(g) : t;
    h.leaves_used = 2u; h.root_ref = o.root_ref; h.depth = o.depth; h.n_leaves = o.n_leaves; h.max_leaf_tris = o.max_leaf_tris;
    for (int k = 0; k < 3; k++) { h.root_min[k] = o.root_min[k]; h.root_max[k] = o.root_max[k]; }
    h.pad = o.pad; h.safe_origin = o.safe_origin;
    b.tree_builder_used = on_device ? 2u : 1u;
    b.hold(kLeafbox, std::move(leafbox));
    if (on_device) {
        h.n_wnodes = g.n_wnodes; h.n_tris = g.n_tris; h.quantised = g.quantised ? 1u : 0u; b.q_top = g.q_top;
        for (int k = 0; k < 3; k++) { h.q_origin[k] = g.q_origin[k]; h.q_scale[k] = g.q_scale[k]; }
        b.on_device(kWnodes, g.wnodes, (size_t)g.n_wnodes * 64, device);
        b.on_device(kTripos, g.tripos, (size_t)g.n_tris * 48, device);
        if (g.quantised) b.on_device(kQnodes, g.qnodes, (size_t)g.n_wnodes * 32, device);
        g.wnodes = nullptr; g.tripos = nullptr; g.qnodes = nullptr;
        return;
    }
    std::vector<uint4> q;
    float qo[3], qs[3];
    if (pt_quantize_nodes(t.wnodes, q, qo, qs, PT_QCACHE_NODES, b.q_top))
        for (int k = 0; k < 3; k++) { h.q_origin[k] = qo[k]; h.q_scale[k] = qs[k]; }
    else q.clear();
    std::vector<float4> w16, r16;
    uint32_t root16, ref_root16;
    if (nt <= 4096u && !t.wnodes.empty() && compact_refs(t.wnodes, t.root_ref, w16, root16) && compact_refs(ref_wnodes, b.ref_root_ref, r16, ref_root16)) {
        b.root_ref16 = root16; b.ref_root_ref16 = ref_root16;
        if (!q.empty()) {                              // (the quantised nodes are renumbered: node 0 stays the root)
            std::vector<uint4> q16 = q;
            bool ok = true;
            for (uint4 &x : q16) if (!(ok = compact_ref(x.w, x.w))) break;
            if (ok) b.hold(kQnodes16, std::move(q16));
        }
        b.hold(kWnodes16, std::move(w16)); b.hold(kRefWnodes16, std::move(r16));
    }
    h.n_wnodes = (uint32_t)(t.wnodes.size() / 4); h.n_tris = (uint32_t)(t.tripos.size() / 3); h.quantised = q.empty() ? 0u : 1u;
    b.hold(kWnodes, std::move(t.wnodes)); b.hold(kTripos, std::move(t.tripos));
    if (!q.empty()) b.hold(kQnodes, std::move(q));
}

// The traversal image of a scene under `opt`. tree_builder = 2 builds on `device` through `stream` (none: the host-only debug entry
// points build on the host). err: why a scene is refused.
int build_image(const ptmi_options &opt, hipStream_t stream, int device, const ptmi_triangle *tris, uint32_t nt,
                const ptmi_bvh_node *nodes, uint32_t nn, Built &b, std::string &err) {
    if (nt == 0 || nn == 0) {                                      // empty scene: every ray misses
        b.hold(kRefWnodes, std::vector<float4>()); b.hold(kRefTripos, std::vector<float4>());
        return PTMI_OK;
    }
    if (nt > PT_LEAF_OFF_MASK) return fail(err, PTMI_E_UNSUPPORTED, "more than %u triangles", PT_LEAF_OFF_MASK);
    // leaf <=> triangleCount > 0 (pt.wgsl:271)
    auto check_leaf = [&](uint32_t i) -> int {
        const ptmi_bvh_node &n = nodes[i];
        if (n.triangle_count > PT_LEAF_MAX_TRIS)
            return fail(err, PTMI_E_UNSUPPORTED, "BVH leaf %u holds %u triangles (limit %u)", i, n.triangle_count, PT_LEAF_MAX_TRIS);
        if ((uint64_t)n.triangle_offset + n.triangle_count > nt)
            return fail(err, PTMI_E_INVALID, "BVH leaf %u references triangles [%u,+%u) beyond %u", i, n.triangle_offset, n.triangle_count, nt);
        return PTMI_OK;
    };
    std::vector<uint32_t> wide_of(nn, PT_REF_NONE);
    std::vector<uint8_t> seen(nn, 0);
    struct Item { uint32_t node, depth; };
    std::vector<Item> stack;
    // pass 1: preorder (left first) numbering of the internal nodes
    stack.push_back({0u, 1u});
    uint32_t n_wide = 0, depth = 0, max_leaf_tris = 0;
    uint64_t next_offset = 0;               // leaves must come in ascending triangle order along the left-first DFS (below)
    while (!stack.empty()) {
        Item it = stack.back(); stack.pop_back();
        if (it.node >= nn) return fail(err, PTMI_E_INVALID, "BVH child index %u out of range (%u nodes)", it.node, nn);
        if (seen[it.node]) return fail(err, PTMI_E_INVALID, "BVH node %u is reachable twice", it.node);
        seen[it.node] = 1;
        depth = std::max(depth, it.depth);
        if (it.depth > 62) return fail(err, PTMI_E_UNSUPPORTED, "BVH deeper than 62 levels (the reference's own traversal stack holds 64 entries, pt.wgsl:249)");
        const ptmi_bvh_node &n = nodes[it.node];
        if (n.triangle_count > 0) {
            int rc = check_leaf(it.node); if (rc) return rc;
            // pt.wgsl:274 keeps the FIRST of equally near hits in its left-first DFS; the kernels visit leaves in another
            // order and break ties by the lowest triangle index. The two agree iff leaf ranges ascend along that DFS —
            // true of every tree bvh.ts builds (children split one contiguous range, left = lower part, bvh.ts:114-127).
            if (n.triangle_offset < next_offset)
                return fail(err, PTMI_E_UNSUPPORTED, "BVH leaf %u starts at triangle %u but an earlier leaf of the left-first DFS ends at %llu: "
                            "leaf ranges must ascend in DFS order (as bvh.ts builds them)", it.node, n.triangle_offset, (unsigned long long)next_offset);
            next_offset = (uint64_t)n.triangle_offset + n.triangle_count;
            max_leaf_tris = std::max(max_leaf_tris, n.triangle_count);
            continue;
        }
        wide_of[it.node] = n_wide++;
        stack.push_back({n.right, it.depth + 1});
        stack.push_back({n.left, it.depth + 1});
    }
    std::vector<float4> wnodes((size_t)n_wide * 4, make_float4(0, 0, 0, 0));
    auto ref_of = [&](uint32_t i) { return nodes[i].triangle_count > 0 ? leaf_ref(nodes[i]) : wide_of[i]; };
    for (uint32_t i = 0; i < nn; i++) {
        if (wide_of[i] == PT_REF_NONE) continue;
        const ptmi_bvh_node &L = nodes[nodes[i].left], &R = nodes[nodes[i].right];
        float4 *w = &wnodes[(size_t)wide_of[i] * 4];
        w[0] = make_float4(L.aabb_min[0], L.aabb_min[1], L.aabb_min[2], L.aabb_max[0]);
        w[1] = make_float4(L.aabb_max[1], L.aabb_max[2], R.aabb_min[0], R.aabb_min[1]);
        w[2] = make_float4(R.aabb_min[2], R.aabb_max[0], R.aabb_max[1], R.aabb_max[2]);
        uint32_t lr = ref_of(nodes[i].left), rr = ref_of(nodes[i].right);
        float fl, fr; std::memcpy(&fl, &lr, 4); std::memcpy(&fr, &rr, 4);
        w[3] = make_float4(fl, fr, 0.0f, 0.0f);
    }
    for (int k = 0; k < 3; k++) { b.ref_root_min[k] = nodes[0].aabb_min[k]; b.ref_root_max[k] = nodes[0].aabb_max[k]; }
    b.ref_root_ref = ref_of(0);
    // the header of the tree as uploaded: the image the kernels walk unless a hierarchy is built below
    ptmi_image_info &h = b.img;
    h.n_wnodes = n_wide; h.n_tris = nt; h.root_ref = b.ref_root_ref; h.depth = h.ref_depth = depth; h.max_leaf_tris = max_leaf_tris;
    for (int k = 0; k < 3; k++) { h.root_min[k] = b.ref_root_min[k]; h.root_max[k] = b.ref_root_max[k]; }
    // Nested tree (each node box contains its children's, all finite)? Then rebuild the hierarchy over the
    // reference's leaves (fast_tree.hip explains why the results cannot change).
    bool nested = n_wide > 0;
    std::vector<PtFastLeaf> leaves;
    for (uint32_t i = 0; i < nn && nested; i++) {
        if (!seen[i]) continue;
        const ptmi_bvh_node &n = nodes[i];
        for (int k = 0; k < 3; k++) nested = nested && std::isfinite(n.aabb_min[k]) && std::isfinite(n.aabb_max[k]);
        if (n.triangle_count > 0) {
            PtFastLeaf l;
            for (int k = 0; k < 3; k++) { l.mn[k] = n.aabb_min[k]; l.mx[k] = n.aabb_max[k]; }
            l.ref = leaf_ref(n); l.weight = n.triangle_count;
            leaves.push_back(l);
        } else {
            for (uint32_t ch : {n.left, n.right})
                for (int k = 0; k < 3; k++)
                    nested = nested && nodes[ch].aabb_min[k] >= n.aabb_min[k] && nodes[ch].aabb_max[k] <= n.aabb_max[k];
        }
    }
    const uint32_t leaves_mode = opt.leaves ? opt.leaves : (uint32_t)PT_LEAVES_DEFAULT;
    bool own = false;
    if (nested && leaves_mode == 2u && !opt.keep_reference_tree) {
        // The library's own leaves (fast_tree.h). What the reference's semantics need from the uploaded tree is kept beside them: the
        // tree itself (slow rays walk it) and, per triangle, the box of the leaf that lists it (the winner's verification).
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> which;
        which.reserve(nt);
        std::vector<float4> leafbox((size_t)nt * 2, make_float4(0, 0, 0, 0));
        for (const PtFastLeaf &l : leaves) {            // (leaf ranges ascend and do not overlap: checked above)
            const uint32_t first = l.ref & PT_LEAF_OFF_MASK;
            for (uint32_t k = 0; k < l.weight; k++) {
                which.push_back(first + k);
                leafbox[2 * (size_t)(first + k)] = make_float4(l.mn[0], l.mn[1], l.mn[2], 0.0f);
                leafbox[2 * (size_t)(first + k) + 1] = make_float4(l.mx[0], l.mx[1], l.mx[2], 0.0f);
            }
        }
        std::sort(which.begin(), which.end());
        const uint32_t k_max = opt.leaf_tris ? opt.leaf_tris : (uint32_t)PT_LEAF_TRIS_DEFAULT;
        // small scenes: at most 14 levels, so that a lane's whole node stack fits the 15 LDS entries of two workgroups per CU
        const uint32_t limit = which.size() <= 2048 ? 14u : 60u;
        // tree_builder = 2: on the device for scenes above 4 096 triangles. Smaller scenes keep the host builder (a few ms): they get the
        // 16-bit images, and which of the LDS variants fits them turns on a few tens of nodes (cornell_spheres: the host tree has 2 038,
        // within the 2 046 of the quantised 16-bit variant; the device tree 2 109). Also on the host: without a device (the host-only
        // debug entry points) and when the device build fails
        PtOwnTreeGpu g;
        PtOwnTree t;
        const bool on_device = opt.tree_builder == 2u && stream && nt > 4096u && which.size() > 2048u &&
                               own_tree_on_device(stream, device, tris, nt, which, leafbox, k_max, limit, b, g);
        own = on_device || pt_build_own_tree(tris, which, leafbox, k_max, limit, t);
        if (own) own_image(b, on_device, device, g, t, nt, wnodes, std::move(leafbox));
        b.tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    std::vector<float4> fast;                   // a hierarchy rebuilt over the reference's leaves
    if (nested && leaves.size() >= 2 && !opt.keep_reference_tree && !own) {
        const auto t0 = std::chrono::steady_clock::now();
        // tree_builder = 2: on the device (gpu_tree.hip); the host builder when that is not wanted, not possible (ptmi_debug_image_stats
        // has no device) or refused
        uint32_t root = PT_REF_NONE, fast_depth = 0;
        const bool on_device = opt.tree_builder == 2u && stream && pt_build_fast_tree_gpu(leaves, fast, root, fast_depth, stream);
        if (!on_device) pt_build_fast_tree(leaves, fast, root, fast_depth);
        h.n_wnodes = (uint32_t)(fast.size() / 4); h.root_ref = root; h.depth = fast_depth;
        b.tree_builder_used = on_device ? 2u : 1u;
        b.tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // triangle images: v0, e1 = v1 - v0, e2 = v2 - v0 (pt.wgsl:128-129; one IEEE subtraction each)
    std::vector<float4> tripos((size_t)nt * 3);
    for (uint32_t i = 0; i < nt; i++) {
        const ptmi_triangle &t = tris[i];
        tripos[3 * (size_t)i + 0] = make_float4(t.v0[0], t.v0[1], t.v0[2], 0.0f);
        tripos[3 * (size_t)i + 1] = make_float4(t.v1[0] - t.v0[0], t.v1[1] - t.v0[1], t.v1[2] - t.v0[2], 0.0f);
        tripos[3 * (size_t)i + 2] = make_float4(t.v2[0] - t.v0[0], t.v2[1] - t.v0[1], t.v2[2] - t.v0[2], 0.0f);
    }
    {   // longest edge squared, in double; NaN / inf edges give 0 (no ray is "bounded" then)
        double emax2 = 0.0; bool finite = true;
        for (size_t k = 0; k < tripos.size(); k++) {
            if (k % 3 == 0) continue;
            const float4 &e = tripos[k];
            const double l2 = (double)e.x * e.x + (double)e.y * e.y + (double)e.z * e.z;
            if (!(l2 <= 1.7e308)) finite = false; else if (l2 > emax2) emax2 = l2;
        }
        const double k = !finite ? 0.0 : (emax2 > 0.0 ? std::ldexp(1.0, 98) / emax2 : 3.0e38);
        b.tri_safe_dsum = (float)(k < 3.0e38 ? k : 3.0e38);
    }
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint4> q;
        std::vector<uint32_t> leaf_stream;
        if (!fast.empty() && pt_quantize_tree(leaves, fast, tripos, q, leaf_stream, h.q_origin, h.q_scale, PT_QCACHE_NODES, b.q_top)) {
            h.quantised = 1u;
            b.hold(kQnodes, std::move(q)); b.hold(kLeafStream, std::move(leaf_stream));
        }
        b.tree_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (!fast.empty()) b.hold(kWnodes, std::move(fast));
    b.hold(kRefWnodes, std::move(wnodes)); b.hold(kRefTripos, std::move(tripos));
    return PTMI_OK;
}

// bytes of the walked image in LDS (nodes and triangle images)
size_t lds_scene_bytes(const ptmi_ctx *c) { return (size_t)c->img.n_wnodes * 64 + (size_t)c->img.n_tris * 48; }
// ptmi_stats.bvh_depth: levels of the uploaded tree, or of the hierarchy rebuilt over its leaves where that is deeper
uint32_t stats_depth(const ptmi_ctx *c) { return c->img.leaves_used == 2u ? c->img.ref_depth : std::max(c->img.depth, c->img.ref_depth); }

// Sizes `variant` (pt_variant) on the uploaded scene with `wgs` workgroups per CU: the per-lane stack, whether it spills, the LDS it
// launches with. False: it does not fit, or the scene has no image in its node format.
bool size_variant(const ptmi_ctx *c, int variant, int wgs, TraverseConfig &cfg) {
    const PtVariant &r = pt_variant(variant);
    const uint32_t depth = std::max(c->img.depth, c->img.ref_depth);    // slow rays walk the uploaded tree on the same stacks
    int entries = 0;
    bool ok = true;
    switch (r.stack) {
    case PT_STACK_DEPTH: entries = depth + 2 <= 16 ? 16 : depth + 2 <= 32 ? 32 : 0; ok = wgs == 1 && entries != 0; break;
    case PT_STACK_NODES: entries = wgs == 2 ? 15 : 16; ok = wgs == 1 || (wgs == 2 && depth + 1 <= 15); break;
    case PT_STACK_SPILL: entries = 16; ok = wgs == 1; break;
    case PT_STACK_16BIT: entries = 15; ok = wgs == 2 && depth + 1 <= 15; break;
    case PT_STACK_16BIT_SPILL: {
        // the 16-bit entries (2 KB each per workgroup) take what the quantised nodes leave of a CU's half
        const size_t nq = (size_t)c->sc.n_wnodes * 32;
        entries = (c->sc.qnodes16 && nq + 64 < kLdsMax / 2) ? std::min<int>(15, (int)((kLdsMax / 2 - 64 - nq) / 2048)) : 0;
        if (const char *e = std::getenv("PTMI_OWN_Q16_ENTRIES"))      // tests: a shorter stack than fits (more spills), never below 8
            entries = std::min(entries, std::max(8, std::atoi(e)));
        ok = wgs == 2 && entries >= 8;
        break;
    }
    }
    ok = ok && (!pt_quantised(r) || (c->sc.own && c->img.quantised)) && (r.nodes != PT_NODES_EXACT16 || c->sc.wnodes16 != nullptr);
    cfg.variant = variant; cfg.wgs_per_cu = wgs; cfg.stack_entries = entries;
    cfg.wants_spill = pt_spills(r, wgs) ? 1 : 0;
    cfg.quantized = pt_quantised(r) ? 1 : 0;
    cfg.lds_bytes = pt_lds_bytes(r, c->sc.n_wnodes, c->sc.own ? c->sc.n_own_tris : c->sc.n_tris, entries);
    return ok && cfg.lds_bytes <= kLdsMax / (size_t)wgs;
}

// Which memory variant a traversal kernel runs as (closest_hit: the extend kernel, else the any-hit kernel). PTMI_OWN_EXTEND /
// PTMI_OWN_SHADOW (a code as ptmi_stats reports it, pt_variant_code: 102 = PT_VARIANT_OWN_LDS16_NODES, two workgroups per CU) override
// the choice of the own-leaf variants where it fits — for same-box A/Bs, not for users.
TraverseConfig traverse_config(const ptmi_ctx *c, bool closest_hit) {
    const bool own = c->sc.own, big = lds_scene_bytes(c) > ((size_t)4 << 20);       // big: beyond an XCD's L2
    const int traversal = c->opt.traversal;
    TraverseConfig cfg{};
    cfg.cull = c->opt.cull ? 1 : 0;
    auto pick = [&](int variant, int wgs) { return size_variant(c, variant, wgs, cfg); };
    // The quantised image pays where node fetches leave the L2 (measured: the 1 M-triangle scene, 67 MB, extend -16 %); a scene
    // that an XCD's 4 MiB L2 holds is bound by the ALUs, and decoding costs more than the bytes save (cornell_spheres walked
    // from global memory: shadow +30 %). AUTO decides by size; GLOBAL asks for the quantised image, GLOBAL_EXACT for the exact one.
    const bool mem_quant = traversal == PTMI_TRAVERSAL_GLOBAL || (traversal == PTMI_TRAVERSAL_AUTO && big);
    auto from_memory = [&]() {
        if (!own) { pick(PT_VARIANT_GLOBAL, 1); cfg.quantized = mem_quant; cfg.wgs_per_cu = 2; }  // (2: the code leaves = 1 has always reported)
        else pick(c->img.quantised && mem_quant ? PT_VARIANT_OWN_QGLOBAL : PT_VARIANT_OWN_GLOBAL, 1);
        return cfg;
    };
    if (traversal == PTMI_TRAVERSAL_GLOBAL || traversal == PTMI_TRAVERSAL_GLOBAL_EXACT) return from_memory();
    if (own && traversal == PTMI_TRAVERSAL_AUTO)
        if (const char *e = std::getenv(closest_hit ? "PTMI_OWN_EXTEND" : "PTMI_OWN_SHADOW")) {
            int code = std::atoi(e);
            // (the earlier short form, below every own-leaf code: 1 - 9 a variant with one workgroup per CU, + 10 with two; 20 / 21
            // variants 10 / 11 with two)
            if (code < 40) code = code == 20 ? 102 : code == 21 ? 112 : (code % 10) * 10 + (code >= 10 ? 2 : 1);
            if (pt_variant(code / 10).own && pick(code / 10, code % 10)) return cfg;
        }
    struct Pick { int variant, wgs; };
    // Own leaves: both kernels are box-step heavy (7 - 8 dependent node fetches per ray against 3 - 4 triangle tests) and gain from the
    // second workgroup per CU — 8 waves per SIMD to cover them — more than from resident triangles (config 1, same box: any-hit kernel
    // from two workgroups with quantised nodes 17.1 ms beside the main stream against 21.1 from the full image, +2 % overall)
    static const Pick own_auto[] = {{PT_VARIANT_OWN_LDS_NODES, 2}, {PT_VARIANT_OWN_LDS16_NODES, 2}, {PT_VARIANT_OWN_QLDS_NODES, 2},
                                    {PT_VARIANT_OWN_QLDS16_NODES, 2}, {PT_VARIANT_OWN_LDS, 1}, {PT_VARIANT_OWN_QLDS, 1},
                                    {PT_VARIANT_OWN_QLDS_NODES, 1}, {PT_VARIANT_OWN_LDS_NODES, 1}};
    static const Pick own_lds[] = {{PT_VARIANT_OWN_LDS, 1}, {PT_VARIANT_OWN_QLDS, 1}};
    // The reference's leaves: the any-hit kernel keeps the full LDS image, one workgroup per CU. From the node cache with two
    // workgroups (80 scalar registers since round 2) it is as fast by itself (8.53 ms per 64 spp either way) but takes every wave slot
    // of its CUs: beside it `shade` stretches from 16.5 to 18.3 ms and config 1 loses 4 % (9 767 -> 9 344); with one workgroup it is
    // 40 % slower itself. Mid-size trees (up to 1536 wide nodes, the last pick): all nodes in LDS, one workgroup per CU, stacks
    // spill; measured on cornell_spheres against the global variant: extend -6 %, shadow +5 % (so closest hit only).
    static const Pick ref_closest[] = {{PT_VARIANT_LDS_NODES, 2}, {PT_VARIANT_LDS, 1}, {PT_VARIANT_LDS_NODES, 1}};
    static const Pick ref_lds[] = {{PT_VARIANT_LDS, 1}};
    auto all = [](const auto &l) { return std::make_pair(std::begin(l), std::end(l)); };
    const auto picks = traversal == PTMI_TRAVERSAL_LDS ? (own ? all(own_lds) : all(ref_lds))
                     : own ? (big ? std::make_pair(own_auto, own_auto) : all(own_auto)) : closest_hit ? all(ref_closest) : all(ref_lds);
    if (own || c->sc.root_ref != PT_REF_NONE)                       // (an empty scene with the reference's leaves: the global variant)
        for (const Pick *p = picks.first; p != picks.second; p++)
            if (pick(p->variant, p->wgs)) {
                if (p->variant == PT_VARIANT_LDS) cfg.wgs_per_cu = 2;  // (the code leaves = 1 has always reported)
                return cfg;
            }
    return from_memory();                   // PTMI_TRAVERSAL_LDS: the caller reports that the scene does not fit
}

// the radiance sits at 16-byte stride beside kernels that wait on node fetches from memory (pt_device.h DevPaths)
bool walks_memory_quantised(const TraverseConfig &cfg) {
    return cfg.quantized && pt_variant(cfg.variant).where == PT_FROM_MEMORY;
}

constexpr uint32_t kAovAll = PTMI_AOV_ALBEDO | PTMI_AOV_NORMAL | PTMI_AOV_ID;

// One row per FramePlane: its size for px pixels, whether it is zero-filled when made, and when it is made: with the frame (ptmi_resize
// and the call that turns it on), or by the first call that needs it since the last resize.
enum PlaneGroup { kWithFrame, kByDenoise, kByAdaptive, kByReproject, kByBlit };
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
    {"adaptive tile sums", tile_sum_bytes, false, kByAdaptive},
    {"output history", per_pixel<PTMI_OUTPUT_STRIDE>, false, kByReproject}, {"moments history", per_pixel<16>, false, kByReproject},
    {"normal history", per_pixel<16>, false, kByReproject}, {"albedo history", per_pixel<16>, false, kByReproject},
    {"id history", per_pixel<8>, false, kByReproject},
    {"float canvas", per_pixel<16>, false, kByBlit}, {"8-bit canvas", per_pixel<4>, false, kByBlit},
};
// sets of planes: a bit per FramePlane
constexpr uint32_t kAllPlanes = (1u << kFramePlanes) - 1u;
constexpr uint32_t bit(FramePlane k) { return 1u << k; }
static_assert(PTMI_AOV_ALBEDO << kAovAlbedo == bit(kAovAlbedo) && PTMI_AOV_NORMAL << kAovAlbedo == bit(kAovNormal) &&
              PTMI_AOV_ID << kAovAlbedo == bit(kAovId), "an AOV mask, shifted, is its set of planes");
uint32_t group_set(PlaneGroup g) {
    uint32_t set = 0;
    for (int k = 0; k < kFramePlanes; k++) if (kFrame[k].group == g) set |= 1u << k;
    return set;
}
// the planes that exist whenever the output buffer does: the output, the AOV planes of the mask, the moments plane while on
uint32_t frame_set(const ptmi_ctx *c) { return bit(kOut) | c->aov_mask << kAovAlbedo | (c->moments_on ? bit(kMoments) : 0u); }
// which: one PTMI_AOV_* bit (else kFramePlanes)
FramePlane aov_plane_of(uint32_t which) {
    return which == PTMI_AOV_ALBEDO ? kAovAlbedo : which == PTMI_AOV_NORMAL ? kAovNormal : which == PTMI_AOV_ID ? kAovId : kFramePlanes;
}
template <class T> T *plane_as(const ptmi_ctx *c, FramePlane k) { return static_cast<T *>(c->plane[k]); }
void view_planes(ptmi_ctx *c) {
    view(c->ad.ballot, c->plane[kAdBallot]); view(c->ad.list, c->plane[kAdList]); view(c->ad.tile_sums, c->plane[kAdTileSums]);
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

// Frees the context's planes of `set` (the caller has synchronised where one may be in use).
void drop_planes(ptmi_ctx *c, uint32_t set) {
    for (int k = 0; k < kFramePlanes; k++) if (set & 1u << k) dfree(c->plane[k]);
    view_planes(c);
}

// Copies a whole plane to the host once everything in flight has finished. src: the plane, or the buffer bound in its place. n: the
// caller's count of `unit`-byte elements (4: floats, 1: bytes), which must be the plane's.
int read_plane(ptmi_ctx *c, FramePlane k, const void *src, void *dst, size_t n, size_t unit) {
    const size_t bytes = kFrame[k].bytes((size_t)c->W * c->H);
    if (n * unit != bytes) return fail(c, PTMI_E_INVALID, "expected %zu %s, got %zu", bytes / unit, unit == 4 ? "floats" : "bytes", n);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

// the control words live for the context's life (ptmi_get_stats reads acc[0]); the planes follow the output buffer's size
int adaptive_words(ptmi_ctx *c) {
    if (!c->ad.ctl) {
        HIP_TRY(c, hipMalloc(&c->ad.ctl, 4 * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(c->ad.ctl, 0, 4 * sizeof(uint32_t)));
    }
    if (!c->ad.acc) {
        HIP_TRY(c, hipMalloc(&c->ad.acc, 4 * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(c->ad.acc, 0, 4 * sizeof(unsigned long long)));
    }
    return PTMI_OK;
}
// a fresh moments plane (ptmi_resize, ptmi_set_moments): no round has listed anything in it
int reset_adaptive_rounds(ptmi_ctx *c) {
    if (c->ad.ctl) HIP_TRY(c, hipMemset(c->ad.ctl, 0, 4 * sizeof(uint32_t)));
    c->ad_rounds = 0;
    return PTMI_OK;
}

int check_ready(ptmi_ctx *c, bool need_output) {
    if (!c) return PTMI_E_INVALID;
    if (!c->have_scene) return fail(c, PTMI_E_STATE, "no scene uploaded (ptmi_upload_scene)");
    if (need_output && (!c->d_out || c->W == 0 || c->H == 0)) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    return PTMI_OK;
}

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

}  // namespace

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
float4 *pt_ctx_output(ptmi_ctx *c) { return c->d_out; }
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
        ok = ok && hipMalloc(&ln.counts, 80 * sizeof(uint32_t)) == hipSuccess;
        if (!ok) { ptmi_destroy(c); return fail(nullptr, PTMI_E_HIP, "stream / event creation failed"); }
    }
    if (hipMalloc(&c->d_stats, kStatsWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->d_scene, sizeof(DevScene)) != hipSuccess || hipMemset(c->d_scene, 0, sizeof(DevScene)) != hipSuccess ||
        hipMemset(c->d_stats, 0, kStatsWords * sizeof(unsigned long long)) != hipSuccess) {
        ptmi_destroy(c); return fail(nullptr, PTMI_E_HIP, "device allocation failed");
    }
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
        dfree(ln.counts); dfree(ln.d_spill); dfree(ln.d_spill_side);
        for (hipEvent_t e : {ln.ev_ready, ln.ev_shadow[0], ln.ev_shadow[1]}) if (e) (void)hipEventDestroy(e);
        if (ln.side) (void)hipStreamDestroy(ln.side);
    }
    for (void *&p : c->buf) dfree(p);
    dfree(c->d_atlas);
    drop_planes(c, kAllPlanes);
    dfree(c->d_stats); dfree(c->d_scene); dfree(c->ad.ctl); dfree(c->ad.acc); dfree(c->d_reproject);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return PTMI_OK;
}

}  // extern "C"

// A scene prepared on the host (validation + traversal image: everything of an upload that does not depend on the device), and the
// caller's blobs it was made from. ptmi_upload_scene = prepare + install; ptmi_multi_upload_scene prepares ONCE and installs on N devices.
struct PtPrepared {
    Built b;                                 // the triangles, materials and lights included
    uint32_t nt, nm, nl;
    double build_ms;
    bool take_device_buffers = false;        // the one install may take b's device buffers instead of copying them (single device)
};

// The shade tables of a scene (pt_device.h): raw copies of the uploaded records, in the order k_shade stages them.
static std::vector<float4> shade_tables(const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                                        const ptmi_light *lights, uint32_t nl) {
    std::vector<float4> tab(pt_tab_mats_q(nm) + pt_tab_lights_q(nl), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    char *at = reinterpret_cast<char *>(tab.data());
    if (nm) std::memcpy(at, mats, (size_t)nm * sizeof(ptmi_material));
    at += pt_tab_mats_q(nm) * sizeof(float4);                                   // (behind the materials: the material of zeros)
    if (nl) std::memcpy(at, lights, (size_t)nl * sizeof(ptmi_light));
    at += (size_t)nl * sizeof(ptmi_light);
    for (uint32_t i = 0; i < nl; i++)
        if (lights[i].light_type == PTMI_LIGHT_EMISSIVE && lights[i].triangle_index < nt)
            std::memcpy(at + (size_t)i * sizeof(ptmi_triangle), &tris[lights[i].triangle_index], sizeof(ptmi_triangle));
    return tab;
}

PtPrepared *pt_prepare_scene(ptmi_ctx *c, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                             const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl, int *rc_out) {
    auto bad = [&](int rc) -> PtPrepared * { *rc_out = rc; return nullptr; };
    if (!c) return bad(PTMI_E_INVALID);
    if ((nt && !tris) || (nm && !mats) || (nn && !nodes) || (nl && !lights))
        return bad(fail(c, PTMI_E_INVALID, "NULL blob with a non-zero count"));
    if (hipSetDevice(c->device) != hipSuccess) return bad(fail(c, PTMI_E_HIP, "hipSetDevice(%d) failed", c->device));
    for (uint32_t i = 0; i < nl; i++) {
        if (lights[i].light_type > PTMI_LIGHT_POINT)
            return bad(fail(c, PTMI_E_INVALID, "light %u has unknown type %u", i, lights[i].light_type));
        if (lights[i].light_type == PTMI_LIGHT_EMISSIVE && lights[i].triangle_index >= nt)
            return bad(fail(c, PTMI_E_INVALID, "emissive light %u references triangle %u of %u", i, lights[i].triangle_index, nt));
    }
    const auto t_start = std::chrono::steady_clock::now();
    PtPrepared *p = new PtPrepared();
    int rc = build_image(c->opt, c->stream, c->device, tris, nt, nodes, nn, p->b, c->err);
    if (rc) { delete p; return bad(rc); }
    if (!p->b.buf[kTris].present) p->b.view(kTris, tris, (size_t)nt * sizeof(ptmi_triangle));     // (else the device copy)
    p->b.view(kMats, mats, (size_t)nm * sizeof(ptmi_material));
    p->b.view(kLights, lights, (size_t)nl * sizeof(ptmi_light));
    p->b.hold(kShadeTab, shade_tables(tris, nt, mats, nm, lights, nl));
    p->nt = nt; p->nm = nm; p->nl = nl;
    p->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    *rc_out = PTMI_OK;
    return p;
}
void pt_free_prepared(PtPrepared *p) { delete p; }

int pt_install_scene(ptmi_ctx *c, PtPrepared *prep) {
    if (!c || !prep) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    const auto t_start = clk::now();
    Built &b = prep->b;
    // Allocate and fill the new buffers first; the context keeps its previous scene until all of them exist. An empty buffer gets 16
    // zeroed bytes. Buffers the preparation made on a device are taken over (the one install on that device) or copied.
    const auto t_copy = clk::now();
    void *n[kSceneBufs] = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < kSceneBufs && e == hipSuccess; k++) {
        HeldBuf &h = b.buf[k];
        if (!h.present) continue;
        if (h.dev && prep->take_device_buffers && h.device == c->device) { n[k] = h.dev; h.dev = nullptr; continue; }
        e = hipMalloc(&n[k], h.bytes ? h.bytes : 16);
        if (e != hipSuccess) break;
        if (h.dev) e = h.device == c->device ? hipMemcpy(n[k], h.dev, h.bytes, hipMemcpyDeviceToDevice)
                                             : hipMemcpyPeer(n[k], c->device, h.dev, h.device, h.bytes);
        else e = h.bytes ? hipMemcpy(n[k], h.host, h.bytes, hipMemcpyHostToDevice) : hipMemset(n[k], 0, 16);
    }
    if (e != hipSuccess) {
        for (void *&p : n) dfree(p);
        return fail(c, PTMI_E_HIP, "scene upload failed: %s (the previous scene, if any, is still in place)", hipGetErrorString(e));
    }
    HIP_TRY(c, sync_all(c));                  // nothing in flight reads the old buffers any more
    for (int k = 0; k < kSceneBufs; k++) { dfree(c->buf[k]); c->buf[k] = n[k]; }
    void *const *d = c->buf;
    const ptmi_image_info &h = b.img;
    const bool own = h.leaves_used == 2u;
    DevScene &s = c->sc;
    s.tris = static_cast<const ptmi_triangle *>(d[kTris]); s.n_tris = prep->nt;
    s.mats = static_cast<const ptmi_material *>(d[kMats]); s.n_mats = prep->nm;
    s.lights = static_cast<const ptmi_light *>(d[kLights]); s.n_lights = prep->nl;
    s.ref_wnodes = static_cast<const float4 *>(d[kRefWnodes]); s.ref_root_ref = b.ref_root_ref; s.has_fast = d[kWnodes] ? 1u : 0u;
    s.wnodes = static_cast<const float4 *>(walked(d, kWnodes));
    s.n_wnodes = h.n_wnodes;
    s.tripos = static_cast<const float4 *>(walked(d, kTripos));
    s.ref_tripos = static_cast<const float4 *>(d[kRefTripos]);
    s.qnodes = static_cast<const uint4 *>(d[kQnodes]); s.leaf_stream = static_cast<const uint32_t *>(d[kLeafStream]);
    for (int k = 0; k < 3; k++) { s.q_origin[k] = h.q_origin[k]; s.q_scale[k] = h.q_scale[k]; }
    s.q_cached = b.q_top;
    s.tri_safe_dsum = b.tri_safe_dsum;
    for (int k = 0; k < 3; k++) {
        s.ref_root_min[k] = b.ref_root_min[k]; s.ref_root_max[k] = b.ref_root_max[k];
        s.root_min[k] = h.root_min[k]; s.root_max[k] = h.root_max[k];
    }
    s.root_ref = h.root_ref;
    s.own = own ? 1u : 0u;
    s.n_own_tris = own ? h.n_tris : 0u;
    s.tri_leafbox = static_cast<const float4 *>(d[kLeafbox]);
    s.wnodes16 = static_cast<const float4 *>(d[kWnodes16]); s.ref_wnodes16 = static_cast<const float4 *>(d[kRefWnodes16]);
    s.qnodes16 = static_cast<const uint4 *>(d[kQnodes16]);
    s.root_ref16 = b.root_ref16; s.ref_root_ref16 = b.ref_root_ref16;
    s.safe_origin = h.safe_origin;
    s.verify_stat = c->d_stats + 4;
    s.self = c->d_scene;
    s.shade_tab = static_cast<const float4 *>(d[kShadeTab]);
    HIP_TRY(c, hipMemcpy(c->d_scene, &c->sc, sizeof(DevScene), hipMemcpyHostToDevice));
    c->img = h;
    c->have_scene = true;
    c->st.leaves_used = h.leaves_used;
    c->st.leaf_tris_used = h.max_leaf_tris;
    c->st.tree_builder_used = b.tree_builder_used;
    c->st.upload_copy_ms = ms_since(t_copy);
    c->st.upload_tree_ms = b.tree_ms;
    c->st.upload_ms = prep->build_ms + ms_since(t_start);
    return PTMI_OK;
}

extern "C" {

int ptmi_upload_scene(ptmi_ctx *c, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                      const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl) {
    int rc = PTMI_OK;
    PtPrepared *p = pt_prepare_scene(c, tris, nt, mats, nm, nodes, nn, lights, nl, &rc);
    if (!p) return rc;
    p->take_device_buffers = true;
    rc = pt_install_scene(c, p);
    pt_free_prepared(p);
    return rc;
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
// length of the call both exist, at most 72 B per pixel of the new size (output, three AOV planes, moments), small beside a batch.
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
    drop_planes(c, kAllPlanes);                       // the denoiser's, the adaptive, the history and the blit planes come back at their first use
    std::copy(fresh, fresh + kFramePlanes, c->plane);
    c->W = w; c->H = h;
    c->d_out = plane_as<float4>(c, kOut);
    return reset_adaptive_rounds(c);
}

int ptmi_set_options(ptmi_ctx *c, const ptmi_options *o) {
    if (!c || !o) return PTMI_E_INVALID;
    if (o->max_bounces < 1 || o->max_bounces > 64) return fail(c, PTMI_E_INVALID, "max_bounces %u not in 1..64", o->max_bounces);
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

namespace {

// ptmi_dispatch (ap NULL: n_frames frames of every pixel of the band, from cam->frame_index) and ptmi_dispatch_adaptive (ap: `rounds`
// rounds of ap->step frames for the listed pixels, each from its own count). Both run the same bounce loop per batch; they differ in
// the raygen in front of it and the folds behind it.
int dispatch(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n_frames, const ptmi_adaptive_params *ap, uint32_t rounds) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!cam) return fail(c, PTMI_E_INVALID, "camera is NULL");
    if (cam->width != c->W || cam->height != c->H)
        return fail(c, PTMI_E_INVALID, "camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
    if (n_frames == 0 || (ap && rounds == 0)) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (ap && ((rc = adaptive_words(c)) || (rc = make_planes(c, group_set(kByAdaptive), (size_t)c->W * c->H, c->plane)))) return rc;
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    if (band.y0 >= band.y1) return fail(c, PTMI_E_INVALID, "tile rows [%u,%u) outside the %u-row frame", band.y0, band.y1, c->H);
    if (band.rows == 0) return PTMI_OK;                         // more parts than strips: nothing to render here
    const uint64_t npix = (uint64_t)band.rows * band.width;
    uint32_t F = c->opt.frames_per_batch;
    // ~128 Mi paths, ~23 GB of state: the last bounces' small queues cost a fixed ~3 ms per batch, so fewer, larger batches
    // (measured at 1080p, Msamples/s: 32 frames 8 920, 64 frames 9 150 - 9 275, 128 frames 9 270 - 9 310)
    const bool auto_F = F == 0;
    Lane &ln = c->lane;
    if (auto_F) {
        F = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, (128ull << 20) / npix));
        // ... but never more than the device has room for: several contexts may share one device (ranks rehearsed on one GPU, a
        // Node host beside another process), and eight ranks of one node each size their batch by what THEIR device has free.
        // Room = free memory + what this context already holds, less a tenth for the rest (spill areas, blit staging).
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t held = (uint64_t)ln.cap * bytes_per_path(ln.aov != nullptr);
            const uint64_t room = (uint64_t)((double)(free_b + held) * 0.9);
            F = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(F, room / (npix * bytes_per_path(c->aov_mask != 0))));
        }
    }
    F = std::min(F, n_frames);
    const bool nee = c->opt.do_mis && c->sc.n_lights > 0;
    // overlap: `shadow` of bounce b on a side stream, beside extend / shade of bounce b + 1. It is then the only kernel that
    // adds to L (emissive hits leave a record too, ShadeParams::emit_records), bounce after bounce on one stream, so every
    // path's sum is formed in the same order as without it. Record buffers alternate by bounce parity; shade(b) waits for
    // shadow(b - 2), the end of the batch for the last one.
    const bool side = nee && c->opt.overlap != 0;
    if (npix * F > 0xFFFFFF00ull) return fail(c, PTMI_E_UNSUPPORTED, "batch of %llu paths exceeds 2^32", (unsigned long long)(npix * F));
    const TraverseConfig cfg0 = traverse_config(c, true), cfg_shadow0 = traverse_config(c, false);
    if (c->opt.traversal == PTMI_TRAVERSAL_LDS && pt_variant(cfg0.variant).where != PT_LDS_ALL)
        return fail(c, PTMI_E_UNSUPPORTED, "scene needs %zu B of LDS plus the stack; it does not fit in %zu B", lds_scene_bytes(c), kLdsMax);
    for (;;) {
        rc = ensure_capacity(c, ln, (size_t)(npix * F));
        if (rc == PTMI_OK) break;
        // out of device memory with a batch size the library chose: halve it and try again (hipMemGetInfo is a snapshot; another
        // context may have allocated since). A size the caller asked for fails loudly.
        if (!auto_F || !c->alloc_oom || F <= 1) return rc;
        F = (F + 1) / 2;
    }
    if (cfg0.wants_spill && !ln.d_spill) HIP_TRY(c, hipMalloc(&ln.d_spill, pt_spill_bytes(c->n_cu * 8)));          // 128 MiB on 256 CUs
    if (cfg_shadow0.wants_spill && !ln.d_spill_side) HIP_TRY(c, hipMalloc(&ln.d_spill_side, pt_spill_bytes(c->n_cu * 8)));
    c->st.traversal_used = pt_variant(cfg0.variant).where == PT_FROM_MEMORY ? PTMI_TRAVERSAL_GLOBAL : PTMI_TRAVERSAL_LDS;
    c->st.extend_variant = pt_variant_code(cfg0);
    c->st.shadow_variant = pt_variant_code(cfg_shadow0);
    c->st.frames_per_batch_used = F;
    c->st.radiance_stride_bytes = (walks_memory_quantised(cfg0) || walks_memory_quantised(cfg_shadow0)) ? 16u : 12u;
    c->st.shade_tables = PT_SHADE_LDS_BUDGET | ((uint32_t)pt_shade_stage(c->sc.n_mats, c->sc.n_lights) << 28);
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
        Timed td(c, 0, t1);
        const hipStream_t ms = c->stream;                                         // the bounce loop's stream
        const hipStream_t ss = side ? ln.side : ms;                               // ... and the shadow kernels'
        const int tiles = (int)(ln.cap / pt_compact_tile_slots() + 1);
        TraverseConfig cfg = cfg0, cfg_shadow = cfg_shadow0;
        cfg.spill = ln.d_spill; cfg_shadow.spill = side ? ln.d_spill_side : ln.d_spill;
        if (cfg_shadow.wants_spill && !cfg_shadow.spill) cfg_shadow.spill = ln.d_spill_side;
        ln.paths.l_stride = c->st.radiance_stride_bytes / 4u;
        const DevPaths bp = ln.paths;
        // Once per batch, after the compaction of the first bounce that plays roulette, the survivors' O / D / C are gathered into the
        // tail arrays at their queue positions: from then on a few percent of the paths are alive, and state left at the path id costs
        // them a line per lane in each stream. From the next bounce on, extend and shade find the state at the slot the queue names
        // and shade writes it back there; the radiance and the records keep the path id (ln.pid).
        const uint32_t rb = PT_REPACK ? pt_repack_bounce() : 0xFFFFFFFEu;
        DevPaths tp = ln.tail;
        tp.L = bp.L; tp.l_stride = bp.l_stride;
        float4 *const aov_rec = c->aov_mask ? ln.aov : nullptr;         // written by shade(0), read by the fold after the last bounce
        float4 *const mom = plane_as<float4>(c, kMoments);
        if (ap && cam->frame_index == 0u) { pt_launch_adaptive_restart(ms, blocks, band, mom); c->ad_rounds = 0; }
        // a batch: fb frames of every pixel from frame0 on, or (ap) of every listed pixel from its own count on
        auto batch = [&](uint32_t frame0, uint32_t fb) -> int {
            const DevPixels px = ap ? DevPixels{band, 0u, c->ad.list, &c->ad.ctl[1], mom, c->ad.acc}
                                    : DevPixels{band, frame0, nullptr, nullptr, nullptr, nullptr};
            { Timed t(c, 4, t3, ms); pt_launch_raygen(ms, blocks, *cam, px, fb, bp, &ln.counts[0]); }
            int cur = 0;
            for (uint32_t b = 0; b < maxb; b++) {
                const bool tail = b > rb;                                   // the state is in the tail arrays
                const uint32_t *q = b == 0 || b == rb + 1 ? nullptr : ln.queue[cur];   // bounce 0 / after the repack: slot i holds path / state i
                const DevPaths sp = tail ? tp : bp;
                const int par = side ? (int)(b & 1u) : 0;
                const ShadeParams shp{b, maxb, c->opt.do_mis, c->d_stats, side ? 1u : 0u, tail ? ln.pid : nullptr};
                { Timed t(c, 1, t2, ms); (c->sc.own ? pt_launch_extend_own : pt_launch_extend)(ms, blocks, cfg, c->sc, sp, q, &ln.counts[b], ln.hits); }
                const bool last = b + 1 == maxb;
                if (side && b >= 2) HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[par], 0));      // its records are read
                { Timed t(c, 2, t3, ms);
                  (c->opt.perf_mode ? pt_launch_shade_fast : pt_launch_shade)(
                      ms, shade_blocks, c->sc, sp, q, &ln.counts[b], ln.hits, ln.sh[par], ln.alive, ln.shadowm, shp,
                      b == 0 ? aov_rec : nullptr); }
                { Timed t(c, 5, t3, ms);
                  pt_launch_compact(ms, tiles, q, &ln.counts[b], ln.alive, nee ? ln.shadowm : nullptr,
                                    ln.word_off, ln.queue[cur ^ 1], &ln.counts[b + 1], ln.sq[par], &ln.counts[kShadowCount + par],
                                    c->d_stats, b, last ? 0 : 1);
                  if (b == rb && !last) pt_launch_repack(ms, blocks, &ln.counts[b + 1], ln.queue[cur ^ 1], bp, tp, ln.pid); }
                if (side) {
                    HIP_TRY(c, hipEventRecord(ln.ev_ready, ms));
                    HIP_TRY(c, hipStreamWaitEvent(ss, ln.ev_ready, 0));
                    { Timed t(c, 3, t3, ss);
                      (c->sc.own ? pt_launch_shadow_own : pt_launch_shadow)(ss, blocks, cfg_shadow, c->sc, bp, ln.sh[par], ln.sq[par],
                                                                            &ln.counts[kShadowCount + par], nullptr); }
                    HIP_TRY(c, hipEventRecord(ln.ev_shadow[par], ss));
                } else if (nee) {
                    Timed t(c, 3, t3, ms);
                    (c->sc.own ? pt_launch_shadow_own : pt_launch_shadow)(ms, blocks, cfg_shadow, c->sc, bp, ln.sh[0], ln.sq[0], &ln.counts[kShadowCount], nullptr);
                }
                cur ^= 1;
            }
            // all additions to L are in before it is folded
            if (side) {
                HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[(maxb - 1) & 1u], 0));
                if (maxb >= 2) HIP_TRY(c, hipStreamWaitEvent(ms, ln.ev_shadow[maxb & 1u], 0));
            }
            Timed t(c, 6, t3, ms);
            pt_launch_accumulate(ms, blocks, px, fb, bp.L, bp.l_stride, c->d_out);
            if (aov_rec)
                pt_launch_accumulate_aov(ms, blocks, px, fb, aov_rec, c->sc.tris, c->sc.n_tris, plane_as<float4>(c, kAovAlbedo),
                                         plane_as<float4>(c, kAovNormal), plane_as<uint2>(c, kAovId));
            // the moments fold goes last: it moves mom.z on, where the other two read the listed pixels' counts. An adaptive dispatch
            // always has the plane (it is refused without); a plain one folds it only while it is on.
            if (ap || mom) pt_launch_accumulate_moments(ms, blocks, px, fb, bp.L, bp.l_stride, mom);
            return PTMI_OK;
        };
        if (ap) {
            for (uint32_t r = 0; r < rounds; r++) {
                pt_launch_adaptive_list(ms, blocks, band, *ap, mom, c->ad);
                for (uint32_t f0 = 0; f0 < n_frames; f0 += F)
                    if ((rc = batch(0u, std::min(F, n_frames - f0)))) return rc;
            }
            c->ad_rounds += rounds;
        } else {
            for (uint32_t f0 = 0; f0 < n_frames; f0 += F)
                if ((rc = batch(cam->frame_index + f0, std::min(F, n_frames - f0)))) return rc;
        }
    }
    HIP_TRY(c, hipGetLastError());
    {   // the end of this dispatch on the context's stream (the fold of its last batch): what ptmi_throttle waits for
        hipEvent_t done = get_event(c);
        HIP_TRY(c, hipEventRecord(done, c->stream));
        c->in_flight.push_back(done);
        if (c->in_flight.size() > kMaxDispatchesInFlight) HIP_TRY(c, throttle(c, kMaxDispatchesInFlight));
    }
    if (!ap) { c->st.paths += npix * n_frames; c->st.frames += n_frames; }      // adaptive: counted on the device (DevAdaptive::acc)
    c->st.dispatches += 1;
    return PTMI_OK;
}

}  // namespace

extern "C" {

int ptmi_dispatch(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n_frames) { return dispatch(c, cam, n_frames, nullptr, 0); }

int ptmi_dispatch_adaptive(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *params, uint32_t rounds) {
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
    return dispatch(c, cam, ap.step, &ap, rounds);
}

int ptmi_adaptive_status(ptmi_ctx *c, struct ptmi_adaptive_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    if (!c->moments_on) return fail(c, PTMI_E_STATE, "the moments plane is off (ptmi_set_moments)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = adaptive_words(c);
    if (rc) return rc;
    std::memset(out, 0, sizeof *out);
    const DevBand band = pt_band_of(c->opt, c->W, c->H);
    const unsigned long long preset[3] = {0ull, ~0ull, 0ull};
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    uint32_t ctl[2] = {0u, 0u};
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    if (band.y0 < band.y1 && band.rows) {
        HIP_TRY(c, hipMemcpyAsync(&c->ad.acc[1], preset, sizeof preset, hipMemcpyHostToDevice, c->stream));
        pt_launch_adaptive_status(c->stream, c->n_cu * 8, band, plane_as<float4>(c, kMoments), c->ad);
        HIP_TRY(c, hipMemcpyAsync(acc, &c->ad.acc[1], sizeof acc, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(ctl, c->ad.ctl, sizeof ctl, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->active = ctl[1];
    out->samples = acc[0];
    out->min_count = acc[1] == ~0ull ? 0u : (uint32_t)acc[1];
    out->max_count = (uint32_t)acc[2];
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
    const TraverseConfig cfg0 = traverse_config(c, true);
    if (c->opt.traversal == PTMI_TRAVERSAL_LDS && pt_variant(cfg0.variant).where != PT_LDS_ALL)
        return fail(c, PTMI_E_UNSUPPORTED, "scene does not fit in LDS");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = (size_t)c->W * c->H;
    const uint32_t history = bit(kRpOut) | bit(kRpMoments) | bit(kRpNormal) | (have_albedo ? bit(kRpAlbedo) : 0u) | (have_ids ? bit(kRpId) : 0u);
    if ((rc = make_planes(c, history, npix, c->plane))) return rc;
    if (!c->d_reproject) HIP_TRY(c, hipMalloc(&c->d_reproject, 4 * sizeof(unsigned long long)));
    Lane &ln = c->lane;
    if (band.rows && (rc = ensure_capacity(c, ln, (size_t)band.rows * band.width))) return rc;
    if (cfg0.wants_spill && !ln.d_spill) HIP_TRY(c, hipMalloc(&ln.d_spill, pt_spill_bytes(c->n_cu * 8)));
    const hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->d_reproject, 0, 4 * sizeof(unsigned long long), s));
    if (band.rows == 0) return PTMI_OK;                         // more parts than strips: no pixel of this context's
    const struct { FramePlane to; const void *from; bool on; } copies[] = {
        {kRpOut, c->d_out, true}, {kRpMoments, c->plane[kMoments], true}, {kRpNormal, c->plane[kAovNormal], true},
        {kRpAlbedo, c->plane[kAovAlbedo], have_albedo}, {kRpId, c->plane[kAovId], have_ids}};
    for (const auto &cp : copies)
        if (cp.on) HIP_TRY(c, hipMemcpyAsync(c->plane[cp.to], cp.from, kFrame[cp.to].bytes(npix), hipMemcpyDeviceToDevice, s));
    TraverseConfig cfg = cfg0;
    cfg.spill = ln.d_spill;
    const int blocks = c->n_cu * 8;
    pt_launch_center_rays(s, blocks, *to, band, ln.paths, &ln.counts[0]);
    (c->sc.own ? pt_launch_extend_own : pt_launch_extend)(s, blocks, cfg, c->sc, ln.paths, nullptr, &ln.counts[0], ln.hits);
    ReprojectArgs a{};
    a.from = *from; a.band = band;
    a.max_history = q.max_history ? q.max_history : 32u;
    a.depth_tolerance = q.depth_tolerance > 0.0f ? q.depth_tolerance : 0.02f;
    a.match_ids = q.match_ids == 2u || (q.match_ids == 0u && have_ids) ? 1u : 0u;
    a.O = ln.paths.O; a.D = ln.paths.D; a.hits = ln.hits;
    a.tris = c->sc.tris; a.n_tris = c->sc.n_tris;
    a.h_out = plane_as<float4>(c, kRpOut); a.h_mom = plane_as<float4>(c, kRpMoments); a.h_normal = plane_as<float4>(c, kRpNormal);
    a.h_albedo = have_albedo ? plane_as<float4>(c, kRpAlbedo) : nullptr; a.h_ids = have_ids ? plane_as<uint2>(c, kRpId) : nullptr;
    a.out = c->d_out; a.mom = plane_as<float4>(c, kMoments); a.normal = plane_as<float4>(c, kAovNormal);
    a.albedo = have_albedo ? plane_as<float4>(c, kAovAlbedo) : nullptr; a.ids = have_ids ? plane_as<uint2>(c, kAovId) : nullptr;
    a.status = c->d_reproject;
    pt_launch_reproject(s, a);
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int ptmi_reproject_status(ptmi_ctx *c, struct ptmi_reproject_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    std::memset(out, 0, sizeof *out);
    if (!c->d_reproject) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    unsigned long long h[4];
    HIP_TRY(c, hipMemcpy(h, c->d_reproject, sizeof h, hipMemcpyDeviceToHost));
    out->carried = h[0]; out->disoccluded = h[1]; out->missed = h[2]; out->samples = h[3];
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
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    HIP_TRY(c, throttle(c, 0));
    return PTMI_OK;
}

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
    HIP_TRY(c, sync_all(c));
    drain_events(c);
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
    if (!mask) { dfree(c->lane.buf[kAovRec]); lane_views(c->lane); }      // the records live only while a plane is on (ensure_capacity makes them)
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

void *ptmi_moments_device_ptr(ptmi_ctx *c) { return c && c->moments_on ? c->plane[kMoments] : nullptr; }

int ptmi_denoise(ptmi_ctx *c, const ptmi_denoise_params *p, float *dst_rgba, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    const ptmi_denoise_params zero = {};
    const ptmi_denoise_params &q = p ? *p : zero;
    if (q.iterations > 10u) return fail(c, PTMI_E_INVALID, "iterations = %u is above 10", q.iterations);
    if (q.demodulate > 2u) return fail(c, PTMI_E_INVALID, "unknown demodulate %u", q.demodulate);
    if (q.reserved[0] || q.reserved[1] || q.reserved[2]) return fail(c, PTMI_E_INVALID, "a reserved word is not zero");
    const float phis[3] = {q.phi_color, q.phi_normal, q.phi_depth};
    for (float f : phis)
        if (!std::isfinite(f) || f < 0.0f) return fail(c, PTMI_E_INVALID, "phi %g is negative or not finite", (double)f);
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    const size_t npix = (size_t)c->W * c->H;
    if (dst_rgba && n_floats != npix * 4) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", npix * 4, n_floats);
    if (!(c->aov_mask & PTMI_AOV_NORMAL) || !c->plane[kAovNormal])
        return fail(c, PTMI_E_STATE, "the denoiser needs the NORMAL plane (ptmi_set_aovs)");
    if (!c->plane[kMoments]) return fail(c, PTMI_E_STATE, "the denoiser needs the moments plane (ptmi_set_moments)");
    const bool have_albedo = (c->aov_mask & PTMI_AOV_ALBEDO) && c->plane[kAovAlbedo];
    if (q.demodulate == 2u && !have_albedo) return fail(c, PTMI_E_STATE, "demodulate = 2 needs the ALBEDO plane (ptmi_set_aovs)");
    const bool demod = q.demodulate == 2u || (q.demodulate == 0u && have_albedo);
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = make_planes(c, group_set(kByDenoise), npix, c->plane);
    if (rc) return rc;
    DenoiseArgs da;
    da.W = c->W; da.H = c->H;
    da.iterations = q.iterations ? q.iterations : 5u;
    da.phi_color = q.phi_color > 0.0f ? q.phi_color : 4.0f;
    da.phi_normal = q.phi_normal > 0.0f ? q.phi_normal : 128.0f;
    da.phi_depth = q.phi_depth > 0.0f ? q.phi_depth : 1.0f;
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
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    unsigned long long h[kStatsWords];
    HIP_TRY(c, hipMemcpy(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost));
    c->st.segments = h[0]; c->st.shadow_rays = h[1] - h[3]; c->st.shadow_traced = h[2] - h[3];      // h[3]: records of emissive hits
    for (int i = 0; i < 64; i++) c->st.segments_by_bounce[i] = h[8 + i];
    c->st.verify_failed = h[4];
    c->st.bvh_depth = stats_depth(c);
    *out = c->st;
    if (c->ad.acc) {                                  // the samples adaptive dispatches traced
        unsigned long long traced = 0;
        HIP_TRY(c, hipMemcpy(&traced, c->ad.acc, sizeof traced, hipMemcpyDeviceToHost));
        out->paths += traced;
    }
    return PTMI_OK;
}

int ptmi_reset_stats(ptmi_ctx *c) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    drain_events(c);
    HIP_TRY(c, hipMemset(c->d_stats, 0, kStatsWords * sizeof(unsigned long long)));
    if (c->ad.acc) HIP_TRY(c, hipMemset(c->ad.acc, 0, sizeof(unsigned long long)));
    const ptmi_stats old = c->st;
    std::memset(&c->st, 0, sizeof c->st);
    c->st.bvh_depth = stats_depth(c);
    c->st.upload_ms = old.upload_ms; c->st.upload_tree_ms = old.upload_tree_ms; c->st.upload_copy_ms = old.upload_copy_ms;
    c->st.leaves_used = old.leaves_used; c->st.leaf_tris_used = old.leaf_tris_used; c->st.tree_builder_used = old.tree_builder_used;
    return PTMI_OK;
}

// ---- per-stage entry points ------------------------------------------------------
int ptmi_debug_raygen(ptmi_ctx *c, const ptmi_camera *cam, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                      const uint32_t *frames, float *o3, float *d3, uint32_t *rng) {
    if (!c || !cam || !xs || !ys || !frames || !o3 || !d3) return PTMI_E_INVALID;
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &ln = c->lane;                              // the per-stage entry points run on the context's stream
    HIP_TRY(c, sync_all(c));
    int rc = ensure_capacity(c, ln, n);
    if (rc) return rc;
    uint32_t *dx = ln.queue[0], *dy = ln.queue[1], *df = reinterpret_cast<uint32_t *>(ln.hits);
    HIP_TRY(c, hipMemcpyAsync(dx, xs, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dy, ys, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(df, frames, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    pt_launch_raygen_list(c->stream, *cam, n, dx, dy, df, ln.paths);
    std::vector<float4> o(n), d(n);
    HIP_TRY(c, hipMemcpyAsync(o.data(), ln.paths.O, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.data(), ln.paths.D, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    for (uint32_t i = 0; i < n; i++) {
        o3[3 * i] = o[i].x; o3[3 * i + 1] = o[i].y; o3[3 * i + 2] = o[i].z;
        d3[3 * i] = d[i].x; d3[3 * i + 1] = d[i].y; d3[3 * i + 2] = d[i].z;
        if (rng) std::memcpy(&rng[i], &o[i].w, 4);
    }
    return PTMI_OK;
}

int ptmi_debug_center_rays(ptmi_ctx *c, const ptmi_camera *cam, float *o3, float *d3, size_t n_floats_each) {
    if (!c) return PTMI_E_INVALID;
    if (!cam || !o3 || !d3) return fail(c, PTMI_E_INVALID, "NULL argument");
    if (c->W == 0 || c->H == 0) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (cam->width != c->W || cam->height != c->H)
        return fail(c, PTMI_E_INVALID, "camera says %ux%u but the output buffer is %ux%u", cam->width, cam->height, c->W, c->H);
    const size_t n = (size_t)c->W * c->H;
    if (n_floats_each != n * 3) return fail(c, PTMI_E_INVALID, "expected %zu floats each, got %zu", n * 3, n_floats_each);
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &ln = c->lane;                              // the per-stage entry points run on the context's stream
    HIP_TRY(c, sync_all(c));
    int rc = ensure_capacity(c, ln, n);
    if (rc) return rc;
    const DevBand whole{c->W, c->H, 0u, c->H, 1u, 1u, 0u, c->H};
    pt_launch_center_rays(c->stream, c->n_cu * 8, *cam, whole, ln.paths, &ln.counts[0]);
    std::vector<float4> o(n), d(n);
    HIP_TRY(c, hipMemcpyAsync(o.data(), ln.paths.O, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.data(), ln.paths.D, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    for (size_t i = 0; i < n; i++) {
        o3[3 * i] = o[i].x; o3[3 * i + 1] = o[i].y; o3[3 * i + 2] = o[i].z;
        d3[3 * i] = d[i].x; d3[3 * i + 1] = d[i].y; d3[3 * i + 2] = d[i].z;
    }
    return PTMI_OK;
}

int ptmi_debug_intersect(ptmi_ctx *c, uint32_t n, const float *o3, const float *d3, float *t, uint32_t *tri,
                         float *u, float *v) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!o3 || !d3 || !t || !tri || !u || !v) return fail(c, PTMI_E_INVALID, "NULL argument");
    if (n == 0) return PTMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &ln = c->lane;                              // the per-stage entry points run on the context's stream
    HIP_TRY(c, sync_all(c));
    rc = ensure_capacity(c, ln, n);
    if (rc) return rc;
    rc = upload_rays(c, n, o3, d3, nullptr, ln.paths.O, ln.paths.D);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(&ln.counts[0], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg = traverse_config(c, true);
    if (c->opt.traversal == PTMI_TRAVERSAL_LDS && pt_variant(cfg.variant).where != PT_LDS_ALL)
        return fail(c, PTMI_E_UNSUPPORTED, "scene does not fit in LDS");
    if (cfg.wants_spill && !ln.d_spill) HIP_TRY(c, hipMalloc(&ln.d_spill, pt_spill_bytes(c->n_cu * 8)));
    cfg.spill = ln.d_spill;
    c->st.extend_variant = pt_variant_code(cfg);
    (c->sc.own ? pt_launch_extend_own : pt_launch_extend)(c->stream, c->n_cu * 8, cfg, c->sc, ln.paths, nullptr, &ln.counts[0], ln.hits);
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
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &ln = c->lane;                              // the per-stage entry points run on the context's stream
    HIP_TRY(c, sync_all(c));
    rc = ensure_capacity(c, ln, n);
    if (rc) return rc;
    {   // every negative distance means "directional light" (ptmi.h). Inside the library -2 is the record of an emissive hit
        // (nothing to trace, traverse.hip ShadowIO::fetch): a caller's -2 must not be read as that, so negatives travel as -1
        std::vector<float> dn(dist, dist + n);
        for (float &x : dn) if (x < 0.0f) x = -1.0f;
        rc = upload_rays(c, n, o3, d3, dn.data(), ln.sh[0].SO, ln.sh[0].SD);
    }
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(&ln.counts[0], &n, 4, hipMemcpyHostToDevice, c->stream));
    TraverseConfig cfg = traverse_config(c, false);
    if (cfg.wants_spill && !ln.d_spill) HIP_TRY(c, hipMalloc(&ln.d_spill, pt_spill_bytes(c->n_cu * 8)));
    cfg.spill = ln.d_spill;
    c->st.shadow_variant = pt_variant_code(cfg);
    (c->sc.own ? pt_launch_shadow_own : pt_launch_shadow)(c->stream, c->n_cu * 8, cfg, c->sc, ln.paths, ln.sh[0], nullptr, &ln.counts[0], ln.d_occ);
    HIP_TRY(c, hipMemcpyAsync(occ, ln.d_occ, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_all(c));
    HIP_TRY(c, hipGetLastError());
    return PTMI_OK;
}

int ptmi_debug_image_stats(const ptmi_triangle *tris, uint32_t nt, const ptmi_bvh_node *nodes, uint32_t nn, double out[8]) {
    if (!out || (nt && !tris) || (nn && !nodes)) return PTMI_E_INVALID;
    for (int i = 0; i < 8; i++) out[i] = 0.0;
    ptmi_options opt;
    default_options(opt);
    opt.leaves = 1;                                 // the image over the reference's leaves (ptmi_debug_build_image: the own one)
    Built b;
    int rc = build_image(opt, nullptr, -1, tris, nt, nodes, nn, b, g_create_err);     // host-only: never touches a device
    if (rc) return rc;
    const std::vector<float4> &fast_wnodes = b.vec<float4>(kWnodes), &tripos = b.vec<float4>(kRefTripos);
    const std::vector<uint4> &qnodes = b.vec<uint4>(kQnodes);
    const std::vector<uint32_t> &leaf_stream = b.vec<uint32_t>(kLeafStream);
    const float *q_origin = b.img.q_origin, *q_scale = b.img.q_scale;
    out[0] = (double)(fast_wnodes.size() / 4); out[2] = fast_wnodes.empty() ? 0.0 : (double)b.img.depth;
    out[3] = (double)(qnodes.size() / 2); out[4] = (double)leaf_stream.size();
    if (qnodes.empty()) return PTMI_OK;
    // every quantised child box, decoded with the kernel's own fmaf, must contain the exact child box it stands for
    double viol = 0.0, infl = 0.0; size_t boxes = 0, leaves = 0, bad_hdr = 0;
    auto area = [](const float *lo, const float *hi) {
        double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return 2.0 * (x * y + y * z + z * x);
    };
    // the quantised nodes are renumbered (top levels first): walk both images together from their roots
    std::vector<std::pair<uint32_t, uint32_t>> todo;       // (node of the exact image, node of the quantised image)
    todo.push_back({0u, 0u});
    size_t visited = 0;
    while (!todo.empty()) {
        const uint32_t i = todo.back().first, qi = todo.back().second;
        todo.pop_back();
        if ((size_t)qi * 2 + 1 >= qnodes.size() || (size_t)i * 4 + 3 >= fast_wnodes.size()) { bad_hdr++; continue; }
        visited++;
        const float4 *w = &fast_wnodes[(size_t)i * 4];
        const float lo[2][3] = {{w[0].x, w[0].y, w[0].z}, {w[1].z, w[1].w, w[2].x}};
        const float hi[2][3] = {{w[0].w, w[1].x, w[1].y}, {w[2].y, w[2].z, w[2].w}};
        uint32_t refs[2]; std::memcpy(&refs[0], &w[3].x, 4); std::memcpy(&refs[1], &w[3].y, 4);
        for (int ch = 0; ch < 2; ch++) {
            const uint4 q = qnodes[(size_t)qi * 2 + ch];
            const uint32_t pl[6] = {q.x & 0xFFFFu, q.x >> 16, q.y & 0xFFFFu, q.y >> 16, q.z & 0xFFFFu, q.z >> 16};   // lo.xyz, hi.xyz
            float dlo[3], dhi[3];
            for (int k = 0; k < 3; k++) {
                dlo[k] = std::fmaf(q_scale[k], (float)pl[k], q_origin[k]);
                dhi[k] = std::fmaf(q_scale[k], (float)pl[3 + k], q_origin[k]);
                if (!(dlo[k] <= lo[ch][k]) || !(dhi[k] >= hi[ch][k])) viol += 1.0;
            }
            const double a0 = area(lo[ch], hi[ch]);
            if (a0 > 0.0) { infl += area(dlo, dhi) / a0 - 1.0; boxes++; }
            if (refs[ch] & PT_REF_LEAF) {
                leaves++;
                if (!(q.w & PT_REF_LEAF)) { bad_hdr++; continue; }
                const uint32_t *h = &leaf_stream[q.w & ~PT_REF_LEAF];
                float hl[3], hh[3]; std::memcpy(hl, h, 12); std::memcpy(hh, h + 4, 12);
                const uint32_t first = refs[ch] & PT_LEAF_OFF_MASK, cnt = ((refs[ch] >> PT_LEAF_OFF_BITS) & (PT_LEAF_MAX_TRIS - 1u)) + 1u;
                bool ok = h[3] == first && h[7] == cnt;
                for (int k = 0; k < 3; k++) ok = ok && hl[k] == lo[ch][k] && hh[k] == hi[ch][k];
                for (uint32_t t = 0; t < cnt && ok; t++)
                    for (int j = 0; j < 3; j++) {
                        const float4 &v = tripos[3 * (size_t)(first + t) + j];
                        float g[3]; std::memcpy(g, h + 8 + 9 * t + 3 * j, 12);
                        ok = ok && std::memcmp(&g[0], &v.x, 4) == 0 && std::memcmp(&g[1], &v.y, 4) == 0 && std::memcmp(&g[2], &v.z, 4) == 0;
                    }
                if (!ok) bad_hdr++;
            } else if (q.w & PT_REF_LEAF) bad_hdr++;
            else {
                // an inner box is the exact union of its two children's boxes (what makes any topology equivalent, §3.2)
                if ((size_t)refs[ch] * 4 + 3 < fast_wnodes.size()) {
                    const float4 *cw = &fast_wnodes[(size_t)refs[ch] * 4];
                    const float clo[3] = {std::min(cw[0].x, cw[1].z), std::min(cw[0].y, cw[1].w), std::min(cw[0].z, cw[2].x)};
                    const float chi[3] = {std::max(cw[0].w, cw[2].y), std::max(cw[1].x, cw[2].z), std::max(cw[1].y, cw[2].w)};
                    for (int k = 0; k < 3; k++) if (clo[k] != lo[ch][k] || chi[k] != hi[ch][k]) { bad_hdr++; break; }
                }
                todo.push_back({refs[ch], q.w});
            }
        }
    }
    if (visited != qnodes.size() / 2) bad_hdr++;          // every node reached exactly once (a tree: no node can be reached twice)
    out[1] = (double)leaves; out[5] = viol; out[6] = boxes ? infl / (double)boxes : 0.0; out[7] = (double)bad_hdr;
    return PTMI_OK;
}

int ptmi_debug_build_image(const ptmi_triangle *tris, uint32_t nt, const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_options *opt,
                           ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12, float *leafbox8) {
    if (!info || (nt && !tris) || (nn && !nodes)) return PTMI_E_INVALID;
    std::memset(info, 0, sizeof *info);
    ptmi_options o;
    default_options(o);
    if (opt) { o.leaves = opt->leaves; o.leaf_tris = opt->leaf_tris; o.keep_reference_tree = opt->keep_reference_tree; }
    Built b;
    int rc = build_image(o, nullptr, -1, tris, nt, nodes, nn, b, g_create_err);       // host-only: never touches a device
    if (rc) return rc;
    *info = b.img;
    const struct { const HeldBuf &from; void *to; } out[] = {
        {walked(b.buf, kWnodes), wnodes16}, {b.buf[kQnodes], qnodes8}, {walked(b.buf, kTripos), tripos12}, {b.buf[kLeafbox], leafbox8}};
    for (const auto &x : out) if (x.to && x.from.bytes) std::memcpy(x.to, x.from.host, x.from.bytes);
    return PTMI_OK;
}

int ptmi_debug_read_image(ptmi_ctx *c, ptmi_image_info *info, float *wnodes16, uint32_t *qnodes8, float *tripos12, float *leafbox8) {
    if (!c || !info) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_all(c));
    *info = c->img;
    if (!c->have_scene) return PTMI_OK;
    void *const *d = c->buf;
    const struct { const void *from; void *to; size_t bytes; } out[] = {
        {walked(d, kWnodes), wnodes16, (size_t)info->n_wnodes * 64},
        {d[kQnodes], qnodes8, info->quantised ? (size_t)info->n_wnodes * 32 : 0},
        {walked(d, kTripos), tripos12, (size_t)info->n_tris * 48},
        {d[kLeafbox], leafbox8, info->leaves_used == 2 ? (size_t)c->sc.n_tris * 32 : 0}};
    for (const auto &x : out) if (x.to && x.bytes) HIP_TRY(c, hipMemcpy(x.to, x.from, x.bytes, hipMemcpyDeviceToHost));
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
