// ptmi_multi.hip — several GPUs of one node behind the C ABI (include/ptmi.h, "several GPUs").
//
// The caller is the reference's frame loop (src/renderer/renderer.ts:415-454): one host thread driving one Renderer. Here the
// Renderer owns N device contexts; the frame's rows are dealt out as interleaved strips (DevBand, pt_device.h), every device
// traces and accumulates its own rows — pixels and RNG streams are independent (pt.wgsl:719, :753-761), so there is no
// collective on the data path — and ONE gather (gather_set) assembles on device 0 any set of the output buffer, the first-hit planes
// and the moments plane, in one pass:
//
//     k_pack_planes (each device: its rows of every named plane -> one share; DevPlaneSet, pt_device.h)   on that device's stream
//     ncclGather    (one group call, root = device 0; RCCL over xGMI; loopback: one peer copy per device)  on the same streams
//     k_unpack_planes (device 0: one pass over the frame, row y from the share of the device that owns it) on device 0's stream
//
// ptmi_multi_gather_planes names the set; ptmi_multi_gather is the set of the output buffer alone. Adaptive rounds with neighbourhood = 1
// exchange one byte per pixel per round (the NOISY flags) among all devices: ncclAllGather, or peer copies in loopback
// (ptmi_multi_dispatch_adaptive).
//
// Equal counts per rank are what ncclGather takes, so every device sends rows_max x width entries of each plane (the last round of strips may
// leave some devices a strip short; the padding is never unpacked). RCCL is loaded with dlopen when the first handle is
// created: a process that renders on one device never maps it.
#include "ptmi_ctx.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <functional>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

thread_local std::string g_multi_create_err;

// the RCCL entry points this file uses, resolved once (rccl.h supplies the types only)
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Gather)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) { err = std::string("cannot load librccl.so.1: ") + dlerror(); return false; }
        auto sym = [&](const char *n) { void *p = dlsym(lib, n); if (!p) err = std::string("librccl lacks ") + n; return p; };
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
        Gather = reinterpret_cast<decltype(Gather)>(sym("ncclGather"));
        AllGather = reinterpret_cast<decltype(AllGather)>(sym("ncclAllGather"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Gather || !AllGather || !GetErrorString) {
            dlclose(lib); lib = nullptr; return false;
        }
        return true;
    }
} g_rccl;

constexpr uint32_t kStripRows = 4;      // measured on Cornell: every N-th 4-row strip is an even sample of the picture

}  // namespace

// what the handle keeps for device r
struct MultiDev {
    ptmi_ctx *ctx = nullptr;
    float4 *d_send = nullptr;                          // its packed rows
    uint8_t *d_flags = nullptr;                        // the whole-frame NOISY flags of an adaptive round, N shares (ptmi_multi::flags_bytes)
    // the events live on device r, ev_copied on device 0 (create_events / destroy_events)
    hipEvent_t ev_done = nullptr;                      // its rendering is done (recorded on its stream when a gather starts)
    hipEvent_t ev_packed = nullptr;                    // loopback: its share is packed
    hipEvent_t ev_copied = nullptr;                    // loopback: its share has been copied out of d_send (recorded on device 0's stream)
    hipEvent_t ev_flags = nullptr;                     // loopback: its flag share is written
    hipEvent_t ev_flags_copied = nullptr;              // loopback: it has copied every flag share
    bool copied_recorded = false, flags_copied_recorded = false;
};

struct ptmi_multi {
    std::vector<MultiDev> d;
    std::vector<int> dev;                              // (dev and comm are arrays of their own: ncclCommInitAll takes them so)
    std::vector<ncclComm_t> comm;                      // empty: loopback copies
    bool loopback = false;
    ptmi_options opt{};                                // as given by the caller (tile_strip 0 = automatic)
    uint32_t W = 0, H = 0, strip = kStripRows;
    size_t rows_max = 0;                               // rows of the largest share
    size_t share_bytes = 0;                            // what every d_send holds (d_recv: N of them): rows_max x W entries of the output
                                                       // and of every plane that is on (plane_set_of), when allocated
    uint32_t aov_mask = 0;                             // ptmi_multi_set_aovs / _set_moments: what every device has on
    bool moments_on = false;
    size_t flags_bytes = 0;                            // what every d_flags holds: N shares of rows_max x W bytes (a device's own share is
                                                       // its context's kAdFlags plane)
    float4 *d_recv = nullptr;                          // device 0: N shares
    hipEvent_t g0 = nullptr, g1 = nullptr;             // around the last gather on device 0's stream
    bool gather_timed = false;
    uint64_t dispatched = 0, gathered = 0;             // dispatch calls so far / included in device 0's frame
    uint64_t gathered_plane[4] = {0, 0, 0, 0};         // ... / included in device 0's ALBEDO, NORMAL, ID and moments plane (kind_of)
    mutable std::string err;
};

namespace {

int mfail(const ptmi_multi *m, int code, const char *fmt, ...) {
    char buf[640];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (m) m->err = buf; else g_multi_create_err = buf;
    return code;
}
// a failed call on device i: carry its message
int cfail(const ptmi_multi *m, int i, int rc, const char *what) {
    return mfail(m, rc, "%s on device %d (ordinal %d): %s", what, i, m->dev[i], ptmi_last_error(m->d[i].ctx));
}
// fn(ctx, args...) on every device's context in turn; the first failure is reported through cfail and ends the loop
template <class Fn, class... Args>
int each_ctx(const ptmi_multi *m, const char *what, Fn fn, const Args &...args) {
    for (size_t i = 0; i < m->d.size(); i++) {
        int rc = fn(m->d[i].ctx, args...);
        if (rc) return cfail(m, (int)i, rc, what);
    }
    return PTMI_OK;
}
#define MHIP(m, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return mfail((m), PTMI_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define MNCCL(m, expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) \
    return mfail((m), PTMI_E_HIP, "%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); } while (0)

// strip height for n devices: kStripRows when the frame is a whole number of rounds of that, else the largest smaller height that
// is (2160 rows over 8 devices: 3); ragged frames work with any height, a whole number of rounds only keeps the shares equal
uint32_t auto_strip(uint32_t H, uint32_t n) {
    if (n <= 1) return kStripRows;
    for (uint32_t s = kStripRows; s > 0; s--) if (H % (s * n) == 0) return s;
    return kStripRows;
}

ptmi_options options_of(const ptmi_multi *m, int i) {
    ptmi_options o = m->opt;
    const uint32_t n = (uint32_t)m->d.size();
    o.tile_y0 = 0; o.tile_y1 = 0;
    o.tile_parts = n > 1 ? n : 0; o.tile_part = n > 1 ? (uint32_t)i : 0; o.tile_strip = m->strip;
    return o;
}

constexpr uint32_t kAovAll = PTMI_AOV_ALBEDO | PTMI_AOV_NORMAL | PTMI_AOV_ID;
constexpr uint32_t kGatherAll = kAovAll | PTMI_MULTI_PLANE_MOMENTS | PTMI_MULTI_PLANE_OUTPUT;
static_assert((kAovAll & (PTMI_MULTI_PLANE_MOMENTS | PTMI_MULTI_PLANE_OUTPUT)) == 0, "the gather bits extend the PTMI_AOV_* bits");
// the planes whose staleness gathered_plane[] tracks (the output's is `gathered`)
const struct { uint32_t bit; const char *name; } kPlaneKinds[4] = {
    {PTMI_AOV_ALBEDO, "ALBEDO"}, {PTMI_AOV_NORMAL, "NORMAL"}, {PTMI_AOV_ID, "ID"}, {PTMI_MULTI_PLANE_MOMENTS, "moments"}};

// what every device has: the output buffer, the AOV planes of the mask, the moments plane while on
uint32_t planes_on(const ptmi_multi *m) { return PTMI_MULTI_PLANE_OUTPUT | m->aov_mask | (m->moments_on ? PTMI_MULTI_PLANE_MOMENTS : 0u); }
// the share of device i for `planes` (all of them on): output, ALBEDO, NORMAL, moments, then the ids
DevPlaneSet plane_set_of(const ptmi_multi *m, int i, uint32_t planes) {
    ptmi_ctx *c = m->d[i].ctx;
    DevPlaneSet set{};
    if (planes & PTMI_MULTI_PLANE_OUTPUT) set.f4[set.n4++] = c->d_out;
    if (planes & PTMI_AOV_ALBEDO) set.f4[set.n4++] = plane_as<float4>(c, kAovAlbedo);
    if (planes & PTMI_AOV_NORMAL) set.f4[set.n4++] = plane_as<float4>(c, kAovNormal);
    if (planes & PTMI_MULTI_PLANE_MOMENTS) set.f4[set.n4++] = plane_as<float4>(c, kMoments);
    if (planes & PTMI_AOV_ID) set.ids = plane_as<uint2>(c, kAovId);
    set.share_px = (uint32_t)(m->rows_max * m->W);
    return set;
}
// bytes of a share of rows_max x W entries of `planes`, a multiple of 16 (DevPlaneSet::share_bytes, before there are pointers)
size_t share_bytes_of(size_t rows_max, uint32_t W, uint32_t planes) {
    const size_t per_px = 16u * (size_t)__builtin_popcount(planes & (kGatherAll & ~(uint32_t)PTMI_AOV_ID)) + ((planes & PTMI_AOV_ID) ? 8u : 0u);
    return (rows_max * W * per_px + 15u) & ~(size_t)15u;
}

void free_buffers(ptmi_multi *m) {
    for (size_t i = 0; i < m->d.size(); i++) {
        MultiDev &d = m->d[i];
        (void)hipSetDevice(m->dev[i]);
        if (d.d_send) { (void)hipFree(d.d_send); d.d_send = nullptr; }
        if (d.d_flags) { (void)hipFree(d.d_flags); d.d_flags = nullptr; }
        d.copied_recorded = d.flags_copied_recorded = false;      // nothing is being copied out of buffers that are gone
    }
    if (m->d_recv) { (void)hipSetDevice(m->dev[0]); (void)hipFree(m->d_recv); m->d_recv = nullptr; }
    m->rows_max = 0; m->share_bytes = 0; m->flags_bytes = 0;
}

// options of every context + the gathers' buffers for the current size, strip height and set of planes that are on
int configure(ptmi_multi *m) {
    const int n = (int)m->d.size();
    m->strip = m->opt.tile_strip ? m->opt.tile_strip : auto_strip(m->H ? m->H : 1, (uint32_t)n);
    for (int i = 0; i < n; i++) {
        const ptmi_options o = options_of(m, i);
        int rc = ptmi_set_options(m->d[i].ctx, &o);
        if (rc) return cfail(m, i, rc, "ptmi_set_options");
    }
    if (m->W == 0) return PTMI_OK;
    size_t rows_max = 0;
    for (int i = 0; i < n; i++) rows_max = std::max<size_t>(rows_max, pt_band_of(options_of(m, i), m->W, m->H).rows);
    // the buffers are sized in BYTES (rows_max x W entries of every plane that is on): a resize that keeps the height but widens the
    // frame needs new ones, and so does a plane turned on. One device without RCCL gathers nothing and has none.
    const bool wanted = n > 1 || !m->comm.empty();
    const size_t share = share_bytes_of(rows_max, m->W, planes_on(m));
    if (rows_max == m->rows_max && share == m->share_bytes && (m->d_recv || !wanted)) return PTMI_OK;
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    free_buffers(m);
    m->rows_max = rows_max;
    if (!wanted) { m->share_bytes = share; return PTMI_OK; }
    for (int i = 0; i < n; i++) {
        MHIP(m, hipSetDevice(m->dev[i]));
        MHIP(m, hipMalloc(&m->d[i].d_send, std::max<size_t>(share, 16)));
        MHIP(m, hipMemset(m->d[i].d_send, 0, std::max<size_t>(share, 16)));
    }
    MHIP(m, hipSetDevice(m->dev[0]));
    MHIP(m, hipMalloc(&m->d_recv, std::max<size_t>(share * n, 16)));
    m->share_bytes = share;
    return PTMI_OK;
}

// every count back to 0 (the frame is the same on every device again, or fresh). A plane that device 0 does not hold whole stays stale.
void reset_counts(ptmi_multi *m, bool fresh) {
    for (uint64_t &g : m->gathered_plane) g = fresh || g == m->dispatched ? 0 : ~0ull;
    m->dispatched = m->gathered = 0;
}

// device 0 now holds `planes` whole
void mark_gathered(ptmi_multi *m, uint32_t planes) {
    if (planes & PTMI_MULTI_PLANE_OUTPUT) m->gathered = m->dispatched;
    for (int k = 0; k < 4; k++) if (planes & kPlaneKinds[k].bit) m->gathered_plane[k] = m->dispatched;
}

// pack -> collective -> unpack of `planes` (all on, not 0, buffers in place) onto device 0: the one body of every gather
int gather_set(ptmi_multi *m, uint32_t planes) {
    const int n = (int)m->d.size();
    hipStream_t s0 = pt_ctx_stream(m->d[0].ctx);
    // the timed region (ptmi_multi_gather_ms) starts when EVERY device has rendered its rows: pack, gather, unpack — not the wait for
    // the slowest device, which is the dispatch's time
    for (int i = 1; i < n; i++) {
        MHIP(m, hipSetDevice(m->dev[i]));
        MHIP(m, hipEventRecord(m->d[i].ev_done, pt_ctx_stream(m->d[i].ctx)));
        MHIP(m, hipSetDevice(m->dev[0]));
        MHIP(m, hipStreamWaitEvent(s0, m->d[i].ev_done, 0));
    }
    MHIP(m, hipSetDevice(m->dev[0]));
    MHIP(m, hipEventRecord(m->g0, s0));
    const DevPlaneSet set0 = plane_set_of(m, 0, planes);
    const size_t share = set0.share_bytes();              // of this gather: at most m->share_bytes, what the buffers hold per device
    if (share > m->share_bytes) return mfail(m, PTMI_E_STATE, "a share of %zu bytes does not fit the %zu-byte buffers", share, m->share_bytes);
    for (int i = 0; i < n; i++) {
        const DevBand band = pt_band_of(options_of(m, i), m->W, m->H);
        MHIP(m, hipSetDevice(m->dev[i]));
        // loopback: the previous gather's copy out of d_send[i] (on device 0's stream) must be done before it is packed again
        if (m->comm.empty() && i > 0 && m->d[i].copied_recorded) MHIP(m, hipStreamWaitEvent(pt_ctx_stream(m->d[i].ctx), m->d[i].ev_copied, 0));
        // (loopback: device 0's share is never read)
        if (band.rows && (i > 0 || !m->comm.empty()))
            pt_launch_pack_planes(pt_ctx_stream(m->d[i].ctx), pt_ctx_cus(m->d[i].ctx) * 8, band, plane_set_of(m, i, planes), m->d[i].d_send);
    }
    if (!m->comm.empty()) {
        MNCCL(m, g_rccl.GroupStart());
        for (int i = 0; i < n; i++) {
            ncclResult_t r = g_rccl.Gather(m->d[i].d_send, i == 0 ? m->d_recv : nullptr, share / 4, ncclFloat, 0, m->comm[i], pt_ctx_stream(m->d[i].ctx));
            if (r != ncclSuccess) { (void)g_rccl.GroupEnd(); return mfail(m, PTMI_E_HIP, "ncclGather (device %d) failed: %s", i, g_rccl.GetErrorString(r)); }
        }
        MNCCL(m, g_rccl.GroupEnd());
    } else {
        // loopback: device r's share is copied into slot r of device 0's receive buffer once it is packed
        for (int i = 1; i < n; i++) {
            MHIP(m, hipSetDevice(m->dev[i]));
            MHIP(m, hipEventRecord(m->d[i].ev_packed, pt_ctx_stream(m->d[i].ctx)));
            MHIP(m, hipSetDevice(m->dev[0]));
            MHIP(m, hipStreamWaitEvent(s0, m->d[i].ev_packed, 0));
            MHIP(m, hipMemcpyPeerAsync(reinterpret_cast<char *>(m->d_recv) + (size_t)i * share, m->dev[0], m->d[i].d_send, m->dev[i], share, s0));
            MHIP(m, hipEventRecord(m->d[i].ev_copied, s0));
            m->d[i].copied_recorded = true;
        }
    }
    MHIP(m, hipSetDevice(m->dev[0]));
    // device 0's own rows are already in place (RCCL delivers a copy of them into slot 0; one device through RCCL — the degenerate
    // gather of its whole frame onto itself — unpacks that copy, so that the planes really went through the collective)
    pt_launch_unpack_planes(s0, pt_ctx_cus(m->d[0].ctx) * 8, pt_band_of(options_of(m, 0), m->W, m->H), set0, m->d_recv, n > 1 ? 0u : 0xFFFFFFFFu);
    MHIP(m, hipEventRecord(m->g1, s0));
    MHIP(m, hipGetLastError());
    m->gather_timed = true;
    mark_gathered(m, planes);
    return PTMI_OK;
}

// of `planes` (all on), those device 0 does not hold whole
uint32_t stale_of(const ptmi_multi *m, uint32_t planes) {
    uint32_t stale = (planes & PTMI_MULTI_PLANE_OUTPUT) && m->gathered != m->dispatched ? PTMI_MULTI_PLANE_OUTPUT : 0u;
    for (int k = 0; k < 4; k++) if ((planes & kPlaneKinds[k].bit) && m->gathered_plane[k] != m->dispatched) stale |= kPlaneKinds[k].bit;
    return stale;
}

// fn(i) for every device, each from a thread of its own for the length of the call (ptmi_multi_dispatch says why); the first failure
int each_threaded(ptmi_multi *m, const char *what, const std::function<int(size_t)> &fn) {
    const size_t n = m->d.size();
    std::vector<int> rcs(n, PTMI_OK);
    std::vector<std::thread> pool;
    pool.reserve(n - 1);
    for (size_t i = 1; i < n; i++) pool.emplace_back([&, i] { rcs[i] = fn(i); });
    rcs[0] = fn(0);
    for (std::thread &t : pool) t.join();
    for (size_t i = 0; i < n; i++) if (rcs[i]) return cfail(m, (int)i, rcs[i], what);
    return PTMI_OK;
}

// the events of device i, each on the device whose stream records it: ev_copied on device 0, the others on device i
bool create_events(ptmi_multi *m, int i) {
    MultiDev &d = m->d[i];
    if (hipSetDevice(m->dev[i]) != hipSuccess) return false;
    for (hipEvent_t *e : {&d.ev_done, &d.ev_packed, &d.ev_flags, &d.ev_flags_copied})
        if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return false;
    return hipSetDevice(m->dev[0]) == hipSuccess && hipEventCreateWithFlags(&d.ev_copied, hipEventDisableTiming) == hipSuccess;
}
void destroy_events(ptmi_multi *m, int i) {
    const MultiDev &d = m->d[i];
    (void)hipSetDevice(m->dev[i]);
    for (hipEvent_t e : {d.ev_done, d.ev_packed, d.ev_flags, d.ev_flags_copied}) if (e) (void)hipEventDestroy(e);
    (void)hipSetDevice(m->dev[0]);
    if (d.ev_copied) (void)hipEventDestroy(d.ev_copied);
}

// fn(ctx, value) on every device in turn; on the first failure, reported through cfail, the devices already changed get `before` back
int each_ctx_or_back(ptmi_multi *m, const char *what, int (*fn)(ptmi_ctx *, uint32_t), uint32_t value, uint32_t before) {
    for (size_t i = 0; i < m->d.size(); i++) {
        const int rc = fn(m->d[i].ctx, value);
        if (rc) {
            cfail(m, (int)i, rc, what);
            for (size_t j = 0; j < i; j++) (void)fn(m->d[j].ctx, before);
            return rc;
        }
    }
    return PTMI_OK;
}

}  // namespace

extern "C" {

const char *ptmi_multi_last_error(const ptmi_multi *m) { return m ? m->err.c_str() : g_multi_create_err.c_str(); }

int ptmi_multi_create(int n, const int *ordinals, uint32_t flags, ptmi_multi **out) {
    if (!out) return mfail(nullptr, PTMI_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || n > 64) return mfail(nullptr, PTMI_E_INVALID, "n_devices %d not in 1..64", n);
    if (flags & ~(uint32_t)PTMI_MULTI_LOOPBACK) return mfail(nullptr, PTMI_E_INVALID, "unknown flags 0x%x", flags);
    ptmi_multi *m = new ptmi_multi();
    m->loopback = (flags & PTMI_MULTI_LOOPBACK) != 0;
    for (int i = 0; i < n; i++) m->dev.push_back(ordinals ? ordinals[i] : i);
    if (!m->loopback)
        for (int i = 0; i < n; i++)
            for (int j = 0; j < i; j++)
                if (m->dev[i] == m->dev[j]) {
                    const int d = m->dev[i]; delete m;
                    return mfail(nullptr, PTMI_E_INVALID, "device ordinal %d is listed twice (only PTMI_MULTI_LOOPBACK lets one device stand in for several)", d);
                }
    for (int i = 0; i < n; i++) {
        ptmi_ctx *c = nullptr;
        int rc = ptmi_create(m->dev[i], &c);
        if (rc) {
            mfail(nullptr, rc, "ptmi_create(%d): %s", m->dev[i], ptmi_last_error(nullptr));
            ptmi_multi_destroy(m);
            return rc;
        }
        m->d.push_back(MultiDev{c});
    }
    ptmi_get_options(m->d[0].ctx, &m->opt);
    m->opt.tile_strip = 0;
    if (!m->loopback && n >= 1) {
        // one communicator per device, one process (ncclCommInitAll). A single device goes through RCCL too: its gather is the
        // degenerate collective, and the un-sharded bits must come out of it unchanged.
        if (!g_rccl.load()) { mfail(nullptr, PTMI_E_UNSUPPORTED, "%s", g_rccl.err.c_str()); ptmi_multi_destroy(m); return PTMI_E_UNSUPPORTED; }
        m->comm.assign(n, nullptr);
        ncclResult_t r = g_rccl.CommInitAll(m->comm.data(), n, m->dev.data());
        if (r != ncclSuccess) {
            m->comm.clear();
            mfail(nullptr, PTMI_E_HIP, "ncclCommInitAll over %d devices failed: %s", n, g_rccl.GetErrorString(r));
            ptmi_multi_destroy(m);
            return PTMI_E_HIP;
        }
    }
    bool ok = true;
    for (int i = 0; i < n && ok; i++) ok = create_events(m, i);
    ok = ok && hipSetDevice(m->dev[0]) == hipSuccess && hipEventCreate(&m->g0) == hipSuccess && hipEventCreate(&m->g1) == hipSuccess;
    if (!ok) { mfail(nullptr, PTMI_E_HIP, "event creation failed"); ptmi_multi_destroy(m); return PTMI_E_HIP; }
    int rc = configure(m);
    if (rc) { g_multi_create_err = m->err; ptmi_multi_destroy(m); return rc; }
    *out = m;
    return PTMI_OK;
}

int ptmi_multi_destroy(ptmi_multi *m) {
    if (!m) return PTMI_E_INVALID;
    for (const MultiDev &d : m->d) (void)ptmi_synchronize(d.ctx);
    for (ncclComm_t c : m->comm) if (c) (void)g_rccl.CommDestroy(c);
    free_buffers(m);
    for (size_t i = 0; i < m->d.size(); i++) destroy_events(m, (int)i);       // (device 0 is current after the last)
    if (m->g0) (void)hipEventDestroy(m->g0);
    if (m->g1) (void)hipEventDestroy(m->g1);
    for (const MultiDev &d : m->d) (void)ptmi_destroy(d.ctx);
    delete m;
    return PTMI_OK;
}

int ptmi_multi_count(const ptmi_multi *m) { return m ? (int)m->d.size() : 0; }
ptmi_ctx *ptmi_multi_context(ptmi_multi *m, int i) { return (m && i >= 0 && i < (int)m->d.size()) ? m->d[i].ctx : nullptr; }

int ptmi_multi_upload_scene(ptmi_multi *m, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                            const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl) {
    if (!m) return PTMI_E_INVALID;
    // validation, the hierarchy and its images are built ONCE on the host (under device 0's options: all devices share them) and copied
    // to every device — the 1 M-triangle scene costs one build, not N (round 3: N x 196 ms)
    int rc = PTMI_OK;
    PtPrepared *p = pt_prepare_scene(m->d[0].ctx, tris, nt, mats, nm, nodes, nn, lights, nl, &rc);
    if (!p) return cfail(m, 0, rc, "ptmi_upload_scene (prepare)");
    for (size_t i = 0; i < m->d.size() && rc == PTMI_OK; i++) {
        rc = pt_install_scene(m->d[i].ctx, p);
        if (rc) rc = cfail(m, (int)i, rc, "ptmi_upload_scene (install)");
    }
    pt_free_prepared(p);
    return rc;
}

int ptmi_multi_upload_atlas(ptmi_multi *m, const void *texels, uint32_t w, uint32_t h, int fmt) {
    if (!m) return PTMI_E_INVALID;
    if (texels && w != 0 && h != 0) {       // checked once, before any device changes: a rejected atlas leaves every shard's in place
        size_t bytes = 0;
        char why[128];
        if (pt_atlas_bytes(w, h, fmt, &bytes, why, sizeof why) != PTMI_OK) return mfail(m, PTMI_E_INVALID, "%s", why);
    }
    return each_ctx(m, "ptmi_upload_atlas", ptmi_upload_atlas, texels, w, h, fmt);
}

int ptmi_multi_upload_environment(ptmi_multi *m, const void *texels, uint32_t w, uint32_t h, int fmt, const ptmi_environment *params) {
    if (!m) return PTMI_E_INVALID;
    if (texels && w != 0 && h != 0) {       // checked once, before any device changes: a rejected map leaves every shard's in place
        const int rc = ptmi_debug_env_table(texels, w, h, fmt, nullptr, nullptr, nullptr, nullptr);
        if (rc) return mfail(m, rc, "%s", ptmi_last_error(nullptr));
    }
    return each_ctx(m, "ptmi_upload_environment", ptmi_upload_environment, texels, w, h, fmt, params);
}

int ptmi_multi_set_environment(ptmi_multi *m, const ptmi_environment *params) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_set_environment", ptmi_set_environment, params);
}

int ptmi_multi_set_medium(ptmi_multi *m, const ptmi_medium *medium) {
    if (!m) return PTMI_E_INVALID;
    std::string why;                        // checked once, before any device changes: a rejected medium leaves every shard's in place
    int rc = pt_check_medium(medium, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    if (medium && pt_ctx_has_medium_grid(m->d[0].ctx) && (rc = pt_check_medium_depth(medium, why))) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_set_medium", ptmi_set_medium, medium);
}

int ptmi_multi_upload_medium_density(ptmi_multi *m, const float *rho, uint32_t nx, uint32_t ny, uint32_t nz, const ptmi_medium_grid *params) {
    if (!m) return PTMI_E_INVALID;
    if (rho && nx != 0 && ny != 0 && nz != 0) {     // checked once, before any device changes: a rejected grid leaves every shard's in place
        std::string why;
        const ptmi_medium *med = pt_ctx_medium(m->d[0].ctx);
        if (!med) return mfail(m, PTMI_E_STATE, "no medium in place (ptmi_set_medium)");
        int rc = pt_check_medium_density(rho, nx, ny, nz, params, nullptr, why);
        if (!rc) rc = pt_check_medium_depth(med, why);
        if (rc) return mfail(m, rc, "%s", why.c_str());
    }
    return each_ctx(m, "ptmi_upload_medium_density", ptmi_upload_medium_density, rho, nx, ny, nz, params);
}

// The alpha cutoff table on every device (alpha.hip). Every device holds the same scene, so device 0's answers the checks that need one.
int ptmi_multi_set_alpha_cutoff(ptmi_multi *m, const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params) {
    if (!m) return PTMI_E_INVALID;
    std::string why;                        // checked once, before any device changes: a rejected table leaves every shard's in place
    if (!pt_ctx_has_scene(m->d[0].ctx)) return mfail(m, PTMI_E_INVALID, "no scene uploaded: the table belongs to a scene's materials");
    const bool remove = !cutoff || n_materials == 0u;
    const int rc = pt_check_alpha_cutoff(remove ? nullptr : cutoff, n_materials, params, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    if (!remove && n_materials != pt_ctx_materials(m->d[0].ctx))
        return mfail(m, PTMI_E_INVALID, "n_materials %u is not the loaded scene's %u", n_materials, pt_ctx_materials(m->d[0].ctx));
    return each_ctx(m, "ptmi_set_alpha_cutoff", ptmi_set_alpha_cutoff, cutoff, n_materials, params);
}

int ptmi_multi_alpha_status(ptmi_multi *m, struct ptmi_alpha_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    for (int i = 0; i < (int)m->d.size(); i++) {
        struct ptmi_alpha_status st;
        const int rc = ptmi_alpha_status(m->d[i].ctx, &st);
        if (rc) return cfail(m, i, rc, "ptmi_alpha_status");
        if (i == 0) *out = st;
        else {
            out->path_passes += st.path_passes; out->path_exhausted += st.path_exhausted;
            out->shadow_passes += st.shadow_passes; out->shadow_exhausted += st.shadow_exhausted;
        }
    }
    return PTMI_OK;
}

// The alpha blend table on every device (alpha.hip), by the cutoff call's pattern.
int ptmi_multi_set_alpha_blend(ptmi_multi *m, const float *factor, uint32_t n_materials, const ptmi_alpha_blend_params *params) {
    if (!m) return PTMI_E_INVALID;
    std::string why;                        // checked once, before any device changes: a rejected table leaves every shard's in place
    if (!pt_ctx_has_scene(m->d[0].ctx)) return mfail(m, PTMI_E_INVALID, "no scene uploaded: the table belongs to a scene's materials");
    const bool remove = !factor || n_materials == 0u;
    const int rc = pt_check_alpha_blend(remove ? nullptr : factor, n_materials, params, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    if (!remove && n_materials != pt_ctx_materials(m->d[0].ctx))
        return mfail(m, PTMI_E_INVALID, "n_materials %u is not the loaded scene's %u", n_materials, pt_ctx_materials(m->d[0].ctx));
    return each_ctx(m, "ptmi_set_alpha_blend", ptmi_set_alpha_blend, factor, n_materials, params);
}

int ptmi_multi_alpha_blend_status(ptmi_multi *m, struct ptmi_alpha_blend_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    for (int i = 0; i < (int)m->d.size(); i++) {
        struct ptmi_alpha_blend_status st;
        const int rc = ptmi_alpha_blend_status(m->d[i].ctx, &st);
        if (rc) return cfail(m, i, rc, "ptmi_alpha_blend_status");
        if (i == 0) *out = st;
        else {
            out->path_tests += st.path_tests; out->path_passes += st.path_passes;
            out->shadow_tests += st.shadow_tests; out->shadow_passes += st.shadow_passes;
        }
    }
    return PTMI_OK;
}

// The edits of a loaded scene on every device (scene_update.hip). Every device holds the same scene under the same options and checks
// before it changes anything, so a refused call is refused by the first device and leaves them all as they were.
int ptmi_multi_update_triangles(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_triangle *tris) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_update_triangles", ptmi_update_triangles, first, count, tris);
}
int ptmi_multi_update_materials(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_material *mats) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_update_materials", ptmi_update_materials, first, count, mats);
}
int ptmi_multi_update_lights(ptmi_multi *m, uint32_t first, uint32_t count, const ptmi_light *lights) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_update_lights", ptmi_update_lights, first, count, lights);
}
int ptmi_multi_scene_update_status(ptmi_multi *m, struct ptmi_scene_update_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    const int rc = ptmi_scene_update_status(m->d[0].ctx, out);
    return rc ? cfail(m, 0, rc, "ptmi_scene_update_status") : PTMI_OK;
}

// The walked tree rebuilt on every device (scene_rebuild.hip). Every device holds the same scene and both builders are deterministic, so
// every device ends with the same image; the checks that refuse a call run once, on device 0's context, before any device changes.
int ptmi_multi_rebuild_tree(ptmi_multi *m, const ptmi_rebuild_params *params) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_rebuild(m->d[0].ctx, params, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_rebuild_tree", ptmi_rebuild_tree, params);
}
int ptmi_multi_rebuild_status(ptmi_multi *m, struct ptmi_rebuild_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    const int rc = ptmi_rebuild_status(m->d[0].ctx, out);
    return rc ? cfail(m, 0, rc, "ptmi_rebuild_status") : PTMI_OK;
}

// Triangle groups on every device (scene_transform.hip). The host-side checks run once, on device 0's context, before any device
// changes; every device holds the same triangles and the same table, so the check pass on the device refuses on the first device or
// on none.
int ptmi_multi_set_triangle_groups(ptmi_multi *m, const uint32_t *group, uint32_t n_triangles) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_triangle_groups(m->d[0].ctx, group, n_triangles, nullptr, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_set_triangle_groups", ptmi_set_triangle_groups, group, n_triangles);
}
int ptmi_multi_transform_groups(ptmi_multi *m, const ptmi_group_transform *ops, uint32_t n_ops) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_group_transforms(m->d[0].ctx, ops, n_ops, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_transform_groups", ptmi_transform_groups, ops, n_ops);
}
int ptmi_multi_transform_status(ptmi_multi *m, struct ptmi_transform_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    const int rc = ptmi_transform_status(m->d[0].ctx, out);
    return rc ? cfail(m, 0, rc, "ptmi_transform_status") : PTMI_OK;
}

// The skin on every device (scene_skin.hip), by the same rule as the groups: checked once on device 0's context.
int ptmi_multi_set_skin(ptmi_multi *m, const uint32_t *triangle, const ptmi_skin_corner *corners, uint32_t n_skinned, uint32_t n_joints) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_skin(m->d[0].ctx, triangle, corners, n_skinned, n_joints, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_set_skin", ptmi_set_skin, triangle, corners, n_skinned, n_joints);
}
int ptmi_multi_pose_skin(ptmi_multi *m, const ptmi_joint_transform *joints, uint32_t n_joints) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_skin_pose(m->d[0].ctx, joints, n_joints, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_pose_skin", ptmi_pose_skin, joints, n_joints);
}
int ptmi_multi_skin_status(ptmi_multi *m, struct ptmi_skin_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    const int rc = ptmi_skin_status(m->d[0].ctx, out);
    return rc ? cfail(m, 0, rc, "ptmi_skin_status") : PTMI_OK;
}

// The morph on every device (scene_morph.hip), by the same rule.
int ptmi_multi_set_morph(ptmi_multi *m, const uint32_t *triangle, const uint32_t *row_start, const ptmi_morph_delta *deltas,
                         uint32_t n_morphed, uint32_t n_targets) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_morph(m->d[0].ctx, triangle, row_start, deltas, n_morphed, n_targets, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_set_morph", ptmi_set_morph, triangle, row_start, deltas, n_morphed, n_targets);
}
int ptmi_multi_pose_morph(ptmi_multi *m, const float *weights, uint32_t n_targets) {
    if (!m) return PTMI_E_INVALID;
    std::string why;
    const int rc = pt_check_morph_pose(m->d[0].ctx, weights, n_targets, why);
    if (rc) return mfail(m, rc, "%s", why.c_str());
    return each_ctx(m, "ptmi_pose_morph", ptmi_pose_morph, weights, n_targets);
}
int ptmi_multi_morph_status(ptmi_multi *m, struct ptmi_morph_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    const int rc = ptmi_morph_status(m->d[0].ctx, out);
    return rc ? cfail(m, 0, rc, "ptmi_morph_status") : PTMI_OK;
}

int ptmi_multi_resize(ptmi_multi *m, uint32_t w, uint32_t h) {
    if (!m) return PTMI_E_INVALID;
    int rc = each_ctx(m, "ptmi_resize", ptmi_resize, w, h);
    if (rc) return rc;
    m->W = w; m->H = h;
    reset_counts(m, true);                  // every plane of every device is zero-filled
    return configure(m);
}

int ptmi_multi_set_options(ptmi_multi *m, const ptmi_options *o) {
    if (!m || !o) return PTMI_E_INVALID;
    if (o->tile_y0 != 0 || o->tile_y1 != 0) return mfail(m, PTMI_E_INVALID, "tile_y0 / tile_y1 must be 0: the rows are dealt out by the library");
    // The strip height decides which device owns which rows: changing it while frames are being accumulated would hand rows that
    // hold k frames to a device whose copy of them holds none. It takes effect with the next ptmi_multi_resize / _write_output.
    const uint32_t new_strip = o->tile_strip ? o->tile_strip : auto_strip(m->H ? m->H : 1, (uint32_t)m->d.size());
    if (m->dispatched != 0 && new_strip != m->strip)
        return mfail(m, PTMI_E_STATE, "tile_strip %u -> %u while %llu dispatches are accumulated: call ptmi_multi_resize or ptmi_multi_write_output first",
                     m->strip, new_strip, (unsigned long long)m->dispatched);
    const ptmi_options old = m->opt;
    m->opt = *o;
    int rc = configure(m);
    if (rc) { m->opt = old; (void)configure(m); }
    return rc;
}
int ptmi_multi_get_options(const ptmi_multi *m, ptmi_options *o) {
    if (!m || !o) return PTMI_E_INVALID;
    *o = m->opt; o->tile_strip = m->strip; o->tile_parts = (uint32_t)m->d.size(); o->tile_part = 0;
    return PTMI_OK;
}

int ptmi_multi_dispatch(ptmi_multi *m, const ptmi_camera *cam, uint32_t n_frames) {
    if (!m) return PTMI_E_INVALID;
    if (cam) {                              // a camera the projection switch rejects: once, before any device enqueues
        std::string why; uint32_t proj;
        const int bad = pt_check_camera(m->d[0].ctx, cam, &proj, why);
        if (bad) return mfail(m, bad, "%s", why.c_str());
    }
    // One ptmi_dispatch of 64 frames is ~45 launches and ~110 event calls: 1.15 ms of host time (profiles/r04_multi.json). Enqueued
    // in turn from one thread, device i would start i x that after device 0 — 8 ms at N = 8 against 16 ms of device time per step of
    // configs[4] — so every device gets its own enqueuing thread for the call (contexts are independent: own device, own streams;
    // a context is still only ever touched by one thread at a time).
    const int rc = each_threaded(m, "ptmi_dispatch", [&](size_t i) { return ptmi_dispatch(m->d[i].ctx, cam, n_frames); });
    if (rc) return rc;
    m->dispatched++;
    return PTMI_OK;
}

// the gather of the output buffer alone
int ptmi_multi_gather(ptmi_multi *m) {
    if (!m) return PTMI_E_INVALID;
    // one device without RCCL holds its frame whole, before any ptmi_multi_resize too (ptmi_multi_gather_planes asks for the size first)
    if (m->d.size() == 1 && m->comm.empty()) { mark_gathered(m, PTMI_MULTI_PLANE_OUTPUT); return PTMI_OK; }
    return ptmi_multi_gather_planes(m, PTMI_MULTI_PLANE_OUTPUT);
}

int ptmi_multi_synchronize(ptmi_multi *m) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_synchronize", ptmi_synchronize);
}

int ptmi_multi_throttle(ptmi_multi *m, uint32_t max_in_flight, uint32_t *in_flight) {
    if (!m) return PTMI_E_INVALID;
    uint32_t worst = 0;
    for (size_t i = 0; i < m->d.size(); i++) {
        uint32_t n = 0;
        int rc = ptmi_throttle(m->d[i].ctx, max_in_flight, &n);
        if (rc) return cfail(m, (int)i, rc, "ptmi_throttle");
        worst = std::max(worst, n);
    }
    if (in_flight) *in_flight = worst;
    return PTMI_OK;
}

int ptmi_multi_read_output(ptmi_multi *m, float *dst, size_t n_floats) {
    if (!m || !dst) return PTMI_E_INVALID;
    if (m->gathered != m->dispatched) { int rc = ptmi_multi_gather(m); if (rc) return rc; }
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    rc = ptmi_read_output(m->d[0].ctx, dst, n_floats);
    return rc ? cfail(m, 0, rc, "ptmi_read_output") : PTMI_OK;
}

int ptmi_multi_write_output(ptmi_multi *m, const float *src, size_t n_floats) {
    if (!m || !src) return PTMI_E_INVALID;
    int rc = each_ctx(m, "ptmi_write_output", ptmi_write_output, src, n_floats);
    if (rc) return rc;
    reset_counts(m, false);                   // every device holds the whole frame again: the rows may be dealt out anew
    return PTMI_OK;
}

int ptmi_multi_blit(ptmi_multi *m, float *dst_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes) {
    if (!m) return PTMI_E_INVALID;
    if (m->gathered != m->dispatched) { int rc = ptmi_multi_gather(m); if (rc) return rc; }
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    rc = ptmi_blit(m->d[0].ctx, dst_f32, n_floats, dst_rgba8, n_bytes);
    return rc ? cfail(m, 0, rc, "ptmi_blit") : PTMI_OK;
}

/* ---- planes, moments, adaptive rounds and the denoiser over the devices ---- */

int ptmi_multi_set_aovs(ptmi_multi *m, uint32_t mask) {
    if (!m) return PTMI_E_INVALID;
    if (mask & ~kAovAll) return mfail(m, PTMI_E_INVALID, "unknown AOV bits 0x%x", mask & ~kAovAll);     // once, before any device changes
    const int rc = each_ctx_or_back(m, "ptmi_set_aovs", ptmi_set_aovs, mask, m->aov_mask);
    if (rc) return rc;
    // a plane turned on is zero on every device, device 0's copy included: nothing to gather
    for (int k = 0; k < 3; k++) if (mask & ~m->aov_mask & kPlaneKinds[k].bit) m->gathered_plane[k] = m->dispatched;
    m->aov_mask = mask;
    return configure(m);
}
int ptmi_multi_get_aovs(const ptmi_multi *m, uint32_t *mask) {
    if (!m || !mask) return PTMI_E_INVALID;
    *mask = m->aov_mask;
    return PTMI_OK;
}
int ptmi_multi_set_moments(ptmi_multi *m, uint32_t on) {
    if (!m) return PTMI_E_INVALID;
    if (on > 1u) return mfail(m, PTMI_E_INVALID, "on = %u is not 0 or 1", on);
    const int rc = each_ctx_or_back(m, "ptmi_set_moments", ptmi_set_moments, on, m->moments_on ? 1u : 0u);
    if (rc) return rc;
    if (on && !m->moments_on) m->gathered_plane[3] = m->dispatched;
    m->moments_on = on != 0;
    return configure(m);
}
int ptmi_multi_get_moments(const ptmi_multi *m, uint32_t *on) {
    if (!m || !on) return PTMI_E_INVALID;
    *on = m->moments_on ? 1u : 0u;
    return PTMI_OK;
}

int ptmi_multi_set_projections(ptmi_multi *m, uint32_t on) {
    if (!m) return PTMI_E_INVALID;
    if (on > 1u) return mfail(m, PTMI_E_INVALID, "on = %u is not 0 or 1", on);
    return each_ctx(m, "ptmi_set_projections", ptmi_set_projections, on);
}
int ptmi_multi_get_projections(const ptmi_multi *m, uint32_t *on) {
    if (!m || !on) return PTMI_E_INVALID;
    return ptmi_get_projections(m->d[0].ctx, on);
}

int ptmi_multi_gather_planes(ptmi_multi *m, uint32_t planes) {
    if (!m) return PTMI_E_INVALID;
    if (planes & ~kGatherAll) return mfail(m, PTMI_E_INVALID, "unknown plane bits 0x%x", planes & ~kGatherAll);
    if (planes & ~planes_on(m)) return mfail(m, PTMI_E_STATE, "plane bits 0x%x name planes that are off", planes & ~planes_on(m));
    if (planes == 0) return PTMI_OK;
    if (m->W == 0) return mfail(m, PTMI_E_STATE, "no output buffer (ptmi_multi_resize)");
    if (m->d.size() == 1 && m->comm.empty()) { mark_gathered(m, planes); return PTMI_OK; }      // one device, no collective: its planes are the frame's
    return gather_set(m, planes);
}

int ptmi_multi_read_aov(ptmi_multi *m, uint32_t which, void *dst, size_t n_bytes) {
    if (!m) return PTMI_E_INVALID;
    // (a `which` that is not one plane, or one that is off, is ptmi_read_aov's to refuse: nothing is gathered for it)
    const uint32_t stale = stale_of(m, which & m->aov_mask);
    if (stale && !(which & (which - 1u)) && dst) { int rc = ptmi_multi_gather_planes(m, stale); if (rc) return rc; }
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    rc = ptmi_read_aov(m->d[0].ctx, which, dst, n_bytes);
    return rc ? cfail(m, 0, rc, "ptmi_read_aov") : PTMI_OK;
}

int ptmi_multi_read_moments(ptmi_multi *m, float *dst, size_t n_floats) {
    if (!m) return PTMI_E_INVALID;
    if (m->moments_on && dst && stale_of(m, PTMI_MULTI_PLANE_MOMENTS)) { int rc = ptmi_multi_gather_planes(m, PTMI_MULTI_PLANE_MOMENTS); if (rc) return rc; }
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    rc = ptmi_read_moments(m->d[0].ctx, dst, n_floats);
    return rc ? cfail(m, 0, rc, "ptmi_read_moments") : PTMI_OK;
}

int ptmi_multi_denoise(ptmi_multi *m, const ptmi_denoise_params *params, float *dst_rgba, size_t n_floats) {
    if (!m) return PTMI_E_INVALID;
    if (!(m->aov_mask & PTMI_AOV_NORMAL)) return mfail(m, PTMI_E_STATE, "the denoiser needs the NORMAL plane (ptmi_multi_set_aovs)");
    if (!m->moments_on) return mfail(m, PTMI_E_STATE, "the denoiser needs the moments plane (ptmi_multi_set_moments)");
    const uint32_t demodulate = params ? params->demodulate : 0u;
    uint32_t need = PTMI_MULTI_PLANE_OUTPUT | PTMI_AOV_NORMAL | PTMI_MULTI_PLANE_MOMENTS;
    if ((demodulate == 0u || demodulate == 2u) && (m->aov_mask & PTMI_AOV_ALBEDO)) need |= PTMI_AOV_ALBEDO;
    if (m->W != 0) {                                      // (before ptmi_multi_resize: ptmi_denoise's PTMI_E_STATE)
        const uint32_t stale = stale_of(m, need);
        if (stale) { int rc = ptmi_multi_gather_planes(m, stale); if (rc) return rc; }
    }
    // on device 0's stream, behind the unpack: the filter sees the whole frame
    const int rc = ptmi_denoise(m->d[0].ctx, params, dst_rgba, n_floats);
    return rc ? cfail(m, 0, rc, "ptmi_denoise") : PTMI_OK;
}

int ptmi_multi_blit_denoised(ptmi_multi *m, float *dst_f32, size_t n_floats, uint8_t *dst_rgba8, size_t n_bytes) {
    if (!m) return PTMI_E_INVALID;
    const int rc = ptmi_blit_denoised(m->d[0].ctx, dst_f32, n_floats, dst_rgba8, n_bytes);
    return rc ? cfail(m, 0, rc, "ptmi_blit_denoised") : PTMI_OK;
}

int ptmi_multi_dispatch_adaptive(ptmi_multi *m, const ptmi_camera *cam, const ptmi_adaptive_params *params, uint32_t rounds) {
    if (!m) return PTMI_E_INVALID;
    const int n = (int)m->d.size();
    ptmi_adaptive_params ap{};
    for (int i = 0; i < n; i++) {                         // checked once, on every device, before anything is enqueued
        const int rc = pt_adaptive_check(m->d[i].ctx, cam, params, &ap);
        if (rc) return cfail(m, i, rc, "ptmi_dispatch_adaptive");
    }
    if (rounds == 0) return PTMI_OK;
    if (ap.neighbourhood == 0u || (n == 1 && m->comm.empty())) {
        // selection is per pixel (or one device has the whole frame): every device runs all rounds on its own rows
        const int rc = each_threaded(m, "ptmi_dispatch_adaptive", [&](size_t i) { return ptmi_dispatch_adaptive(m->d[i].ctx, cam, params, rounds); });
        if (rc) return rc;
        m->dispatched++;
        return PTMI_OK;
    }
    // neighbourhood = 1: a pixel's neighbours may be another device's, so every round exchanges the NOISY flags of the whole frame
    const size_t share_px = m->rows_max * m->W, map_bytes = share_px * (size_t)n;
    if (m->flags_bytes != map_bytes) {
        for (int i = 0; i < n; i++) {
            MHIP(m, hipSetDevice(m->dev[i]));
            MultiDev &d = m->d[i];
            if (d.d_flags) { MHIP(m, hipStreamSynchronize(pt_ctx_stream(d.ctx))); MHIP(m, hipFree(d.d_flags)); d.d_flags = nullptr; }
            MHIP(m, hipMalloc(&d.d_flags, std::max<size_t>(map_bytes, 16)));
            d.flags_copied_recorded = false;
        }
        m->flags_bytes = map_bytes;
    }
    std::vector<uint8_t *> share(n, nullptr);
    for (uint32_t r = 0; r < rounds; r++) {
        for (int i = 0; i < n; i++) {
            MHIP(m, hipSetDevice(m->dev[i]));
            // loopback: every device has copied share i of the round before out of the plane it is written to again
            if (m->comm.empty())
                for (int d = 0; d < n; d++)
                    if (d != i && m->d[d].flags_copied_recorded) MHIP(m, hipStreamWaitEvent(pt_ctx_stream(m->d[i].ctx), m->d[d].ev_flags_copied, 0));
            const int rc = pt_adaptive_flags(m->d[i].ctx, &ap, r == 0 && cam->frame_index == 0u, &share[i]);
            if (rc) return cfail(m, i, rc, "ptmi_dispatch_adaptive (flags)");
            if (m->comm.empty()) MHIP(m, hipEventRecord(m->d[i].ev_flags, pt_ctx_stream(m->d[i].ctx)));
        }
        if (!m->comm.empty()) {
            MNCCL(m, g_rccl.GroupStart());
            for (int i = 0; i < n; i++) {
                ncclResult_t e = g_rccl.AllGather(share[i], m->d[i].d_flags, share_px, ncclUint8, m->comm[i], pt_ctx_stream(m->d[i].ctx));
                if (e != ncclSuccess) { (void)g_rccl.GroupEnd(); return mfail(m, PTMI_E_HIP, "ncclAllGather (device %d) failed: %s", i, g_rccl.GetErrorString(e)); }
            }
            MNCCL(m, g_rccl.GroupEnd());
        } else {
            for (int d = 0; d < n; d++) {
                MHIP(m, hipSetDevice(m->dev[d]));
                hipStream_t sd = pt_ctx_stream(m->d[d].ctx);
                for (int i = 0; i < n; i++) {
                    if (i != d) MHIP(m, hipStreamWaitEvent(sd, m->d[i].ev_flags, 0));
                    MHIP(m, hipMemcpyPeerAsync(m->d[d].d_flags + (size_t)i * share_px, m->dev[d], share[i], m->dev[i], share_px, sd));
                }
                MHIP(m, hipEventRecord(m->d[d].ev_flags_copied, sd));
                m->d[d].flags_copied_recorded = 1;
            }
        }
        const int rc = each_threaded(m, "ptmi_dispatch_adaptive (round)", [&](size_t i) {
            return pt_adaptive_round(m->d[i].ctx, cam, &ap, m->d[i].d_flags, (uint32_t)share_px, r == 0);
        });
        if (rc) return rc;
    }
    m->dispatched++;
    return PTMI_OK;
}

int ptmi_multi_adaptive_status(ptmi_multi *m, struct ptmi_adaptive_status *out) {
    if (!m || !out) return PTMI_E_INVALID;
    struct ptmi_adaptive_status sum{};
    bool first = true;
    for (size_t i = 0; i < m->d.size(); i++) {
        struct ptmi_adaptive_status s;
        const int rc = ptmi_adaptive_status(m->d[i].ctx, &s);
        if (rc) return cfail(m, (int)i, rc, "ptmi_adaptive_status");
        if (i == 0) sum.rounds = s.rounds;
        sum.active += s.active; sum.samples += s.samples;
        if (pt_band_of(options_of(m, (int)i), m->W, m->H).rows == 0) continue;       // a device without rows has no counts
        sum.min_count = first ? s.min_count : std::min(sum.min_count, s.min_count);
        sum.max_count = first ? s.max_count : std::max(sum.max_count, s.max_count);
        first = false;
    }
    *out = sum;
    return PTMI_OK;
}

int ptmi_multi_get_stats(ptmi_multi *m, ptmi_stats *out) {
    if (!m || !out) return PTMI_E_INVALID;
    ptmi_stats sum;
    for (size_t i = 0; i < m->d.size(); i++) {
        ptmi_stats s;
        int rc = ptmi_get_stats(m->d[i].ctx, &s);
        if (rc) return cfail(m, (int)i, rc, "ptmi_get_stats");
        if (i == 0) { sum = s; continue; }
        sum.paths += s.paths; sum.segments += s.segments; sum.shadow_rays += s.shadow_rays; sum.shadow_traced += s.shadow_traced;
        for (int b = 0; b < 64; b++) sum.segments_by_bounce[b] += s.segments_by_bounce[b];
        sum.gpu_ms = std::max(sum.gpu_ms, s.gpu_ms); sum.extend_ms = std::max(sum.extend_ms, s.extend_ms);
        sum.shade_ms = std::max(sum.shade_ms, s.shade_ms); sum.shadow_ms = std::max(sum.shadow_ms, s.shadow_ms);
        sum.raygen_ms = std::max(sum.raygen_ms, s.raygen_ms); sum.compact_ms = std::max(sum.compact_ms, s.compact_ms);
        sum.accumulate_ms = std::max(sum.accumulate_ms, s.accumulate_ms);
        sum.upload_ms = std::max(sum.upload_ms, s.upload_ms);
        sum.verify_failed += s.verify_failed;
    }
    *out = sum;
    return PTMI_OK;
}

int ptmi_multi_reset_stats(ptmi_multi *m) {
    if (!m) return PTMI_E_INVALID;
    return each_ctx(m, "ptmi_reset_stats", ptmi_reset_stats);
}

int ptmi_multi_gather_ms(ptmi_multi *m, double *ms) {
    if (!m || !ms) return PTMI_E_INVALID;
    *ms = -1.0;
    if (!m->gather_timed) return PTMI_OK;
    int rc = ptmi_multi_synchronize(m);
    if (rc) return rc;
    float f = 0.0f;
    MHIP(m, hipSetDevice(m->dev[0]));
    MHIP(m, hipEventElapsedTime(&f, m->g0, m->g1));
    *ms = f;
    return PTMI_OK;
}

}  // extern "C"
