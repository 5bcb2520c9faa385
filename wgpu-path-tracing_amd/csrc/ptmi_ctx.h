// ptmi_ctx.h — the context behind the C ABI of include/ptmi.h, and what the files that implement it share. Host code only; internal.
//   ptmi_api.hip       the context and its options, the frame planes, the batch arrays, output, statistics
//   scene_image.hip    scene validation, the traversal image, ptmi_upload_scene
//   traverse_pick.hip  which variant a traversal kernel runs as, and the launch of one
//   dispatch.hip       the wavefront dispatch loop, adaptive sampling, reprojection, event timing
//   debug_stages.hip   the per-stage debug entry points
//   environment.hip    the environment map: its tables, upload and removal, its debug entry points
//   medium.hip         the participating medium: its checks, installation and removal, its debug entry points
//   medium_grid.hip    the medium's density grid: its checks, upload and removal, its debug entry points
//   scene_update.hip   edits of a loaded scene in place: ptmi_update_triangles (the refit on the device), _materials, _lights
//   alpha.hip          alpha cutouts: the cutoff table, the two resolve loops between the existing kernels, their debug entry points
//   scene_rebuild.hip  the walked own-leaf tree rebuilt in place: the unit list on the device, the swap (ptmi_rebuild_tree)
//   motion.hip         reprojection across a geometry edit: the previous positions, their commit, the motion plane (ptmi_set_motion)
//   scene_transform.hip  triangle groups moved by matrix on the device: the table, the rest pose, the check and write passes
#pragma once
#include "ptmi.h"
#include "pt_device.h"

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

// what ptmi_multi.hip needs from a context
struct ptmi_ctx;
struct PtPrepared;               // a scene prepared on the host: validation + traversal image (scene_image.hip)
PtPrepared *pt_prepare_scene(ptmi_ctx *c, const ptmi_triangle *tris, uint32_t nt, const ptmi_material *mats, uint32_t nm,
                             const ptmi_bvh_node *nodes, uint32_t nn, const ptmi_light *lights, uint32_t nl, int *rc_out);
int pt_install_scene(ptmi_ctx *c, PtPrepared *p);            // allocates and copies on c's device; c keeps its old scene on failure
void pt_free_prepared(PtPrepared *p);
// bytes of a width x height atlas of `format` (ptmi_upload_atlas); PTMI_E_INVALID, with the reason in `why`, for an unknown
// format or a size that does not fit in size_t
int pt_atlas_bytes(uint32_t width, uint32_t height, int format, size_t *bytes, char *why, size_t why_len);
// the field checks of ptmi_set_medium (medium.hip): PTMI_E_INVALID with the reason in err; m NULL (removal) is fine
int pt_check_medium(const ptmi_medium *m, std::string &err);
// the optical-depth limit of a medium that carries a density grid (medium.hip): PTMI_E_UNSUPPORTED with the reason in err
int pt_check_medium_depth(const ptmi_medium *m, std::string &err);
// the argument checks of ptmi_upload_medium_density (medium_grid.hip), without a context: PTMI_E_INVALID with the reason in err;
// *st (may be NULL) = what ptmi_medium_grid_status reports for these values. Not called for a removal (rho NULL or a zero dimension).
int pt_check_medium_density(const float *rho, uint32_t nx, uint32_t ny, uint32_t nz, const ptmi_medium_grid *params,
                            struct ptmi_medium_grid_status *st, std::string &err);
// the medium of a context as it was set (NULL: none in place), and whether it carries a grid
const ptmi_medium *pt_ctx_medium(const ptmi_ctx *c);
bool pt_ctx_has_medium_grid(const ptmi_ctx *c);
// the argument checks of ptmi_set_alpha_cutoff that need no context (alpha.hip): PTMI_E_INVALID with the reason in err; cutoff NULL
// (removal) checks the params alone. And what its other checks compare with: whether c has a scene, and how many materials.
int pt_check_alpha_cutoff(const float *cutoff, uint32_t n_materials, const ptmi_alpha_params *params, std::string &err);
bool pt_ctx_has_scene(const ptmi_ctx *c);
uint32_t pt_ctx_materials(const ptmi_ctx *c);
hipStream_t pt_ctx_stream(ptmi_ctx *c);
int pt_ctx_device(const ptmi_ctx *c);
int pt_ctx_cus(const ptmi_ctx *c);
// the argument and state checks of ptmi_rebuild_tree (scene_rebuild.hip), which change nothing: its error codes, the reason in err
int pt_check_rebuild(const ptmi_ctx *c, const ptmi_rebuild_params *params, std::string &err);
// the argument and state checks of ptmi_set_triangle_groups and ptmi_transform_groups that run on the host (scene_transform.hip), which
// change nothing: their error codes, the reason in err. *n_groups_out (may be NULL): the largest id + 1.
int pt_check_triangle_groups(const ptmi_ctx *c, const uint32_t *group, uint32_t n_triangles, uint32_t *n_groups_out, std::string &err);
int pt_check_group_transforms(const ptmi_ctx *c, const ptmi_group_transform *ops, uint32_t n_ops, std::string &err);
// Adaptive rounds driven from outside, one at a time (ptmi_multi_dispatch_adaptive with neighbourhood = 1; dispatch.hip).
// pt_adaptive_check: everything ptmi_dispatch_adaptive checks before it enqueues, with its error codes; *ap = the params with their defaults.
int pt_adaptive_check(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *params, ptmi_adaptive_params *ap);
// restart: the band's counts go back to 0 first. Then the NOISY flag of every pixel of c's rows is written to c's flag share
// (*share_out: band-local pixel order, one byte each; DevFlagMap), on c's stream.
int pt_adaptive_flags(ptmi_ctx *c, const ptmi_adaptive_params *ap, bool restart, uint8_t **share_out);
// one round of ptmi_dispatch_adaptive with the selection taken from `map` (the shares of every device, device memory on c's device,
// share_px entries each). count_call: this round is the first of its ptmi_multi_dispatch_adaptive call (ptmi_stats.dispatches).
int pt_adaptive_round(ptmi_ctx *c, const ptmi_camera *cam, const ptmi_adaptive_params *ap, const uint8_t *map, uint32_t share_px,
                      bool count_call);

// What follows is shared by the files above only: hidden, so that the library exports the C ABI and the pt_* names and no helper.
// (A definition takes the visibility of the namespace block it stands in, so every block of pt_host is opened with PT_HOST.)
#define PT_HOST namespace pt_host __attribute__((visibility("hidden")))
PT_HOST {
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
    // the plan of ptmi_update_triangles (scene_update.hip), made at the first update after an upload, re-made by ptmi_rebuild_tree and
    // gone with the next upload:
    kPlanRefOrder, kPlanOrder,         // the nodes of kRefWnodes / kWnodes by height above their deepest leaf, lowest first
    kPlanQnum,                         // per node of kWnodes, its number in kQnodes
    kPlanUnits, kPlanExact,            // own leaves: the unit box of every listed triangle (leaf order); both exact child boxes per node
    kPlanWords,                        // the reduction words of one update and the partial sums of the cost
    kAlphaCutoff,                      // the per-material cutoff table of ptmi_set_alpha_cutoff (alpha.hip); gone with the next upload
    kMotionPrev,                       // the previous positions of ptmi_set_motion (motion.hip): 3 float4 per triangle; re-made by an upload
    // triangle groups (ptmi_set_triangle_groups; scene_transform.hip), gone with the next upload:
    kGroupTab,                         // one group id per uploaded triangle
    kGroupRest,                        // the rest pose: v0, v1, v2, n0, n1, n2 of every triangle, 6 float4 each
    kGroupOps,                         // the op records of the ptmi_transform_groups call at hand (grown on demand)
    kGroupMap,                         // 4 words (word 0: the smallest offending triangle of the check pass), then group -> op index
    kSceneBufs
};

// The per-pixel buffers that follow the output size, one entry each (ptmi_api.hip kFrame: what each takes and when it is made).
enum FramePlane {
    kOut,                                          // the context's own output buffer (binding 0)
    kAovAlbedo, kAovNormal, kAovId,                // first-hit planes (ptmi_set_aovs), in the order of the PTMI_AOV_* bits
    kMoments,                                      // sample moments (ptmi_set_moments)
    kDnGuide, kDnGrad, kDnA, kDnB, kDnOut,         // the denoiser's: guide (unit normal, depth), depth gradient, two ping-pong colour +
                                                   // variance planes, the result
    kAdBallot, kAdList, kAdTileSums,               // adaptive sampling: ballot words, pixel list, tile totals
    kAdFlags,                                      // ... over several devices: this context's share of the whole-frame flag map
    kRpOut, kRpMoments, kRpNormal, kRpAlbedo, kRpId,   // reprojection: the snapshot of the output, moments and first-hit planes
    kBlitF32, kBlitU8,                             // canvas staging of ptmi_blit
    kMotion,                                       // the motion plane of ptmi_set_motion: where each pixel's surface was in `from`
    kFramePlanes
};

// The per-path arrays of a batch, one entry each (ptmi_api.hip kLaneBytes: what each takes per path), in the order they are allocated.
enum LaneBuf {
    kPathO, kPathD, kPathC, kPathL,                // path state; L has room for either stride
    kHits,
    kShadow0, kShadowIdx0, kShadow1, kShadowIdx1,  // shadow records (SO, SD, SC in one block) and their index arrays, by bounce parity
    kTailO, kTailD, kTailC, kPid,                  // state by queue slot after the repack, and the path id of each such slot
    kQueue0, kQueue1,
    kOcc,                                          // occlusion bytes (ptmi_debug_occluded)
    kAovRec,                                       // first-hit records of bounce 0 (k_shade<true>); only while AOV planes are on
    kPathW, kTailW,                                // the environment's MIS weight of a bounce ray, by path and (after the repack) by queue
                                                   // slot; only while a sampled environment is in place
    kAlphaO, kAlphaD, kAlphaList0, kAlphaList1, kAlphaHits,   // alpha cutouts (pt_device.h DevAlpha): scratch rays, the two retry lists,
                                                   // scratch hits; only while a cutoff table with a positive entry is in place
    kLaneBufs
};

// A timed stretch of a stream: the two events around it and the statistic it adds to (dispatch.hip kEventStat).
enum EventKind { kDispatch, kExtend, kShade, kShadow, kRaygen, kCompact, kAccumulate, kEventKinds };
struct EventPair { hipEvent_t a, b; EventKind kind; };

}  // namespace pt_host
using namespace pt_host;

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
    uint32_t *word_off = nullptr;
    uint32_t *d_spill = nullptr;          // node-stack overflow of the global traversal variant (128 MiB on 256 CUs; first use)
    uint32_t *d_spill_side = nullptr;     // ... of the `shadow` kernel when it runs beside `extend`
    uint8_t *d_occ = nullptr;
    hipStream_t side = nullptr;           // `shadow` of bounce b beside the kernels of bounce b + 1
    hipEvent_t ev_ready = nullptr, ev_shadow[2] = {nullptr, nullptr};
    float4 *aov = nullptr;                // first-hit records of bounce 0, 32 B per path (k_shade<true>); only while AOV planes are on
    DevAlpha alpha{};                     // the alpha resolve loops' arrays (RO NULL: none); cutoff, control, stats and max_layers are set per use
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
    void *d_env = nullptr, *d_env_alias = nullptr;     // the environment map's texel and alias tables (DevScene::env points at them)
    double env_weight_sum = 0.0;                       // sum of the map's sampling weights (0: all black, never sampled)
    bool env_lookup_only = false;                      // ptmi_environment.sample = 1
    ptmi_medium medium{};                              // the medium as the caller gave it (ptmi_get_medium); DevScene::med.on: in place
    float *d_med_grid = nullptr;                       // the medium's density grid (DevScene::med.grid points at it; NULL: homogeneous)
    struct ptmi_medium_grid_status med_grid{};                // ... as ptmi_medium_grid_status reports it
    // alpha cutouts (ptmi_set_alpha_cutoff; alpha.hip): the table is buf[kAlphaCutoff], one float per material of the loaded scene
    bool alpha_present = false;                        // a table is in place
    uint32_t alpha_cutout = 0, alpha_layers = 0;       // its positive entries (0: inactive, no launch and no buffer differs); max_layers, resolved
    DevScene *d_scene = nullptr;                       // sc in device memory (DevScene::self), rewritten whenever sc changes
    DevScene sc{};
    bool have_scene = false;
    ptmi_image_info img{};                   // what the last upload (or rebuild) put on the device (ptmi_debug_read_image)
    uint32_t n_ref_wnodes = 0;               // wide nodes of the tree as uploaded (kRefWnodes)
    bool tree_nested = false;                // the uploaded tree was nested and finite: a hierarchy could be built over it
    // ptmi_update_triangles since the last upload (scene_update.hip): the level lists of the plan (level l of a list: entries
    // [off[l], off[l + 1])) and what ptmi_scene_update_status reports
    bool upd_planned = false;
    std::vector<uint32_t> upd_ref_off, upd_off;
    struct ptmi_scene_update_status upd{};
    struct ptmi_rebuild_status reb{};         // ptmi_rebuild_tree since the last upload (scene_rebuild.hip)

    // motion (ptmi_set_motion; motion.hip): the previous positions are buf[kMotionPrev], the plane is plane[kMotion]
    bool motion_on = false;
    uint32_t motion_epochs = 0;                        // commits since the last upload or ptmi_set_motion(1)
    uint32_t motion_dirty_first = 0, motion_dirty_count = 0;   // the union of the ranges updated since the last commit (0, 0: none)

    // triangle groups (ptmi_set_triangle_groups; scene_transform.hip): the table is buf[kGroupTab], the rest pose buf[kGroupRest]
    bool grp_present = false;
    size_t grp_ops_cap = 0;                            // op records buf[kGroupOps] has room for
    std::vector<uint32_t> grp_lo, grp_hi, grp_members; // per group: its lowest and highest member (lo > hi: none), how many it has
    std::vector<uint32_t> grp_map;                     // the host's copy of buf[kGroupMap], all "not named" between calls
    std::vector<uint8_t> grp_moved;                    // per group: a matrix is set (mats below holds it)
    std::vector<ptmi_group_transform> grp_mats;        // per group: its current matrix
    struct ptmi_transform_status tf{};                 // what ptmi_transform_status reports

    // output (binding 0)
    uint32_t W = 0, H = 0;
    void *plane[kFramePlanes] = {};                    // indexed by FramePlane, W x H pixels each (absent: NULL)
    float4 *d_out = nullptr;                           // what dispatches write: plane[kOut] or the caller's buffer (ptmi_bind_output_device)
    uint32_t aov_mask = 0;                             // ptmi_set_aovs: a plane is present while its bit is set and the output buffer exists
    bool moments_on = false;                           // ptmi_set_moments: likewise
    // the counter and control words (pt_device.h CounterWord, ControlWord): made and zeroed by ptmi_create
    unsigned long long *d_counters = nullptr;          // kCounterWords
    uint32_t *d_control = nullptr;                     // kControlWords
    // adaptive sampling (ptmi_dispatch_adaptive): ballot, list and tile_sums are views of the planes, control and counters of the two blocks
    DevAdaptive ad{};
    uint32_t ad_rounds = 0;                            // rounds since the last restart

    // statistics
    ptmi_stats st{};
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> event_pool;
    std::deque<hipEvent_t> in_flight;                  // one event per ptmi_dispatch, recorded behind its last kernel (ptmi_throttle)
};

PT_HOST {

extern thread_local std::string g_create_err;      // the error of a call that has no context (ptmi_last_error(NULL))
int fail(std::string &err, int code, const char *fmt, ...);
int fail(const ptmi_ctx *c, int code, const char *fmt, ...);
#define HIP_TRY(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail((c), PTMI_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

template <class T> void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }
// device scratch of one call (the ptmi_debug_*math entry points), freed on every way out of it
template <class T> struct Scratch { T *p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } };
template <class T> void view(T *&p, void *b) { p = static_cast<T *>(b); }      // a typed member that stands for an entry of a buffer table
template <class T> T *plane_as(const ptmi_ctx *c, FramePlane k) { return static_cast<T *>(c->plane[k]); }

// ptmi_api.hip
void default_options(ptmi_options &o);
hipError_t sync_all(ptmi_ctx *c);
size_t bytes_per_path(bool aov, bool env_w, bool alpha);
void lane_views(Lane &ln);
int ensure_capacity(ptmi_ctx *c, Lane &ln, size_t n);
enum PlaneGroup { kWithFrame, kByDenoise, kByAdaptive, kByReproject, kByBlit };     // when a plane is made (the kFrame table)
constexpr uint32_t bit(FramePlane k) { return 1u << k; }                            // sets of planes: a bit per FramePlane
uint32_t group_set(PlaneGroup g);
size_t plane_bytes(FramePlane k, size_t px);                                        // what plane k takes for px pixels
int make_planes(ptmi_ctx *c, uint32_t set, size_t px, void **into);
int check_ready(ptmi_ctx *c, bool need_output);

// dispatch.hip
void drain_events(ptmi_ctx *c);
hipError_t quiesce(ptmi_ctx *c);

// scene_update.hip: the plan of ptmi_update_triangles. make_plan reads the topology of both hierarchies as they stand and leaves the
// context's scene alone (a failure leaves no plan behind; the caller drops what is left); walked_cost: the cost of the walked hierarchy
// as it stands on the device (include/ptmi.h ptmi_scene_update_status), synchronises
void drop_plan(ptmi_ctx *c);
int make_plan(ptmi_ctx *c);
int walked_cost(ptmi_ctx *c, double &cost);
// What ptmi_update_triangles and ptmi_transform_groups share around the write of the records. refit_begin: the tree must be one a refit
// can serve (PTMI_E_UNSUPPORTED otherwise, nothing touched). refit_ready: waits for the work in flight and makes the plan at the first
// edit after an upload. refit_written: everything behind the write - the triangle images, the light triangles, both trees, the root
// boxes, the header, the cost and the status (updates grows by one; refit_ms counts from t0, when the entry point was entered).
int refit_begin(ptmi_ctx *c);
int refit_ready(ptmi_ctx *c);
int refit_written(ptmi_ctx *c, std::chrono::steady_clock::time_point t0);

// scene_transform.hip: the table goes with its scene (ptmi_upload_scene; the buffers have gone with the others); records
// [first, first + count) that ptmi_update_triangles has just written become the rest pose of their triangles, on c's stream
void groups_forget(ptmi_ctx *c);
int groups_rebase(ptmi_ctx *c, uint32_t first, uint32_t count);

// scene_image.hip: the own-leaf image of the loaded scene built anew from what is on the device (ptmi_rebuild_tree), by the code an
// upload builds it with. d_which: the unit list (n_units entries, device memory). buf: new device buffers for the entries a rebuild
// replaces (kWnodes, kTripos, kQnodes and the three 16-bit copies; absent: NULL), owned here until the swap takes them.
struct OwnRebuilt {
    void *buf[kSceneBufs] = {};
    ptmi_image_info img{};
    uint32_t q_top = 0, root_ref16 = 0xFFFFFFFFu, ref_root_ref16 = 0xFFFFFFFFu, builder_used = 0;
    OwnRebuilt() = default;
    OwnRebuilt(const OwnRebuilt &) = delete;
    OwnRebuilt &operator=(const OwnRebuilt &) = delete;
    ~OwnRebuilt() { for (void *p : buf) if (p) (void)hipFree(p); }
};
int rebuild_own_image(ptmi_ctx *c, const ptmi_options &opt, const uint32_t *d_which, uint32_t n_units, OwnRebuilt &out);

// motion.hip
// an upload or an update while motion is on: the previous positions filled from all of the device's triangles (dirty range and epochs
// cleared), on c's stream; the union of the dirty range with [first, first + count)
int motion_fill(ptmi_ctx *c);
void motion_widen(ptmi_ctx *c, uint32_t first, uint32_t count);
// copies the current positions over the dirty range, clears it and counts an epoch (ptmi_motion_commit; the end of ptmi_reproject)
int motion_commit(ptmi_ctx *c);
inline size_t motion_prev_bytes(uint32_t n_tris) { return n_tris ? (size_t)n_tris * 48u : 16u; }

// alpha.hip. Active: a table with a positive entry is in place; only then do the loops run and the lane carry their arrays.
inline bool alpha_active(const ptmi_ctx *c) { return c->alpha_cutout != 0u; }
// the path loop on the *count hit records `extend` (variant cfg) has just written for the rays p.O / p.D at queue[i] (NULL: i), on stream s
void alpha_resolve_paths(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, const uint32_t *queue, const uint32_t *count,
                         float2 *hits, uint32_t *layers_out);
// the shadow stage of a bounce in place of the any-hit kernel: `extend` on the records, then the shadow loop. hits0: room for the first
// trace's hits, one per queue entry (the bounce's hit array, which `shade` is done with)
void alpha_shadow_stage(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, DevShadow sh, const uint32_t *sq,
                        const uint32_t *count, float2 *hits0, uint8_t *occ_out, uint32_t *layers_out);

// traverse_pick.hip
bool walks_memory_quantised(const TraverseConfig &cfg);
// A traced launch in two steps, for the callers that have work between them (traverse_ready: both, for those that have none).
// traverse_pick chooses the variant of the extend (closest_hit) or the any-hit kernel and touches no device; PTMI_E_UNSUPPORTED: the
// option is PTMI_TRAVERSAL_LDS and the scene does not fit (extend only: the any-hit kernel is never refused).
// traverse_arm makes the spill area on first use, sets cfg.spill and (record) writes ptmi_stats.extend_variant / shadow_variant.
// Kernels that run at the same time need a spill area each, so every kernel has the lane's d_spill (kSpillMain) except the any-hit
// kernel of a dispatch: that one makes d_spill_side, and uses it beside `extend` on the side stream (kSpillSide); on the main stream
// (kSpillAfterExtend) it uses d_spill where extend's variant has made one, else d_spill_side.
enum SpillArea { kSpillMain, kSpillSide, kSpillAfterExtend };
int traverse_pick(const ptmi_ctx *c, bool closest_hit, TraverseConfig &cfg);
int traverse_arm(ptmi_ctx *c, bool closest_hit, SpillArea area, TraverseConfig &cfg, bool record);
int traverse_ready(ptmi_ctx *c, bool closest_hit, TraverseConfig &cfg);            // pick, then arm with d_spill, recorded
// the launch of either kernel on c->n_cu * 8 workgroups: the own-leaf launcher or the reference-leaf one, by the uploaded scene
void launch_extend(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, const uint32_t *queue, const uint32_t *count,
                   float2 *hits);
void launch_shadow(ptmi_ctx *c, hipStream_t s, const TraverseConfig &cfg, DevPaths p, DevShadow sh, const uint32_t *shadow_queue,
                   const uint32_t *count, uint8_t *occluded_out);
}  // namespace pt_host
