/*
 * ptmi_napi.c — thin N-API (Node >= 12, N-API 4) addon over the C ABI of include/ptmi.h.
 *
 * One JS function per operation, for both handle types: create(device) and multiCreate([ordinal, ...], flags) return a
 * handle, and every other function calls ptmi_X or ptmi_multi_X by the kind of handle it is given. Scene / camera blobs
 * travel as ArrayBuffers (or typed-array views) in the exact WGSL layouts the reference writes with
 * device.queue.writeBuffer (src/renderer/renderer.ts:242-355, :403-413). A non-zero ptmi status becomes a JS Error
 * "<C function> failed (<rc>): <ptmi_last_error or ptmi_multi_last_error>"; anything but a live handle is a TypeError
 * before any library call. No rendering logic lives here.
 *
 * build: oracle-free, see Makefile next to this file
 *   gcc -shared -fPIC -I/usr/include/node -I../../../include ptmi_napi.c -L../../lib -lptmi
 */
#define NAPI_VERSION 4
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ptmi.h"
#include "ptmi_scene.h"

#define NAPI_OK(env, call)                                                        \
    do {                                                                          \
        if ((call) != napi_ok) {                                                  \
            napi_throw_error((env), NULL, "N-API call failed: " #call);           \
            return NULL;                                                          \
        }                                                                         \
    } while (0)

/* What a JS handle points at: which library type, and the library object (NULL once destroy() has run). The kinds are
 * unlikely bit patterns, so that get_handle can tell this record from another addon's external. */
enum { KIND_CTX = 0x70746d31, KIND_MULTI = 0x70746d4e };
typedef struct {
    uint32_t kind;
    union { void *p; ptmi_ctx *ctx; ptmi_multi *m; };
} handle;

/* ptmi_<fn>(ctx, ...) or ptmi_multi_<fn>(m, ...), by the handle's kind */
#define RUN(h, fn, ...) ((h)->kind == KIND_MULTI ? ptmi_multi_##fn((h)->m, ##__VA_ARGS__) : ptmi_##fn((h)->ctx, ##__VA_ARGS__))
/* RUN, and a non-zero status throws, naming the function that ran */
#define CALL(env, h, fn, ...)                                                                                   \
    do {                                                                                                        \
        int rc_ = RUN(h, fn, ##__VA_ARGS__);                                                                    \
        if (rc_) return throw_ptmi((env), (h), rc_, (h)->kind == KIND_MULTI ? "ptmi_multi_" #fn : "ptmi_" #fn); \
    } while (0)

static napi_value throw_ptmi(napi_env env, const handle *h, int rc, const char *what) {
    char buf[768];
    snprintf(buf, sizeof buf, "%s failed (%d): %s", what, rc,
             h->kind == KIND_MULTI ? ptmi_multi_last_error(h->m) : ptmi_last_error(h->ctx));
    napi_throw_error(env, "PTMI", buf);
    return NULL;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    return 1;
}

/* the finalizer frees the record only: the library object lives until destroy() */
static void free_handle(napi_env env, void *data, void *hint) {
    (void)env; (void)hint;
    free(data);
}

static napi_value new_handle(napi_env env, uint32_t kind, void *p) {
    handle *h = malloc(sizeof *h);
    napi_value ext;
    if (!h) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    h->kind = kind; h->p = p;
    if (napi_create_external(env, h, free_handle, NULL, &ext) != napi_ok) {
        free(h);
        napi_throw_error(env, NULL, "N-API call failed: napi_create_external");
        return NULL;
    }
    return ext;
}

/* the call's arguments, and the live handle in the first; NULL after throwing a TypeError */
static handle *get_handle(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    void *p = NULL;
    handle *h = NULL;
    if (!get_args(env, info, want, argv)) return NULL;
    if (napi_get_value_external(env, argv[0], &p) == napi_ok) h = p;
    if (!h || (h->kind != KIND_CTX && h->kind != KIND_MULTI) || !h->p) {
        napi_throw_type_error(env, NULL, "expected a ptmi handle from create() or multiCreate() that has not been destroyed");
        return NULL;
    }
    return h;
}

/* ArrayBuffer or TypedArray/DataView -> (pointer, byte length); null/undefined -> (NULL, 0) */
static int get_bytes(napi_env env, napi_value v, void **data, size_t *len) {
    napi_valuetype t;
    bool is;
    *data = NULL; *len = 0;
    if (napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined)) return 1;
    if (napi_is_arraybuffer(env, v, &is) == napi_ok && is) return napi_get_arraybuffer_info(env, v, data, len) == napi_ok;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type tt; size_t n; napi_value ab; size_t off;
        if (napi_get_typedarray_info(env, v, &tt, &n, data, &ab, &off) != napi_ok) return 0;
        static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        *len = n * esz[tt];
        return 1;
    }
    if (napi_is_dataview(env, v, &is) == napi_ok && is) {
        napi_value ab; size_t off;
        return napi_get_dataview_info(env, v, len, data, &ab, &off) == napi_ok;
    }
    napi_throw_type_error(env, NULL, "expected an ArrayBuffer or a typed array");
    return 0;
}

static uint32_t get_u32_prop(napi_env env, napi_value obj, const char *name, uint32_t dflt) {
    napi_value v; bool has = false; uint32_t out = dflt;
    if (napi_has_named_property(env, obj, name, &has) == napi_ok && has &&
        napi_get_named_property(env, obj, name, &v) == napi_ok)
        napi_get_value_uint32(env, v, &out);
    return out;
}

static napi_value js_create(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    int32_t dev = 0;
    NAPI_OK(env, napi_get_value_int32(env, argv[0], &dev));
    ptmi_ctx *ctx = NULL;
    int rc = ptmi_create(dev, &ctx);
    if (rc) return throw_ptmi(env, &(handle){.kind = KIND_CTX}, rc, "ptmi_create");
    return new_handle(env, KIND_CTX, ctx);
}

/* multiCreate([ordinal, ...], flags) */
static napi_value js_multi_create(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    uint32_t n = 0, flags = 0;
    bool is_array = false;
    if (napi_is_array(env, argv[0], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[0], &n) != napi_ok || n < 1 || n > 64) {
        napi_throw_type_error(env, NULL, "expected an array of 1..64 device ordinals");
        return NULL;
    }
    int dev[64];
    for (uint32_t i = 0; i < n; i++) {
        napi_value e; int32_t d = 0;
        NAPI_OK(env, napi_get_element(env, argv[0], i, &e));
        NAPI_OK(env, napi_get_value_int32(env, e, &d));
        dev[i] = d;
    }
    napi_get_value_uint32(env, argv[1], &flags);
    ptmi_multi *m = NULL;
    int rc = ptmi_multi_create((int)n, dev, flags, &m);
    if (rc) return throw_ptmi(env, &(handle){.kind = KIND_MULTI}, rc, "ptmi_multi_create");
    return new_handle(env, KIND_MULTI, m);
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    (void)RUN(h, destroy);
    h->p = NULL;
    return NULL;
}

static napi_value js_upload_scene(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    handle *h = get_handle(env, info, 5, argv);
    if (!h) return NULL;
    void *p[4]; size_t n[4];
    static const size_t stride[4] = {sizeof(ptmi_triangle), sizeof(ptmi_material), sizeof(ptmi_bvh_node), sizeof(ptmi_light)};
    for (int i = 0; i < 4; i++) {
        if (!get_bytes(env, argv[1 + i], &p[i], &n[i])) return NULL;
        if (n[i] % stride[i]) { napi_throw_range_error(env, NULL, "blob length is not a multiple of its element size"); return NULL; }
    }
    CALL(env, h, upload_scene, (const ptmi_triangle *)p[0], (uint32_t)(n[0] / stride[0]),
         (const ptmi_material *)p[1], (uint32_t)(n[1] / stride[1]),
         (const ptmi_bvh_node *)p[2], (uint32_t)(n[2] / stride[2]),
         (const ptmi_light *)p[3], (uint32_t)(n[3] / stride[3]));
    return NULL;
}

static napi_value js_upload_atlas(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    handle *h = get_handle(env, info, 5, argv);
    if (!h) return NULL;
    void *p; size_t n; uint32_t w = 0, hh = 0; int32_t fmt = 0;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &w); napi_get_value_uint32(env, argv[3], &hh); napi_get_value_int32(env, argv[4], &fmt);
    if (p && n < (size_t)w * hh * (fmt == PTMI_ATLAS_RGBA16F ? 8 : 16)) { napi_throw_range_error(env, NULL, "atlas buffer too small"); return NULL; }
    CALL(env, h, upload_atlas, p, w, hh, fmt);
    return NULL;
}

/* uploadEnvironment(handle, float32 RGBA texels | null, width, height, {intensity, rotation (radians), sample}) */
static napi_value js_upload_environment(napi_env env, napi_callback_info info) {
    napi_value argv[5], v;
    handle *h = get_handle(env, info, 5, argv);
    if (!h) return NULL;
    void *p; size_t n; uint32_t w = 0, hh = 0; double d;
    ptmi_environment prm = {0};
    napi_valuetype t;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &w); napi_get_value_uint32(env, argv[3], &hh);
    if (napi_typeof(env, argv[4], &t) == napi_ok && t == napi_object) {
        if (napi_get_named_property(env, argv[4], "intensity", &v) == napi_ok && napi_get_value_double(env, v, &d) == napi_ok) prm.intensity = (float)d;
        if (napi_get_named_property(env, argv[4], "rotation", &v) == napi_ok && napi_get_value_double(env, v, &d) == napi_ok) prm.rotation = (float)d;
        prm.sample = get_u32_prop(env, argv[4], "sample", 0);
    }
    if (p && n / 16 / (w ? w : 1) < hh) { napi_throw_range_error(env, NULL, "environment buffer too small"); return NULL; }
    CALL(env, h, upload_environment, p, w, hh, PTMI_ATLAS_RGBA32F, &prm);
    return NULL;
}

/* a number property of obj into *out; 0 when it is absent or not a number */
static int get_float_prop(napi_env env, napi_value obj, const char *name, float *out) {
    napi_value v; double d;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok || napi_get_value_double(env, v, &d) != napi_ok) return 0;
    *out = (float)d;
    return 1;
}
/* an array property of three numbers */
static int get_float3_prop(napi_env env, napi_value obj, const char *name, float out[3]) {
    napi_value arr, v; double d;
    if (napi_get_named_property(env, obj, name, &arr) != napi_ok) return 0;
    for (uint32_t k = 0; k < 3; k++) {
        if (napi_get_element(env, arr, k, &v) != napi_ok || napi_get_value_double(env, v, &d) != napi_ok) return 0;
        out[k] = (float)d;
    }
    return 1;
}

/* setMedium(handle, {sigmaT, albedo: [r, g, b], g, min: [x, y, z], max: [x, y, z]} | null): ptmi_set_medium; null removes it */
static napi_value js_set_medium(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    napi_valuetype t = napi_undefined;
    if (napi_typeof(env, argv[1], &t) != napi_ok) t = napi_undefined;
    if (t == napi_null || t == napi_undefined) {
        CALL(env, h, set_medium, NULL);
        return NULL;
    }
    ptmi_medium m = {0};
    if (t != napi_object || !get_float_prop(env, argv[1], "sigmaT", &m.sigma_t) || !get_float3_prop(env, argv[1], "albedo", m.albedo) ||
        !get_float_prop(env, argv[1], "g", &m.g) || !get_float3_prop(env, argv[1], "min", m.box_min) ||
        !get_float3_prop(env, argv[1], "max", m.box_max)) {
        napi_throw_type_error(env, NULL, "setMedium: expected {sigmaT, albedo: [3], g, min: [3], max: [3]} or null");
        return NULL;
    }
    CALL(env, h, set_medium, &m);
    return NULL;
}

/* uploadMediumDensity(handle, Float32Array | null, [nx, ny, nz], filter): ptmi_upload_medium_density; null or a zero dimension removes the grid */
static napi_value js_upload_medium_density(napi_env env, napi_callback_info info) {
    napi_value argv[4], v;
    handle *h = get_handle(env, info, 4, argv);
    if (!h) return NULL;
    void *p; size_t n; uint32_t dim[3] = {0, 0, 0};
    ptmi_medium_grid prm = {0};
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    for (uint32_t k = 0; p && k < 3; k++)
        if (napi_get_element(env, argv[2], k, &v) != napi_ok || napi_get_value_uint32(env, v, &dim[k]) != napi_ok) {
            napi_throw_type_error(env, NULL, "uploadMediumDensity: expected the dimensions [nx, ny, nz]");
            return NULL;
        }
    napi_get_value_uint32(env, argv[3], &prm.filter);
    /* (dimensions above the limit are the library's to refuse: only what it would read is checked here) */
    if (p && dim[0] <= 1024 && dim[1] <= 1024 && dim[2] <= 1024 && n / 4 < (size_t)dim[0] * dim[1] * dim[2]) {
        napi_throw_range_error(env, NULL, "density buffer too small");
        return NULL;
    }
    CALL(env, h, upload_medium_density, (const float *)p, dim[0], dim[1], dim[2], &prm);
    return NULL;
}

/* updateTriangles / updateMaterials / updateLights(handle, first, blob): ptmi_update_*; the blob holds whole records in the upload's layout */
#define JS_UPDATE(name, fn, type)                                                                                              \
    static napi_value name(napi_env env, napi_callback_info info) {                                                            \
        napi_value argv[3];                                                                                                    \
        handle *h = get_handle(env, info, 3, argv);                                                                            \
        if (!h) return NULL;                                                                                                   \
        void *p; size_t n; uint32_t first = 0;                                                                                 \
        NAPI_OK(env, napi_get_value_uint32(env, argv[1], &first));                                                             \
        if (!get_bytes(env, argv[2], &p, &n)) return NULL;                                                                     \
        if (n % sizeof(type)) { napi_throw_range_error(env, NULL, "blob length is not a multiple of its element size"); return NULL; } \
        CALL(env, h, fn, first, (uint32_t)(n / sizeof(type)), (const type *)p);                                                \
        return NULL;                                                                                                           \
    }
JS_UPDATE(js_update_triangles, update_triangles, ptmi_triangle)
JS_UPDATE(js_update_materials, update_materials, ptmi_material)
JS_UPDATE(js_update_lights, update_lights, ptmi_light)

/* sceneUpdateStatus(handle) -> {updates, quantisedKept, planMs, refitMs, costBuilt, costNow, rootMin: [3], rootMax: [3]} */
static napi_value js_scene_update_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v, arr[2];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_scene_update_status st;
    CALL(env, h, scene_update_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"updates", st.updates}, {"quantisedKept", st.quantised_kept}, {"planMs", st.plan_ms}, {"refitMs", st.refit_ms},
        {"costBuilt", st.cost_built}, {"costNow", st.cost_now}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    for (int side = 0; side < 2; side++) {
        NAPI_OK(env, napi_create_array_with_length(env, 3, &arr[side]));
        for (uint32_t k = 0; k < 3; k++) {
            NAPI_OK(env, napi_create_double(env, side ? st.root_max[k] : st.root_min[k], &v));
            NAPI_OK(env, napi_set_element(env, arr[side], k, v));
        }
    }
    NAPI_OK(env, napi_set_named_property(env, out, "rootMin", arr[0]));
    NAPI_OK(env, napi_set_named_property(env, out, "rootMax", arr[1]));
    return out;
}

/* setTriangleGroups(handle, Uint32Array | null): ptmi_set_triangle_groups; one id per uploaded triangle, null removes the table */
static napi_value js_set_triangle_groups(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (n % sizeof(uint32_t)) { napi_throw_range_error(env, NULL, "the group table is not whole uint32 words"); return NULL; }
    CALL(env, h, set_triangle_groups, (const uint32_t *)p, (uint32_t)(n / sizeof(uint32_t)));
    return NULL;
}

/* transformGroups(handle, blob): ptmi_transform_groups; the blob holds whole 96-byte ptmi_group_transform records */
static napi_value js_transform_groups(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (n % sizeof(ptmi_group_transform)) { napi_throw_range_error(env, NULL, "blob length is not a multiple of 96 bytes"); return NULL; }
    CALL(env, h, transform_groups, (const ptmi_group_transform *)p, (uint32_t)(n / sizeof(ptmi_group_transform)));
    return NULL;
}

/* normalMatrix(handle, Float32Array(12) m, Float32Array(9) out): ptmi_normal_matrix. The library function needs no context; the handle
 * is asked for like everywhere else, so that every export but the constructors takes one. */
static napi_value js_normal_matrix(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_handle(env, info, 3, argv)) return NULL;
    void *m, *nm; size_t nm_bytes, m_bytes;
    if (!get_bytes(env, argv[1], &m, &m_bytes) || !get_bytes(env, argv[2], &nm, &nm_bytes)) return NULL;
    if (m_bytes != 12 * sizeof(float) || nm_bytes != 9 * sizeof(float)) {
        napi_throw_range_error(env, NULL, "normalMatrix: expected a Float32Array(12) and a Float32Array(9)");
        return NULL;
    }
    ptmi_normal_matrix((const float *)m, (float *)nm);
    return NULL;
}

/* transformStatus(handle) -> {present, nGroups, transforms, lastMoved, firstBad, transformMs} */
static napi_value js_transform_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_transform_status st;
    CALL(env, h, transform_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"present", st.present}, {"nGroups", st.n_groups}, {"transforms", st.transforms}, {"lastMoved", st.last_moved},
        {"firstBad", st.first_bad}, {"transformMs", st.transform_ms}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

/* setSkin(handle, Uint32Array | null triangles, corners blob | null, nJoints): ptmi_set_skin; the blob holds three 32-byte
 * ptmi_skin_corner records per listed triangle; null triangles remove the skin */
static napi_value js_set_skin(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_handle(env, info, 4, argv);
    if (!h) return NULL;
    void *t, *c; size_t tn, cn;
    uint32_t n_joints = 0;
    if (!get_bytes(env, argv[1], &t, &tn) || !get_bytes(env, argv[2], &c, &cn)) return NULL;
    NAPI_OK(env, napi_get_value_uint32(env, argv[3], &n_joints));
    if (tn % sizeof(uint32_t)) { napi_throw_range_error(env, NULL, "the triangle list is not whole uint32 words"); return NULL; }
    if (c && cn != tn / sizeof(uint32_t) * 3 * sizeof(ptmi_skin_corner)) {
        napi_throw_range_error(env, NULL, "the corner blob does not hold three 32-byte records per listed triangle");
        return NULL;
    }
    CALL(env, h, set_skin, (const uint32_t *)t, (const ptmi_skin_corner *)c, (uint32_t)(tn / sizeof(uint32_t)), n_joints);
    return NULL;
}

/* poseSkin(handle, blob): ptmi_pose_skin; the blob holds one 96-byte ptmi_joint_transform record per joint, in joint order */
static napi_value js_pose_skin(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (n % sizeof(ptmi_joint_transform)) { napi_throw_range_error(env, NULL, "blob length is not a multiple of 96 bytes"); return NULL; }
    CALL(env, h, pose_skin, (const ptmi_joint_transform *)p, (uint32_t)(n / sizeof(ptmi_joint_transform)));
    return NULL;
}

/* skinStatus(handle) -> {present, nJoints, nSkinned, poses, firstBad, poseMs} */
static napi_value js_skin_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_skin_status st;
    CALL(env, h, skin_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"present", st.present}, {"nJoints", st.n_joints}, {"nSkinned", st.n_skinned}, {"poses", st.poses},
        {"firstBad", st.first_bad}, {"poseMs", st.pose_ms}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

/* setMorph(handle, Uint32Array | null triangles, Uint32Array | null rowStart, deltas blob | null, nTargets): ptmi_set_morph; rowStart
 * holds one word more than triangles, the blob whole 96-byte ptmi_morph_delta records, as many as rowStart's last word; null
 * triangles remove the morph */
static napi_value js_set_morph(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    handle *h = get_handle(env, info, 5, argv);
    if (!h) return NULL;
    void *t, *r, *d; size_t tn, rn, dn;
    uint32_t n_targets = 0;
    if (!get_bytes(env, argv[1], &t, &tn) || !get_bytes(env, argv[2], &r, &rn) || !get_bytes(env, argv[3], &d, &dn)) return NULL;
    NAPI_OK(env, napi_get_value_uint32(env, argv[4], &n_targets));
    if (tn % sizeof(uint32_t)) { napi_throw_range_error(env, NULL, "the triangle list is not whole uint32 words"); return NULL; }
    if (t && r && rn != tn + sizeof(uint32_t)) {
        napi_throw_range_error(env, NULL, "rowStart does not hold one word more than the triangle list");
        return NULL;
    }
    if (d && dn % sizeof(ptmi_morph_delta)) { napi_throw_range_error(env, NULL, "the delta blob is not whole 96-byte records"); return NULL; }
    if (t && r && tn && ((const uint32_t *)r)[tn / sizeof(uint32_t)] > (d ? dn / sizeof(ptmi_morph_delta) : 0)) {
        napi_throw_range_error(env, NULL, "rowStart reaches beyond the delta blob");
        return NULL;
    }
    CALL(env, h, set_morph, (const uint32_t *)t, (const uint32_t *)r, (const ptmi_morph_delta *)d, (uint32_t)(tn / sizeof(uint32_t)), n_targets);
    return NULL;
}

/* poseMorph(handle, Float32Array weights): ptmi_pose_morph; one weight per target */
static napi_value js_pose_morph(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (n % sizeof(float)) { napi_throw_range_error(env, NULL, "the weights are not whole float32 words"); return NULL; }
    CALL(env, h, pose_morph, (const float *)p, (uint32_t)(n / sizeof(float)));
    return NULL;
}

/* morphStatus(handle) -> {present, nTargets, nMorphed, nRecords, nInSkin, poses, activeTargets, firstBad, skinStale, poseMs} */
static napi_value js_morph_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_morph_status st;
    CALL(env, h, morph_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"present", st.present}, {"nTargets", st.n_targets}, {"nMorphed", st.n_morphed}, {"nRecords", st.n_records},
        {"nInSkin", st.n_in_skin}, {"poses", st.poses}, {"activeTargets", st.active_targets}, {"firstBad", st.first_bad},
        {"skinStale", st.skin_stale}, {"poseMs", st.pose_ms}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

/* rebuildStatus(handle) -> {rebuilds, builderUsed, buildMs, costBefore, costAfter} */
static napi_value js_rebuild_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_rebuild_status st;
    CALL(env, h, rebuild_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"rebuilds", st.rebuilds}, {"builderUsed", st.builder_used}, {"buildMs", st.build_ms},
        {"costBefore", st.cost_before}, {"costAfter", st.cost_after}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

/* rebuildTree(handle, builder): ptmi_rebuild_tree; builder 0 picks the default */
static napi_value js_rebuild_tree(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    ptmi_rebuild_params prm = {0};
    napi_get_value_uint32(env, argv[1], &prm.builder);
    CALL(env, h, rebuild_tree, &prm);
    return NULL;
}

/* setAlphaCutoff(handle, Float32Array | null, maxLayers): ptmi_set_alpha_cutoff; one cutoff per uploaded material, null removes the table */
static napi_value js_set_alpha_cutoff(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_handle(env, info, 3, argv);
    if (!h) return NULL;
    void *p; size_t n;
    ptmi_alpha_params prm = {0};
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &prm.max_layers);
    if (n % sizeof(float)) { napi_throw_range_error(env, NULL, "cutoff table is not whole floats"); return NULL; }
    CALL(env, h, set_alpha_cutoff, (const float *)p, (uint32_t)(n / sizeof(float)), &prm);
    return NULL;
}

/* alphaStatus(handle) -> {present, materials, cutout, maxLayers, pathPasses, pathExhausted, shadowPasses, shadowExhausted} */
static napi_value js_alpha_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_alpha_status st;
    CALL(env, h, alpha_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"present", st.present}, {"materials", st.n_materials}, {"cutout", st.n_cutout}, {"maxLayers", st.max_layers},
        {"pathPasses", (double)st.path_passes}, {"pathExhausted", (double)st.path_exhausted},
        {"shadowPasses", (double)st.shadow_passes}, {"shadowExhausted", (double)st.shadow_exhausted}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

/* setAlphaBlend(handle, Float32Array | null, maxLayers, seed): ptmi_set_alpha_blend; one entry per uploaded material, null removes the table */
static napi_value js_set_alpha_blend(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_handle(env, info, 4, argv);
    if (!h) return NULL;
    void *p; size_t n;
    ptmi_alpha_blend_params prm = {0};
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &prm.max_layers);
    napi_get_value_uint32(env, argv[3], &prm.seed);
    if (n % sizeof(float)) { napi_throw_range_error(env, NULL, "blend table is not whole floats"); return NULL; }
    CALL(env, h, set_alpha_blend, (const float *)p, (uint32_t)(n / sizeof(float)), &prm);
    return NULL;
}

/* alphaBlendStatus(handle) -> {present, materials, blend, maxLayers, seed, pathTests, pathPasses, shadowTests, shadowPasses} */
static napi_value js_alpha_blend_status(napi_env env, napi_callback_info info) {
    napi_value argv[1], out, v;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_alpha_blend_status st;
    CALL(env, h, alpha_blend_status, &st);
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; double value; } num[] = {
        {"present", st.present}, {"materials", st.n_materials}, {"blend", st.n_blend}, {"maxLayers", st.max_layers}, {"seed", st.seed},
        {"pathTests", (double)st.path_tests}, {"pathPasses", (double)st.path_passes},
        {"shadowTests", (double)st.shadow_tests}, {"shadowPasses", (double)st.shadow_passes}};
    for (size_t i = 0; i < sizeof num / sizeof num[0]; i++) {
        NAPI_OK(env, napi_create_double(env, num[i].value, &v));
        NAPI_OK(env, napi_set_named_property(env, out, num[i].name, v));
    }
    return out;
}

static napi_value js_resize(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_handle(env, info, 3, argv);
    if (!h) return NULL;
    uint32_t w = 0, hh = 0;
    napi_get_value_uint32(env, argv[1], &w); napi_get_value_uint32(env, argv[2], &hh);
    CALL(env, h, resize, w, hh);
    return NULL;
}

/* setOptions(h, {maxBounces, doMis, ...}): JS option names -> ptmi_options; unset properties keep their current values */
static napi_value js_set_options(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    ptmi_options o;
    (void)RUN(h, get_options, &o);
    /* several devices: the library deals out the rows, unless tileStrip says otherwise */
    if (h->kind == KIND_MULTI) { o.tile_parts = 0; o.tile_part = 0; o.tile_strip = 0; }
    napi_value js = argv[1];
    o.max_bounces = get_u32_prop(env, js, "maxBounces", o.max_bounces);
    o.do_mis = get_u32_prop(env, js, "doMis", o.do_mis);
    o.tile_y0 = get_u32_prop(env, js, "tileY0", o.tile_y0);
    o.tile_y1 = get_u32_prop(env, js, "tileY1", o.tile_y1);
    o.frames_per_batch = get_u32_prop(env, js, "framesPerBatch", o.frames_per_batch);
    o.traversal = get_u32_prop(env, js, "traversal", o.traversal);
    o.cull = get_u32_prop(env, js, "cull", o.cull);
    o.timing = get_u32_prop(env, js, "timing", o.timing);
    o.keep_reference_tree = get_u32_prop(env, js, "keepReferenceTree", o.keep_reference_tree);
    o.tile_parts = get_u32_prop(env, js, "tileParts", o.tile_parts);
    o.tile_part = get_u32_prop(env, js, "tilePart", o.tile_part);
    o.tile_strip = get_u32_prop(env, js, "tileStrip", o.tile_strip);
    o.perf_mode = get_u32_prop(env, js, "perfMode", o.perf_mode);
    o.overlap = get_u32_prop(env, js, "overlap", o.overlap);
    o.tree_builder = get_u32_prop(env, js, "treeBuilder", o.tree_builder);
    o.leaves = get_u32_prop(env, js, "leaves", o.leaves);
    o.leaf_tris = get_u32_prop(env, js, "leafTris", o.leaf_tris);
    CALL(env, h, set_options, &o);
    return NULL;
}

static napi_value js_dispatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_handle(env, info, 3, argv);
    if (!h) return NULL;
    void *p; size_t n; uint32_t frames = 1;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!p || n != sizeof(ptmi_camera)) { napi_throw_range_error(env, NULL, "camera blob must be 96 bytes"); return NULL; }
    napi_get_value_uint32(env, argv[2], &frames);
    ptmi_camera cam;
    memcpy(&cam, p, sizeof cam);
    CALL(env, h, dispatch, &cam, frames);
    return NULL;
}

/* gather(h): several devices assemble the frame on the first; one device has nothing to do */
static napi_value js_gather(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    int rc = h->kind == KIND_MULTI ? ptmi_multi_gather(h->m) : PTMI_OK;
    if (rc) return throw_ptmi(env, h, rc, "ptmi_multi_gather");
    return NULL;
}

/* gatherPlanes(h, bits): PTMI_AOV_* | PTMI_MULTI_PLANE_*; several devices assemble those planes on the first in one pass */
static napi_value js_gather_planes(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    uint32_t planes = 0;
    napi_get_value_uint32(env, argv[1], &planes);
    int rc = h->kind == KIND_MULTI ? ptmi_multi_gather_planes(h->m, planes) : PTMI_OK;
    if (rc) return throw_ptmi(env, h, rc, "ptmi_multi_gather_planes");
    return NULL;
}

static napi_value js_synchronize(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    CALL(env, h, synchronize);
    return NULL;
}

/* throttle(h, maxInFlight) -> dispatches still in flight (blocks until at most maxInFlight are) */
static napi_value js_throttle(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    uint32_t max = 0, n = 0;
    napi_get_value_uint32(env, argv[1], &max);
    CALL(env, h, throttle, max, &n);
    napi_value v;
    NAPI_OK(env, napi_create_uint32(env, n, &v));
    return v;
}

/* readOutput(h, Float32Array dst) */
static napi_value js_read_output(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    CALL(env, h, read_output, (float *)p, n / 4);
    return argv[1];
}

static napi_value js_write_output(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    CALL(env, h, write_output, (const float *)p, n / 4);
    return NULL;
}

/* get_handle for the reprojection calls, which take one device's handle: ptmi_multi has no counterpart (include/ptmi.h) */
static handle *get_single_handle(napi_env env, napi_callback_info info, size_t want, napi_value *argv, const char *what) {
    handle *h = get_handle(env, info, want, argv);
    if (h && h->kind == KIND_MULTI) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s: reprojection is not supported with several devices", what);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    return h;
}

/* setAovs(h, mask): PTMI_AOV_* bits */
static napi_value js_set_aovs(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    uint32_t mask = 0;
    napi_get_value_uint32(env, argv[1], &mask);
    CALL(env, h, set_aovs, mask);
    return NULL;
}

/* readAov(h, which, dst typed array of width*height*16 (or *8 for PTMI_AOV_ID) bytes) */
static napi_value js_read_aov(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_handle(env, info, 3, argv);
    if (!h) return NULL;
    uint32_t which = 0;
    napi_get_value_uint32(env, argv[1], &which);
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    CALL(env, h, read_aov, which, p, n);
    return argv[2];
}

/* blit(h, Uint8Array dstRgba8) — the reference's blit pass (blit.wgsl) into an 8-bit canvas, row 0 = top */
static napi_value js_blit(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!p) { napi_throw_type_error(env, NULL, "expected a Uint8Array of width*height*4 bytes"); return NULL; }
    /* the library writes width*height*4 bytes: a short (or stale, after resize()) array must not reach it. Several devices
     * blit on the first, whose size is the frame's. */
    uint32_t w = 0, hh = 0;
    int rc = ptmi_get_size(h->kind == KIND_MULTI ? ptmi_multi_context(h->m, 0) : h->ctx, &w, &hh);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_get_size");
    if (n != (size_t)w * hh * 4) {
        char msg[128];
        snprintf(msg, sizeof msg, "blit: expected a Uint8Array of %zu bytes (%ux%ux4), got %zu", (size_t)w * hh * 4, w, hh, n);
        napi_throw_range_error(env, NULL, msg);
        return NULL;
    }
    CALL(env, h, blit, NULL, 0, (uint8_t *)p, n);
    return argv[1];
}

/* the canvas-sized typed array a call writes: width*height*4 elements of elem_bytes each, else a RangeError (a short or stale
 * array, after resize(), must not reach the library) */
static int check_canvas(napi_env env, handle *h, const char *what, const char *type, size_t elem_bytes, void *p, size_t n) {
    if (!p) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s: expected a %s of width*height*4 elements", what, type);
        napi_throw_type_error(env, NULL, msg);
        return 0;
    }
    uint32_t w = 0, hh = 0;
    int rc = ptmi_get_size(h->kind == KIND_MULTI ? ptmi_multi_context(h->m, 0) : h->ctx, &w, &hh);     /* several devices: the first's size is the frame's */
    if (rc) { throw_ptmi(env, h, rc, "ptmi_get_size"); return 0; }
    if (n != (size_t)w * hh * 4 * elem_bytes) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: expected a %s of %zu bytes (%ux%ux4), got %zu", what, type, (size_t)w * hh * 4 * elem_bytes, w,
                 hh, n);
        napi_throw_range_error(env, NULL, msg);
        return 0;
    }
    return 1;
}

static float get_f32_prop(napi_env env, napi_value obj, const char *name, float dflt) {
    napi_value v; bool has = false; double out = dflt;
    if (napi_has_named_property(env, obj, name, &has) == napi_ok && has &&
        napi_get_named_property(env, obj, name, &v) == napi_ok)
        napi_get_value_double(env, v, &out);
    return (float)out;
}

/* setMoments(h, on) */
static napi_value js_set_moments(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    bool on = false;
    napi_get_value_bool(env, argv[1], &on);
    CALL(env, h, set_moments, on ? 1u : 0u);
    return NULL;
}

/* getMoments(h) -> boolean */
static napi_value js_get_moments(napi_env env, napi_callback_info info) {
    napi_value argv[1], out;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    uint32_t on = 0;
    CALL(env, h, get_moments, &on);
    napi_get_boolean(env, on != 0, &out);
    return out;
}

/* setProjections(h, on): ptmi_set_projections / ptmi_multi_set_projections. While on, bytes 88..95 of every camera blob are read */
static napi_value js_set_projections(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    bool on = false;
    napi_get_value_bool(env, argv[1], &on);
    CALL(env, h, set_projections, on ? 1u : 0u);
    return NULL;
}

/* getProjections(h) -> boolean */
static napi_value js_get_projections(napi_env env, napi_callback_info info) {
    napi_value argv[1], out;
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    uint32_t on = 0;
    CALL(env, h, get_projections, &on);
    napi_get_boolean(env, on != 0, &out);
    return out;
}

/* denoise(h, {iterations, demodulate, phiColor, phiNormal, phiDepth} or null, Float32Array dst of width*height*4) */
static napi_value js_denoise(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_handle(env, info, 3, argv);
    if (!h) return NULL;
    ptmi_denoise_params prm;
    memset(&prm, 0, sizeof prm);
    napi_valuetype t;
    if (napi_typeof(env, argv[1], &t) == napi_ok && t == napi_object) {
        prm.iterations = get_u32_prop(env, argv[1], "iterations", 0);
        prm.demodulate = get_u32_prop(env, argv[1], "demodulate", 0);
        prm.phi_color = get_f32_prop(env, argv[1], "phiColor", 0.0f);
        prm.phi_normal = get_f32_prop(env, argv[1], "phiNormal", 0.0f);
        prm.phi_depth = get_f32_prop(env, argv[1], "phiDepth", 0.0f);
    }
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    if (!check_canvas(env, h, "denoise", "Float32Array", 4, p, n)) return NULL;
    CALL(env, h, denoise, &prm, (float *)p, n / 4);
    return argv[2];
}

static void set_num(napi_env env, napi_value obj, const char *k, double v);

/* dispatchAdaptive(h, cameraBytes, {threshold, floor, minFrames, maxFrames, step, neighbourhood}, rounds): ptmi_dispatch_adaptive */
static napi_value js_dispatch_adaptive(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_handle(env, info, 4, argv);
    if (!h) return NULL;
    void *p; size_t n; uint32_t rounds = 1;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!p || n != sizeof(ptmi_camera)) { napi_throw_range_error(env, NULL, "camera blob must be 96 bytes"); return NULL; }
    ptmi_adaptive_params prm;
    memset(&prm, 0, sizeof prm);
    napi_valuetype t;
    if (napi_typeof(env, argv[2], &t) == napi_ok && t == napi_object) {
        prm.threshold = get_f32_prop(env, argv[2], "threshold", 0.0f);
        prm.floor = get_f32_prop(env, argv[2], "floor", 0.0f);
        prm.min_frames = get_u32_prop(env, argv[2], "minFrames", 0);
        prm.max_frames = get_u32_prop(env, argv[2], "maxFrames", 0);
        prm.step = get_u32_prop(env, argv[2], "step", 0);
        prm.neighbourhood = get_u32_prop(env, argv[2], "neighbourhood", 0);
    }
    napi_get_value_uint32(env, argv[3], &rounds);
    ptmi_camera cam;
    memcpy(&cam, p, sizeof cam);
    CALL(env, h, dispatch_adaptive, &cam, &prm, rounds);
    return NULL;
}

/* adaptiveStatus(h) -> {active, samples, minCount, maxCount, rounds}; synchronises */
static napi_value js_adaptive_status(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    struct ptmi_adaptive_status s;
    CALL(env, h, adaptive_status, &s);
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "active", (double)s.active); set_num(env, o, "samples", (double)s.samples);
    set_num(env, o, "minCount", (double)s.min_count); set_num(env, o, "maxCount", (double)s.max_count);
    set_num(env, o, "rounds", (double)s.rounds);
    return o;
}

/* reproject(h, fromCameraBytes, toCameraBytes, {maxHistory, depthTolerance, matchIds} or null): ptmi_reproject */
static napi_value js_reproject(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_single_handle(env, info, 4, argv, "reproject");
    if (!h) return NULL;
    ptmi_camera cams[2];
    for (int k = 0; k < 2; k++) {
        void *p; size_t n;
        if (!get_bytes(env, argv[1 + k], &p, &n)) return NULL;
        if (!p || n != sizeof(ptmi_camera)) { napi_throw_range_error(env, NULL, "camera blob must be 96 bytes"); return NULL; }
        memcpy(&cams[k], p, sizeof cams[k]);
    }
    ptmi_reproject_params prm;
    memset(&prm, 0, sizeof prm);
    napi_valuetype t;
    if (napi_typeof(env, argv[3], &t) == napi_ok && t == napi_object) {
        prm.max_history = get_u32_prop(env, argv[3], "maxHistory", 0);
        prm.depth_tolerance = get_f32_prop(env, argv[3], "depthTolerance", 0.0f);
        prm.match_ids = get_u32_prop(env, argv[3], "matchIds", 0);
    }
    int rc = ptmi_reproject(h->ctx, &cams[0], &cams[1], &prm);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_reproject");
    return NULL;
}

/* reprojectStatus(h) -> {carried, disoccluded, missed, samples} of the last reproject(); synchronises */
static napi_value js_reproject_status(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "reprojectStatus");
    if (!h) return NULL;
    struct ptmi_reproject_status s;
    int rc = ptmi_reproject_status(h->ctx, &s);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_reproject_status");
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "carried", (double)s.carried); set_num(env, o, "disoccluded", (double)s.disoccluded);
    set_num(env, o, "missed", (double)s.missed); set_num(env, o, "samples", (double)s.samples);
    return o;
}

/* setMotion(h, on): ptmi_set_motion. Like reprojection, one device's handle only */
static napi_value js_set_motion(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "setMotion");
    if (!h) return NULL;
    bool on = false;
    napi_get_value_bool(env, argv[1], &on);
    int rc = ptmi_set_motion(h->ctx, on ? 1u : 0u);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_set_motion");
    return NULL;
}

/* motionCommit(h): ptmi_motion_commit */
static napi_value js_motion_commit(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "motionCommit");
    if (!h) return NULL;
    int rc = ptmi_motion_commit(h->ctx);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_motion_commit");
    return NULL;
}

/* motionStatus(h) -> {on, epochs, dirtyFirst, dirtyCount, moved, movedCarried}; synchronises */
static napi_value js_motion_status(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "motionStatus");
    if (!h) return NULL;
    struct ptmi_motion_status s;
    int rc = ptmi_motion_status(h->ctx, &s);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_motion_status");
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "on", (double)s.on); set_num(env, o, "epochs", (double)s.epochs);
    set_num(env, o, "dirtyFirst", (double)s.dirty_first); set_num(env, o, "dirtyCount", (double)s.dirty_count);
    set_num(env, o, "moved", (double)s.moved); set_num(env, o, "movedCarried", (double)s.moved_carried);
    return o;
}

/* readMotion(h, Float32Array dst of width*height*4): the motion plane */
static napi_value js_read_motion(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "readMotion");
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!check_canvas(env, h, "readMotion", "Float32Array", 4, p, n)) return NULL;
    int rc = ptmi_read_motion(h->ctx, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_read_motion");
    return argv[1];
}

/* debugMotionPrev(h, first, count, Float32Array dst of count*9): the previous positions of triangles [first, first + count) */
static napi_value js_debug_motion_prev(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_single_handle(env, info, 4, argv, "debugMotionPrev");
    if (!h) return NULL;
    uint32_t first = 0, count = 0;
    napi_get_value_uint32(env, argv[1], &first);
    napi_get_value_uint32(env, argv[2], &count);
    void *p; size_t n;
    if (!get_bytes(env, argv[3], &p, &n)) return NULL;
    if (n != (size_t)count * 9 * sizeof(float)) { napi_throw_range_error(env, NULL, "debugMotionPrev: expected count * 9 floats"); return NULL; }
    int rc = ptmi_debug_motion_prev(h->ctx, first, count, (float *)p);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_debug_motion_prev");
    return argv[3];
}

/* ---- lightmap baking (include/ptmi.h ptmi_upload_bake_surface ...): one device's handle only, like reprojection ---- */

/* {firstFrame, bias} or null -> ptmi_bake_params; absent members take the C defaults */
static void get_bake_params(napi_env env, napi_value v, ptmi_bake_params *prm) {
    napi_valuetype t;
    memset(prm, 0, sizeof *prm);
    prm->bias = 1e-6f;
    if (napi_typeof(env, v, &t) == napi_ok && t == napi_object) {
        prm->first_frame = get_u32_prop(env, v, "firstFrame", 0);
        prm->bias = get_f32_prop(env, v, "bias", 1e-6f);
    }
}

/* uploadBakeSurface(h, texels (32-byte records) or null, width, height) */
static napi_value js_upload_bake_surface(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    handle *h = get_single_handle(env, info, 4, argv, "uploadBakeSurface");
    if (!h) return NULL;
    void *p; size_t n; uint32_t w = 0, hh = 0;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &w); napi_get_value_uint32(env, argv[3], &hh);
    if (p && n != (size_t)w * hh * sizeof(ptmi_bake_texel)) {
        napi_throw_range_error(env, NULL, "uploadBakeSurface: expected width * height records of 32 bytes"); return NULL;
    }
    int rc = ptmi_upload_bake_surface(h->ctx, (const ptmi_bake_texel *)p, w, hh);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_upload_bake_surface");
    return NULL;
}

/* dispatchBake(h, {firstFrame, bias} or null, frames): ptmi_dispatch_bake */
static napi_value js_dispatch_bake(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "dispatchBake");
    if (!h) return NULL;
    ptmi_bake_params prm;
    uint32_t frames = 1;
    get_bake_params(env, argv[1], &prm);
    napi_get_value_uint32(env, argv[2], &frames);
    int rc = ptmi_dispatch_bake(h->ctx, &prm, frames);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_dispatch_bake");
    return NULL;
}

/* bakeStatus(h) -> {present, width, height, covered} */
static napi_value js_bake_status(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "bakeStatus");
    if (!h) return NULL;
    struct ptmi_bake_status s;
    int rc = ptmi_bake_status(h->ctx, &s);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_bake_status");
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "present", (double)s.present); set_num(env, o, "width", (double)s.width);
    set_num(env, o, "height", (double)s.height); set_num(env, o, "covered", (double)s.covered);
    return o;
}

/* bakeDilate(h, passes, Float32Array dst of width*height*4): the gutter-filled copy of the output buffer, w = the state */
static napi_value js_bake_dilate(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "bakeDilate");
    if (!h) return NULL;
    uint32_t passes = 0;
    napi_get_value_uint32(env, argv[1], &passes);
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    if (!check_canvas(env, h, "bakeDilate", "Float32Array", 4, p, n)) return NULL;
    int rc = ptmi_bake_dilate(h->ctx, passes, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_bake_dilate");
    return argv[2];
}

/* bakeDenoise(h, {iterations, dilate, phiColor, phiNormal, phiPosition} or null, Float32Array dst of width*height*4): the filtered
 * lightmap (ptmi_bake_denoise), w = the state; absent members take the C defaults */
static napi_value js_bake_denoise(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "bakeDenoise");
    if (!h) return NULL;
    ptmi_bake_denoise_params prm;
    memset(&prm, 0, sizeof prm);
    napi_valuetype t;
    if (napi_typeof(env, argv[1], &t) == napi_ok && t == napi_object) {
        prm.iterations = get_u32_prop(env, argv[1], "iterations", 0);
        prm.dilate = get_u32_prop(env, argv[1], "dilate", 0);
        prm.phi_color = get_f32_prop(env, argv[1], "phiColor", 0.0f);
        prm.phi_normal = get_f32_prop(env, argv[1], "phiNormal", 0.0f);
        prm.phi_position = get_f32_prop(env, argv[1], "phiPosition", 0.0f);
    }
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    if (!check_canvas(env, h, "bakeDenoise", "Float32Array", 4, p, n)) return NULL;
    int rc = ptmi_bake_denoise(h->ctx, &prm, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_bake_denoise");
    return argv[2];
}

/* writeMoments(h, Float32Array src of width*height*4): ptmi_write_moments */
static napi_value js_write_moments(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "writeMoments");
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!check_canvas(env, h, "writeMoments", "Float32Array", 4, p, n)) return NULL;
    int rc = ptmi_write_moments(h->ctx, (const float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_write_moments");
    return NULL;
}

/* ---- light probes (include/ptmi.h ptmi_upload_probes ...): one device's handle only, like baking ---- */

/* uploadProbes(h, records (16 bytes each) or null, tile) */
static napi_value js_upload_probes(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "uploadProbes");
    if (!h) return NULL;
    void *p; size_t n; uint32_t tile = 0;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    napi_get_value_uint32(env, argv[2], &tile);
    if (p && (n % sizeof(ptmi_probe) || n / sizeof(ptmi_probe) > 0xFFFFFFFFu)) {
        napi_throw_range_error(env, NULL, "uploadProbes: expected records of 16 bytes"); return NULL;
    }
    int rc = ptmi_upload_probes(h->ctx, (const ptmi_probe *)p, p ? (uint32_t)(n / sizeof(ptmi_probe)) : 0u, tile);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_upload_probes");
    return NULL;
}

/* dispatchProbes(h, {firstFrame} or null, frames): ptmi_dispatch_probes */
static napi_value js_dispatch_probes(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "dispatchProbes");
    if (!h) return NULL;
    ptmi_probe_params prm;
    napi_valuetype t;
    uint32_t frames = 1;
    memset(&prm, 0, sizeof prm);
    if (napi_typeof(env, argv[1], &t) == napi_ok && t == napi_object) prm.first_frame = get_u32_prop(env, argv[1], "firstFrame", 0);
    napi_get_value_uint32(env, argv[2], &frames);
    int rc = ptmi_dispatch_probes(h->ctx, &prm, frames);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_dispatch_probes");
    return NULL;
}

/* probeStatus(h) -> {present, tile, count, enabled, texels} */
static napi_value js_probe_status(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "probeStatus");
    if (!h) return NULL;
    struct ptmi_probe_status s;
    int rc = ptmi_probe_status(h->ctx, &s);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_probe_status");
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "present", (double)s.present); set_num(env, o, "tile", (double)s.tile); set_num(env, o, "count", (double)s.count);
    set_num(env, o, "enabled", (double)s.enabled); set_num(env, o, "texels", (double)s.texels);
    return o;
}

/* probeSh(h, Float32Array dst of count * 27): SH9 of every probe's tile */
static napi_value js_probe_sh(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "probeSh");
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    int rc = ptmi_probe_sh(h->ctx, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_probe_sh");
    return argv[1];
}

/* probeIrradiance(h, m, Float32Array dst of count * m * m * 4): the m x m irradiance tile (E / pi) of every probe */
static napi_value js_probe_irradiance(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "probeIrradiance");
    if (!h) return NULL;
    uint32_t m = 0;
    napi_get_value_uint32(env, argv[1], &m);
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    int rc = ptmi_probe_irradiance(h->ctx, m, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_probe_irradiance");
    return argv[2];
}

/* ---- probe visibility (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility) ---- */

/* setProbeDepth(h, maxDistance or null): the depth plane on with this clamp, or off */
static napi_value js_set_probe_depth(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "setProbeDepth");
    if (!h) return NULL;
    ptmi_probe_depth_params prm;
    napi_valuetype t;
    double d = 0.0;
    memset(&prm, 0, sizeof prm);
    const int on = napi_typeof(env, argv[1], &t) == napi_ok && t == napi_number && napi_get_value_double(env, argv[1], &d) == napi_ok;
    prm.max_distance = (float)d;
    int rc = ptmi_set_probe_depth(h->ctx, on ? &prm : NULL);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_set_probe_depth");
    return NULL;
}

/* getProbeDepth(h) -> maxDistance while the plane is on, else null */
static napi_value js_get_probe_depth(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_single_handle(env, info, 1, argv, "getProbeDepth");
    if (!h) return NULL;
    uint32_t on = 0;
    ptmi_probe_depth_params prm;
    int rc = ptmi_get_probe_depth(h->ctx, &on, &prm);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_get_probe_depth");
    napi_value v;
    if (on) NAPI_OK(env, napi_create_double(env, (double)prm.max_distance, &v));
    else NAPI_OK(env, napi_get_null(env, &v));
    return v;
}

/* readProbeDepth(h, Float32Array dst of width*height*4): the depth plane */
static napi_value js_read_probe_depth(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "readProbeDepth");
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    int rc = ptmi_read_probe_depth(h->ctx, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_read_probe_depth");
    return argv[1];
}

/* writeProbeDepth(h, Float32Array src of width*height*4): restores a cached plane */
static napi_value js_write_probe_depth(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_single_handle(env, info, 2, argv, "writeProbeDepth");
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    int rc = ptmi_write_probe_depth(h->ctx, (const float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_write_probe_depth");
    return NULL;
}

/* probeVisibility(h, {m, sharpness, border}, Float32Array dst of count * side * side * 4), side = m + 2 * border */
static napi_value js_probe_visibility(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    handle *h = get_single_handle(env, info, 3, argv, "probeVisibility");
    if (!h) return NULL;
    ptmi_probe_visibility_params prm;
    napi_valuetype t;
    memset(&prm, 0, sizeof prm);
    if (napi_typeof(env, argv[1], &t) == napi_ok && t == napi_object) {
        prm.m = get_u32_prop(env, argv[1], "m", 0);
        prm.sharpness_log2 = get_u32_prop(env, argv[1], "sharpness", 6);
        prm.border = get_u32_prop(env, argv[1], "border", 0);
    }
    void *p; size_t n;
    if (!get_bytes(env, argv[2], &p, &n)) return NULL;
    int rc = ptmi_probe_visibility(h->ctx, &prm, (float *)p, n / 4);
    if (rc) return throw_ptmi(env, h, rc, "ptmi_probe_visibility");
    return argv[2];
}

/* readMoments(h, Float32Array dst of width*height*4): the sample-moments plane */
static napi_value js_read_moments(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!check_canvas(env, h, "readMoments", "Float32Array", 4, p, n)) return NULL;
    CALL(env, h, read_moments, (float *)p, n / 4);
    return argv[1];
}

/* blitDenoised(h, Uint8Array dstRgba8): blit() of the last denoise() result */
static napi_value js_blit_denoised(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    handle *h = get_handle(env, info, 2, argv);
    if (!h) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[1], &p, &n)) return NULL;
    if (!check_canvas(env, h, "blitDenoised", "Uint8Array", 1, p, n)) return NULL;
    CALL(env, h, blit_denoised, NULL, 0, (uint8_t *)p, n);
    return argv[1];
}

static void set_num(napi_env env, napi_value obj, const char *k, double v) {
    napi_value n;
    if (napi_create_double(env, v, &n) == napi_ok) napi_set_named_property(env, obj, k, n);
}

/* getStats(h); several devices add gatherMs (once a gather has been timed) and devices */
static napi_value js_get_stats(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    ptmi_stats s;
    CALL(env, h, get_stats, &s);
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    set_num(env, o, "paths", (double)s.paths); set_num(env, o, "segments", (double)s.segments);
    set_num(env, o, "shadowRays", (double)s.shadow_rays); set_num(env, o, "frames", (double)s.frames);
    set_num(env, o, "dispatches", (double)s.dispatches); set_num(env, o, "gpuMs", s.gpu_ms);
    set_num(env, o, "extendMs", s.extend_ms); set_num(env, o, "shadeMs", s.shade_ms); set_num(env, o, "shadowMs", s.shadow_ms);
    set_num(env, o, "shadowTraced", (double)s.shadow_traced); set_num(env, o, "uploadMs", s.upload_ms);
    set_num(env, o, "bvhDepth", s.bvh_depth); set_num(env, o, "traversalUsed", s.traversal_used);
    set_num(env, o, "framesPerBatchUsed", s.frames_per_batch_used);
    set_num(env, o, "leavesUsed", s.leaves_used); set_num(env, o, "leafTrisUsed", s.leaf_tris_used);
    set_num(env, o, "extendVariant", s.extend_variant); set_num(env, o, "shadowVariant", s.shadow_variant);
    set_num(env, o, "verifyFailed", (double)s.verify_failed); set_num(env, o, "treeBuilderUsed", s.tree_builder_used);
    if (h->kind == KIND_MULTI) {
        double ms = -1.0;
        if (ptmi_multi_gather_ms(h->m, &ms) == 0) set_num(env, o, "gatherMs", ms);
        set_num(env, o, "devices", ptmi_multi_count(h->m));
    }
    return o;
}

/* resetStats(h): the status is not reported */
static napi_value js_reset_stats(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    handle *h = get_handle(env, info, 1, argv);
    if (!h) return NULL;
    (void)RUN(h, reset_stats);
    return NULL;
}

/* ---- host-side scene preparation (include/ptmi_scene.h, libptmi_scene.so; no GPU involved) ---- */

/* buildBvh(trianglesArrayBuffer) -> { nodes: ArrayBuffer (48-B nodes), depth }; sorts the triangles in place
 * exactly like src/renderer/bvh.ts does */
static napi_value js_build_bvh(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    void *p; size_t n;
    if (!get_bytes(env, argv[0], &p, &n)) return NULL;
    if (!p || n % sizeof(ptmi_triangle)) { napi_throw_range_error(env, NULL, "expected a triangle blob (128-byte elements)"); return NULL; }
    uint32_t nt = (uint32_t)(n / sizeof(ptmi_triangle));
    uint32_t cap = ptmi_scene_bvh_node_bound(nt), count = 0, depth = 0;
    void *nodes = NULL;
    napi_value ab;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)cap * sizeof(ptmi_bvh_node), &nodes, &ab));
    int rc = ptmi_scene_build_bvh((ptmi_triangle *)p, nt, 4, 12, (ptmi_bvh_node *)nodes, cap, &count, &depth);
    if (rc) { napi_throw_error(env, "PTMI_SCENE", ptmi_scene_last_error()); return NULL; }
    /* hand back exactly `count` nodes */
    void *out = NULL;
    napi_value ab2, obj, d;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)count * sizeof(ptmi_bvh_node), &out, &ab2));
    memcpy(out, nodes, (size_t)count * sizeof(ptmi_bvh_node));
    NAPI_OK(env, napi_create_object(env, &obj));
    NAPI_OK(env, napi_create_uint32(env, depth, &d));
    napi_set_named_property(env, obj, "nodes", ab2);
    napi_set_named_property(env, obj, "depth", d);
    return obj;
}

/* emissiveLights(triangles, materials, punctualLights) -> ArrayBuffer of 48-B lights: the punctual ones first,
 * then one per emissive triangle in post-sort order (src/renderer/gpu.ts:121-138) */
static napi_value js_emissive_lights(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    void *pt, *pm, *pl; size_t nt, nm, nl;
    if (!get_bytes(env, argv[0], &pt, &nt) || !get_bytes(env, argv[1], &pm, &nm) || !get_bytes(env, argv[2], &pl, &nl)) return NULL;
    if (nt % sizeof(ptmi_triangle) || nm % sizeof(ptmi_material) || nl % sizeof(ptmi_light)) {
        napi_throw_range_error(env, NULL, "blob length is not a multiple of its element size"); return NULL;
    }
    uint32_t ntri = (uint32_t)(nt / sizeof(ptmi_triangle)), n0 = (uint32_t)(nl / sizeof(ptmi_light)), count = n0;
    uint32_t cap = n0 + ntri;
    void *tmp = NULL;
    napi_value ab;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)(cap ? cap : 1) * sizeof(ptmi_light), &tmp, &ab));
    if (n0) memcpy(tmp, pl, nl);
    if (ntri) {
        int rc = ptmi_scene_emissive_lights((const ptmi_triangle *)pt, ntri, (const ptmi_material *)pm,
                                            (uint32_t)(nm / sizeof(ptmi_material)), (ptmi_light *)tmp, cap, &count);
        if (rc) { napi_throw_error(env, "PTMI_SCENE", ptmi_scene_last_error()); return NULL; }
    }
    void *out = NULL;
    napi_value ab2;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)count * sizeof(ptmi_light), &out, &ab2));
    if (count) memcpy(out, tmp, (size_t)count * sizeof(ptmi_light));
    return ab2;
}

static napi_value js_abi_version(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, ptmi_abi_version(), &v));
    return v;
}

static napi_value init(napi_env env, napi_value exports) {
    static const struct { const char *name; napi_callback fn; } fns[] = {
        {"abiVersion", js_abi_version}, {"create", js_create}, {"multiCreate", js_multi_create}, {"destroy", js_destroy},
        {"uploadScene", js_upload_scene}, {"uploadAtlas", js_upload_atlas}, {"uploadEnvironment", js_upload_environment}, {"setMedium", js_set_medium}, {"uploadMediumDensity", js_upload_medium_density},
        {"updateTriangles", js_update_triangles}, {"updateMaterials", js_update_materials}, {"updateLights", js_update_lights}, {"sceneUpdateStatus", js_scene_update_status},
        {"setTriangleGroups", js_set_triangle_groups}, {"transformGroups", js_transform_groups}, {"transformStatus", js_transform_status},
        {"normalMatrix", js_normal_matrix},
        {"setSkin", js_set_skin}, {"poseSkin", js_pose_skin}, {"skinStatus", js_skin_status},
        {"setMorph", js_set_morph}, {"poseMorph", js_pose_morph}, {"morphStatus", js_morph_status},
        {"rebuildTree", js_rebuild_tree}, {"rebuildStatus", js_rebuild_status},
        {"setAlphaCutoff", js_set_alpha_cutoff}, {"alphaStatus", js_alpha_status},
        {"setAlphaBlend", js_set_alpha_blend}, {"alphaBlendStatus", js_alpha_blend_status},
        {"resize", js_resize}, {"setOptions", js_set_options},
        {"dispatch", js_dispatch}, {"gather", js_gather}, {"gatherPlanes", js_gather_planes}, {"synchronize", js_synchronize}, {"throttle", js_throttle},
        {"readOutput", js_read_output}, {"writeOutput", js_write_output}, {"setAovs", js_set_aovs}, {"readAov", js_read_aov},
        {"blit", js_blit}, {"getStats", js_get_stats}, {"resetStats", js_reset_stats},
        {"setMoments", js_set_moments}, {"denoise", js_denoise}, {"blitDenoised", js_blit_denoised},
        {"dispatchAdaptive", js_dispatch_adaptive}, {"adaptiveStatus", js_adaptive_status}, {"readMoments", js_read_moments},
        {"reproject", js_reproject}, {"reprojectStatus", js_reproject_status},
        {"setMotion", js_set_motion}, {"motionCommit", js_motion_commit}, {"motionStatus", js_motion_status}, {"readMotion", js_read_motion},
        {"debugMotionPrev", js_debug_motion_prev},
        {"setProjections", js_set_projections}, {"getProjections", js_get_projections},
        {"uploadBakeSurface", js_upload_bake_surface}, {"dispatchBake", js_dispatch_bake}, {"bakeStatus", js_bake_status},
        {"bakeDilate", js_bake_dilate}, {"bakeDenoise", js_bake_denoise}, {"getMoments", js_get_moments}, {"writeMoments", js_write_moments},
        {"uploadProbes", js_upload_probes}, {"dispatchProbes", js_dispatch_probes}, {"probeStatus", js_probe_status},
        {"probeSh", js_probe_sh}, {"probeIrradiance", js_probe_irradiance},
        {"setProbeDepth", js_set_probe_depth}, {"getProbeDepth", js_get_probe_depth}, {"readProbeDepth", js_read_probe_depth},
        {"writeProbeDepth", js_write_probe_depth}, {"probeVisibility", js_probe_visibility},
        {"buildBvh", js_build_bvh}, {"emissiveLights", js_emissive_lights},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
            napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
            napi_throw_error(env, NULL, "cannot register addon functions");
            return NULL;
        }
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
