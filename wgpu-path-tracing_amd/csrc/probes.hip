// probes.hip — light probes (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance,
// ptmi_probe_visibility): the probe records, the texel list of the enabled probes' tiles and the two float64 tables
// of a tile size, the checks of a probe dispatch, the debug rays, and the reductions that turn a probe's tiles into what an engine
// reads: SH9 from the radiance tile, and irradiance from it and visibility from the depth tile by one tile gather over a lobe policy
// (k_probe_gather, gather_tiles). The debug rays are debug_stages.hip's listed-rays routine. The probe's ray generation is with the other ray
// sources (pipeline.hip ProbeRays); its pixels are BakedPixels, its folds pipeline.hip's (fold_probe_depth among them) and its bounce
// loop the plain dispatch's (dispatch.hip); the depth plane's switch is with the other planes' (ptmi_api.hip).
// No counterpart in the reference, which renders from a camera only.
#include "ptmi_ctx.h"
#include "pt_math.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

namespace {

constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr float INV_PI = 0.318309886f;

// for s = 32, 16, ..., 1: v[l] = v[l] + v[l + s]; lane 0 ends with the sum of the wave (a lane whose partner is past the wave adds
// its own value, which no lower lane ever reads)
template <int K>
PT_DEV void butterfly(float (&v)[K]) {
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int k = 0; k < K; k++) v[k] = __fadd_rn(v[k], __shfl_down(v[k], s));
    }
}

// SH9 of every probe's tile: one wave per probe, WAVES probes per workgroup, no LDS (a texel and its nine basis values are read once).
// Lane l takes texels l, l + 64, ...: 64 consecutive float4 of at most 64 / N tile rows, whole 16-byte reads.
__global__ __launch_bounds__(BLOCK) void k_probe_sh(DevProbeAtlas a, const float *__restrict__ basis, float *__restrict__ sh) {
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= a.count) return;                                       // (the whole wave)
    float acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0f;
    if (__float_as_uint(a.probes[i].w) != 0u) {
        const uint32_t N = 1u << a.shift, NN = N << a.shift;
        const float4 *const tile = a.out + (size_t)((i / a.cols) << a.shift) * a.W + ((i % a.cols) << a.shift);
        for (uint32_t t = lane; t < NN; t += 64u) {
            const float4 L = tile[(size_t)(t >> a.shift) * a.W + (t & (N - 1u))];
            const float *const bt = basis + (size_t)t * 9u;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const float bk = bt[k];
                acc[3 * k] = __fadd_rn(acc[3 * k], __fmul_rn(bk, L.x));
                acc[3 * k + 1] = __fadd_rn(acc[3 * k + 1], __fmul_rn(bk, L.y));
                acc[3 * k + 2] = __fadd_rn(acc[3 * k + 2], __fmul_rn(bk, L.z));
            }
        }
    }
    butterfly(acc);
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 27; k++) sh[(size_t)i * 27u + k] = acc[k];
    }
}

// The tile gather of ptmi_probe_irradiance and ptmi_probe_visibility: one workgroup per probe. Every one of the m * m output texels
// sums over all N * N texels of the probe's tile, so the tile (as three planes, 12 B a texel) and the (d, dw) table (16 B) are staged
// once in dynamic LDS: 28 B a texel, 112 KB at N = 64, which leaves one workgroup per CU there and five at N = 32. A wave takes output
// texels wave, wave + WAVES, ...; its lanes split t as k_probe_sh's do, so consecutive lanes read consecutive LDS words (no bank
// conflict) and one b128 each of the table. A disabled probe's tile is zeros. The lobe policy says the rest:
//   SUMS          3: the three channels; 4: the weights too
//   side(m)       the output tile's side
//   shape(c)      the lobe's value from the clamped cosine c
//   store(...)    lane 0's finish of output texel j from the wave's sums
template <class Lobe>
__global__ __launch_bounds__(BLOCK) void k_probe_gather(DevProbeAtlas a, const float4 *__restrict__ dir_dw,
                                                        const float4 *__restrict__ normals, uint32_t m, const Lobe lobe,
                                                        float4 *__restrict__ out) {
    extern __shared__ float4 lds[];
    const uint32_t i = blockIdx.x, N = 1u << a.shift, NN = N << a.shift, mm = m * m, out_texels = lobe.side(m) * lobe.side(m);
    float4 *const dst = out + (size_t)i * out_texels;
    if (__float_as_uint(a.probes[i].w) == 0u) {                     // (the whole workgroup)
        for (uint32_t j = threadIdx.x; j < out_texels; j += BLOCK) dst[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float4 *const tab = lds;
    float *const c0 = reinterpret_cast<float *>(lds + NN), *const c1 = c0 + NN, *const c2 = c1 + NN;
    const float4 *const tile = a.out + (size_t)((i / a.cols) << a.shift) * a.W + ((i % a.cols) << a.shift);
    for (uint32_t t = threadIdx.x; t < NN; t += BLOCK) {
        const float4 L = tile[(size_t)(t >> a.shift) * a.W + (t & (N - 1u))];
        tab[t] = dir_dw[t]; c0[t] = L.x; c1[t] = L.y; c2[t] = L.z;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t j = threadIdx.x >> 6; j < mm; j += WAVES) {
        const v3 n = xyz(normals[j]);
        float acc[Lobe::SUMS] = {};
        for (uint32_t t = lane; t < NN; t += 64u) {
            const float4 d = tab[t];
            float c = dot3(n, xyz(d));
            c = c > 0.0f ? c : 0.0f;
            const float wgt = __fmul_rn(lobe.shape(c), d.w);
            acc[0] = __fadd_rn(acc[0], __fmul_rn(wgt, c0[t]));
            acc[1] = __fadd_rn(acc[1], __fmul_rn(wgt, c1[t]));
            acc[2] = __fadd_rn(acc[2], __fmul_rn(wgt, c2[t]));
            if constexpr (Lobe::SUMS == 4) acc[3] = __fadd_rn(acc[3], wgt);
        }
        butterfly(acc);
        if (lane == 0u) lobe.store(dst, m, j, acc);
    }
}

// Irradiance (what the documents call k_probe_irradiance): the clamped cosine over the radiance tile, times 1 / pi.
struct IrradianceLobe {
    static constexpr int SUMS = 3;
    PT_HD uint32_t side(uint32_t m) const { return m; }
    PT_DEV float shape(float c) const { return c; }
    PT_DEV void store(float4 *dst, uint32_t, uint32_t j, const float (&acc)[3]) const {
        dst[j] = make_float4(__fmul_rn(acc[0], INV_PI), __fmul_rn(acc[1], INV_PI), __fmul_rn(acc[2], INV_PI), 1.0f);
    }
};

// Visibility (include/ptmi.h ptmi_probe_visibility; what the documents call k_probe_visibility): over the probe's tile of the depth
// plane, a power-cosine lobe of `sharp` squarings of the clamped cosine, divided by the sum of the weights. With border = 1 the lane
// that writes an interior texel of the tile's rim writes the ring texels that copy it as well (up to three): every ring texel has one
// source, so nothing is read back and nothing is written twice.
struct VisibilityLobe {
    uint32_t sharp, border;
    static constexpr int SUMS = 4;
    PT_HD uint32_t side(uint32_t m) const { return m + 2u * border; }
    PT_DEV float shape(float p) const {
        for (uint32_t k = 0; k < sharp; k++) p = __fmul_rn(p, p);
        return p;
    }
    PT_DEV void store(float4 *dst, uint32_t m, uint32_t j, const float (&acc)[4]) const {
        const float4 v = make_float4(__fdiv_rn(acc[0], acc[3]), __fdiv_rn(acc[1], acc[3]), __fdiv_rn(acc[2], acc[3]), 1.0f);
        const uint32_t x = j % m, y = j / m, e = m - 1u, side = m + 2u * border;
        dst[(size_t)(y + border) * side + (x + border)] = v;
        if (border == 0u) return;
        // the ring texels that copy this one under the octahedral wrap (include/ptmi.h has the table), bordered coordinates
        if (x == 0u) dst[(size_t)(e - y + 1u) * side] = v;                          // (-1, e - y)
        if (x == e) dst[(size_t)(e - y + 1u) * side + (m + 1u)] = v;                // (m, e - y)
        if (y == 0u) dst[e - x + 1u] = v;                                           // (e - x, -1)
        if (y == e) dst[(size_t)(m + 1u) * side + (e - x + 1u)] = v;                // (e - x, m)
        if ((x == 0u || x == e) && (y == 0u || y == e))                             // the opposite corner of the ring
            dst[(size_t)(y ? 0u : m + 1u) * side + (x ? 0u : m + 1u)] = v;
    }
};

// ---- the tables (include/ptmi.h states them): float64, + - * / and sqrt alone, rounded once ---------------------------------------
constexpr double PI64 = 3.141592653589793;

bool tile_ok(uint32_t tile, uint32_t lo, uint32_t hi) { return tile >= lo && tile <= hi && (tile & (tile - 1u)) == 0u; }
uint32_t log2_of(uint32_t pow2) { uint32_t s = 0; while ((1u << s) < pow2) s++; return s; }

// dir_dw: N * N * 4 floats (d_t, dw_t); basis (may be NULL): N * N * 9
void probe_tables(uint32_t N, float *dir_dw, float *basis) {
    const size_t NN = (size_t)N * N;
    std::vector<double> d(NN * 3), dw(NN);
    const double step = 2.0 / (double)N, cell = 4.0 / ((double)N * (double)N);
    double sum = 0.0;
    for (size_t t = 0; t < NN; t++) {
        const double a = ((double)(t % N) + 0.5) * step - 1.0, b = ((double)(t / N) + 0.5) * step - 1.0;
        const double w = (1.0 - std::fabs(a)) - std::fabs(b);
        double pa = a, pb = b;
        if (w < 0.0) { pa = std::copysign(1.0 - std::fabs(b), a); pb = std::copysign(1.0 - std::fabs(a), b); }
        const double len = std::sqrt((pa * pa + pb * pb) + w * w);
        d[3 * t] = pa / len; d[3 * t + 1] = pb / len; d[3 * t + 2] = w / len;
        dw[t] = cell / ((len * len) * len);
        sum = sum + dw[t];
    }
    const double scale = (4.0 * PI64) / sum;
    for (size_t t = 0; t < NN; t++) {
        const double x = d[3 * t], y = d[3 * t + 1], z = d[3 * t + 2], w = dw[t] * scale;
        if (dir_dw) { dir_dw[4 * t] = (float)x; dir_dw[4 * t + 1] = (float)y; dir_dw[4 * t + 2] = (float)z; dir_dw[4 * t + 3] = (float)w; }
        if (!basis) continue;
        const double Y[9] = {0.28209479177387814,
                             0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
                             (1.0925484305920792 * x) * y, (1.0925484305920792 * y) * z, 0.31539156525252005 * ((3.0 * z) * z - 1.0),
                             (1.0925484305920792 * x) * z, 0.5462742152960396 * (x * x - y * y)};
        for (int k = 0; k < 9; k++) basis[9 * t + k] = (float)(Y[k] * w);
    }
}

// what k_probe_gather stages for a tile of 1 << shift texels a side
size_t tile_lds(uint32_t shift) { return ((size_t)1 << (2u * shift)) * (sizeof(float4) + 3u * sizeof(float)); }

// the default dynamic-LDS cap is 64 KB: raise it for k_probe_gather<Lobe> to what the largest tile takes, once per device. The
// attribute is a kernel's own, so each instantiation has its own `raised`.
template <class Lobe>
void allow_tile_lds() {
    static std::atomic<uint64_t> raised{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (raised.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe_gather<Lobe>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds(6));
    raised.fetch_or(bit, std::memory_order_relaxed);
}

int resolve_params(ptmi_ctx *c, const ptmi_probe_params *params, ptmi_probe_params *out) {
    ptmi_probe_params pp{0u, {0u, 0u, 0u}};
    if (params) pp = *params;
    if (pp._reserved[0] || pp._reserved[1] || pp._reserved[2]) return fail(c, PTMI_E_INVALID, "a reserved word of ptmi_probe_params is not zero");
    *out = pp;
    return PTMI_OK;
}

ProbeSet probe_set(const ptmi_ctx *c) { return ProbeSet{c->d_probes, log2_of(c->probe.tile), c->W / c->probe.tile, c->probe.count}; }
DevProbeAtlas probe_atlas(const ptmi_ctx *c) {
    return DevProbeAtlas{c->d_out, c->d_probes, c->W, log2_of(c->probe.tile), c->W / c->probe.tile, c->probe.count};
}

// what ptmi_probe_sh and ptmi_probe_irradiance check first, and the wait for the dispatches that write what they read
int reduction_ready(ptmi_ctx *c, const float *dst, size_t n_floats, size_t want) {
    if (!dst) return fail(c, PTMI_E_INVALID, "dst is NULL");
    if (!c->d_out) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (!c->d_probes) return fail(c, PTMI_E_INVALID, "no probes in place (ptmi_upload_probes)");
    if (n_floats != want) return fail(c, PTMI_E_INVALID, "expected %zu floats, got %zu", want, n_floats);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));
    return PTMI_OK;
}

// What ptmi_probe_irradiance and ptmi_probe_visibility do once their own parameters are checked: the check of m, reduction_ready, the
// m * m directions of the output tile to the device, k_probe_gather<Lobe> over the probes' tiles of `frame` (the output buffer, the
// depth plane) into scratch, and the copy of the count * side * side float4 to dst.
template <class Lobe>
int gather_tiles(ptmi_ctx *c, const float4 *frame, uint32_t m, const Lobe &lobe, float *dst, size_t n_floats) {
    if (c->d_probes && (!tile_ok(m, 2u, 16u) || m > c->probe.tile))
        return fail(c, PTMI_E_INVALID, "m = %u is not a power of two in [2, min(16, tile = %u)]", m, c->probe.tile);
    const size_t side = lobe.side(m), n = (size_t)c->probe.count * side * side * 4u;
    const int rc = reduction_ready(c, dst, n_floats, n);
    if (rc) return rc;
    std::vector<float> normals((size_t)m * m * 4);
    probe_tables(m, normals.data(), nullptr);
    Scratch<float4> tiles;
    HIP_TRY(c, hipMalloc(&tiles.p, n * sizeof(float)));
    HIP_TRY(c, hipMemcpyAsync(c->d_probe_normals, normals.data(), normals.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DevProbeAtlas a = probe_atlas(c);
    a.out = frame;
    allow_tile_lds<Lobe>();
    hipLaunchKernelGGL(k_probe_gather<Lobe>, dim3(a.count), dim3(BLOCK), tile_lds(a.shift), c->stream, a, c->d_probe_dir_dw,
                       c->d_probe_normals, m, lobe, tiles.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(dst, tiles.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

}  // namespace

void pt_launch_probe_sh(hipStream_t s, DevProbeAtlas a, const float *basis9, float *sh) {
    hipLaunchKernelGGL(k_probe_sh, dim3((a.count + WAVES - 1) / WAVES), dim3(BLOCK), 0, s, a, basis9, sh);
}

PT_HOST {

void probes_forget(ptmi_ctx *c) {
    dfree(c->d_probes); dfree(c->d_probe_list); dfree(c->d_probe_dir_dw); dfree(c->d_probe_basis); dfree(c->d_probe_normals);
    c->probe = {};
}

int probes_check(ptmi_ctx *c, const ptmi_probe_params *params, ListedRays *out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    ptmi_probe_params pp;
    if ((rc = resolve_params(c, params, &pp))) return rc;
    if (!c->d_probes) return fail(c, PTMI_E_INVALID, "no probes in place (ptmi_upload_probes)");
    if ((rc = listed_check(c, "a probe dispatch"))) return rc;
    *out = ListedRays{probe_set(c), c->d_probe_list, c->probe.texels, pp.first_frame,
                      c->probe_depth_on && c->plane[kProbeDepth] ? c->probe_depth.max_distance : 0.0f};
    return PTMI_OK;
}

}  // namespace pt_host

extern "C" {

int ptmi_debug_probe_tables(uint32_t tile, float *dir_dw4, float *basis9) {
    if (!tile_ok(tile, 2u, 64u)) return fail(g_create_err, PTMI_E_INVALID, "tile %u is not a power of two in [2, 64]", tile);
    probe_tables(tile, dir_dw4, basis9);
    return PTMI_OK;
}

// Everything is checked and the new buffers are on the device before the old probes go: a failed call leaves them in place.
int ptmi_upload_probes(ptmi_ctx *c, const ptmi_probe *probes, uint32_t count, uint32_t tile) {
    if (!c) return PTMI_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!probes) {
        HIP_TRY(c, sync_all(c));
        probes_forget(c);
        return PTMI_OK;
    }
    if (!tile_ok(tile, 4u, 64u)) return fail(c, PTMI_E_INVALID, "tile %u is not a power of two in [4, 64]", tile);
    if (c->W == 0 || c->H == 0 || c->W % tile || c->H % tile)
        return fail(c, PTMI_E_INVALID, "the %ux%u output buffer is not a whole number of %ux%u tiles", c->W, c->H, tile, tile);
    const uint32_t cols = c->W / tile, rows = c->H / tile;
    if (count == 0 || count > (uint64_t)cols * rows) return fail(c, PTMI_E_INVALID, "%u probes: the atlas has room for 1 ... %u", count, cols * rows);
    uint32_t enabled = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (!probes[i].enabled) continue;
        for (float v : probes[i].position)
            if (!std::isfinite(v)) return fail(c, PTMI_E_INVALID, "probe %u: the position is not finite", i);
        enabled++;
    }
    // the texels of the enabled probes' tiles, by ascending frame index: rows of the frame from the bottom, each left to right
    std::vector<uint32_t> list;
    list.reserve((size_t)enabled * tile * tile);
    for (uint32_t y = 0; y < c->H; y++)
        for (uint32_t tx = 0; tx < cols; tx++) {
            const uint64_t i = (uint64_t)(y / tile) * cols + tx;
            if (i >= count || !probes[i].enabled) continue;
            for (uint32_t x = tx * tile; x < (tx + 1u) * tile; x++) list.push_back(y * c->W + x);
        }
    const size_t NN = (size_t)tile * tile;
    std::vector<float> dir_dw(NN * 4), basis(NN * 9);
    probe_tables(tile, dir_dw.data(), basis.data());
    float4 *d_rec = nullptr, *d_dir = nullptr, *d_nrm = nullptr;
    uint32_t *d_list = nullptr;
    float *d_basis = nullptr;
    hipError_t e = hipMalloc(&d_rec, (size_t)count * sizeof(ptmi_probe));
    if (e == hipSuccess) e = hipMalloc(&d_list, std::max<size_t>(list.size(), 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_dir, NN * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc(&d_basis, NN * 9 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d_nrm, 256 * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(d_rec, probes, (size_t)count * sizeof(ptmi_probe), hipMemcpyHostToDevice);
    if (e == hipSuccess && !list.empty()) e = hipMemcpy(d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_dir, dir_dw.data(), NN * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_basis, basis.data(), NN * 9 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sync_all(c);               // nothing in flight reads the old probes any more
    if (e != hipSuccess) {
        dfree(d_rec); dfree(d_list); dfree(d_dir); dfree(d_basis); dfree(d_nrm);
        (void)hipGetLastError();
        return fail(c, PTMI_E_HIP, "probe upload failed: %s (the previous probes, if any, are still in place)", hipGetErrorString(e));
    }
    probes_forget(c);
    c->d_probes = d_rec; c->d_probe_list = d_list; c->d_probe_dir_dw = d_dir; c->d_probe_basis = d_basis; c->d_probe_normals = d_nrm;
    c->probe.present = 1u; c->probe.tile = tile; c->probe.count = count; c->probe.enabled = enabled; c->probe.texels = (uint32_t)list.size();
    return PTMI_OK;
}

int ptmi_probe_status(ptmi_ctx *c, struct ptmi_probe_status *out) {
    if (!c || !out) return PTMI_E_INVALID;
    *out = c->probe;
    return PTMI_OK;
}

int ptmi_probe_sh(ptmi_ctx *c, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    const size_t n = (size_t)c->probe.count * 27u;
    const int rc = reduction_ready(c, dst, n_floats, n);
    if (rc) return rc;
    Scratch<float> sh;
    HIP_TRY(c, hipMalloc(&sh.p, n * sizeof(float)));
    pt_launch_probe_sh(c->stream, probe_atlas(c), c->d_probe_basis, sh.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(dst, sh.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTMI_OK;
}

int ptmi_probe_irradiance(ptmi_ctx *c, uint32_t m, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    return gather_tiles(c, c->d_out, m, IrradianceLobe{}, dst, n_floats);
}

int ptmi_probe_visibility(ptmi_ctx *c, const ptmi_probe_visibility_params *params, float *dst, size_t n_floats) {
    if (!c) return PTMI_E_INVALID;
    if (!c->probe_depth_on) return fail(c, PTMI_E_STATE, "the probe depth plane is off (ptmi_set_probe_depth)");
    if (!c->plane[kProbeDepth]) return fail(c, PTMI_E_STATE, "no output buffer (ptmi_resize)");
    if (!params) return fail(c, PTMI_E_INVALID, "params is NULL");
    const ptmi_probe_visibility_params q = *params;
    if (q._reserved) return fail(c, PTMI_E_INVALID, "the reserved word of ptmi_probe_visibility_params is not zero");
    if (q.sharpness_log2 > 6u) return fail(c, PTMI_E_INVALID, "sharpness_log2 = %u is above 6", q.sharpness_log2);
    if (q.border > 1u) return fail(c, PTMI_E_INVALID, "border = %u is not 0 or 1", q.border);
    return gather_tiles(c, plane_as<float4>(c, kProbeDepth), q.m, VisibilityLobe{q.sharpness_log2, q.border}, dst, n_floats);
}

int ptmi_debug_probe_rays(ptmi_ctx *c, const ptmi_probe_params *params, uint32_t n, const uint32_t *xs, const uint32_t *ys,
                          const uint32_t *frames, float *o3, float *d3, uint32_t *rng) {
    if (!c) return PTMI_E_INVALID;
    if (!xs || !ys || !frames || !o3 || !d3) return fail(c, PTMI_E_INVALID, "NULL argument");
    ptmi_probe_params pp;
    int rc = resolve_params(c, params, &pp);
    if (rc) return rc;
    if (!c->d_probes) return fail(c, PTMI_E_INVALID, "no probes in place (ptmi_upload_probes)");
    for (uint32_t i = 0; i < n; i++)
        if (xs[i] >= c->W || ys[i] >= c->H) return fail(c, PTMI_E_INVALID, "texel (%u, %u) outside the %ux%u atlas", xs[i], ys[i], c->W, c->H);
    return debug_listed_rays(c, probe_set(c), c->W, n, xs, ys, frames, o3, d3, rng);
}

}  // extern "C"
