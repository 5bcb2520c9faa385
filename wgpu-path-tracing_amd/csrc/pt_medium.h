// pt_medium.h — the participating medium on the device: the interval a ray spends inside the box, free-flight sampling,
// transmittance, the Henyey-Greenstein phase value and its sampling (include/ptmi.h ptmi_set_medium); and, while a
// density grid is in place, the grid lookup with delta and ratio tracking (ptmi_upload_medium_density).
// Included by shade.hip (both builds) and by medium.hip, whose debug kernels call the same functions the renders run.
//
// Arithmetic: ln and exp are the device's logf / expf, so the free-flight distance, the scatter decision within rounding of the
// interval's end and the transmittance are outside the arithmetic contract (like the sky lookup and blit). Everything else is float32
// in the order written: the reciprocals of the direction in the slab test are the contract's rcp1, the square roots its sqrt1, sin / cos
// its sincos1, and every other quotient is a plain '/', which the contract build rounds correctly (PT_SHADE_FAST: the fast forms).
#pragma once
#include "pt_device.h"
#include "pt_math.h"

#define PT_FOUR_PI 12.5663706144f
// k_shade's MED axis: which medium code an instantiation contains
enum { PT_MED_NONE = 0, PT_MED_HOMOGENEOUS = 1, PT_MED_GRID = 2 };

struct MedInterval { float near, far, a, b; };      // the ray is inside the box for t in [near, far]; the segment for t in (a, b)

// The slab test of the box per axis with fmin / fmax (v_min_f32 / v_max_f32: a NaN from 0 * inf gives the other operand).
// t_hit: the segment's end, +inf on a miss. No interval: NOT b > a. A ray whose slab distances are NaN on all three axes (the NaN origin or
// direction of a degenerate path; far is NaN only then) would leave the fmin / fmax as inside the medium from 0 to t_hit, wherever the
// box is: it has no interval.
PT_DEV MedInterval med_interval(const DevMedium &m, v3 o, v3 d, float t_hit) {
    const float ix = rcp1(d.x), iy = rcp1(d.y), iz = rcp1(d.z);
    const float x1 = (m.box_min[0] - o.x) * ix, x2 = (m.box_max[0] - o.x) * ix;
    const float y1 = (m.box_min[1] - o.y) * iy, y2 = (m.box_max[1] - o.y) * iy;
    const float z1 = (m.box_min[2] - o.z) * iz, z2 = (m.box_max[2] - o.z) * iz;
    MedInterval r;
    r.near = max1(max1(min1(x1, x2), min1(y1, y2)), min1(z1, z2));
    r.far = min1(min1(max1(x1, x2), max1(y1, y2)), max1(z1, z2));
    r.a = max1(r.near, 0.0f);
    r.b = r.far == r.far ? min1(r.far, t_hit) : r.a;
    return r;
}
// the distance to the next collision from one uniform in [0, 1]: r = 1 gives +inf (no collision), r = 0 gives 0
PT_DEV float med_free_flight(const DevMedium &m, float r) { return -logf(1.0f - r) / m.sigma_t; }
// the transmittance of a next-event sample from o towards wi, dist away (dist < 0: directional or sky, to the box's far side)
PT_DEV float med_tr(const DevMedium &m, v3 o, v3 wi, float dist) {
    const MedInterval iv = med_interval(m, o, wi, __builtin_inff());
    const float end = dist < 0.0f ? iv.far : min1(iv.far, dist);
    return expf(-m.sigma_t * max1(0.0f, end - iv.a));
}
// Henyey-Greenstein: value and density of scattering from the direction of travel d into wi, cos_t = dot(d, wi)
PT_DEV float med_phase(float g, float cos_t) {
    const float g2 = g * g;
    const float k = 1.0f + g2 - 2.0f * g * cos_t;
    return (1.0f - g2) / (PT_FOUR_PI * (k * sqrt1(k)));
}
// the direction a scatter takes, from two uniforms: cos theta about d by inversion of the phase function, the azimuth in the frame of
// Duff et al. 2017 about d. cos_out: the sampled cosine (the direction's phase value is med_phase(g, cos_out)).
PT_DEV v3 med_sample_phase(float g, v3 d, float xi1, float xi2, float &cos_out) {
    float ct;
    if (__builtin_fabsf(g) < 1e-3f) {
        ct = 1.0f - 2.0f * xi1;
    } else {
        const float g2 = g * g;
        const float q = (1.0f - g2) / (1.0f - g + 2.0f * g * xi1);
        ct = (1.0f + g2 - q * q) / (2.0f * g);
    }
    ct = min1(max1(ct, -1.0f), 1.0f);
    const float st = sqrt1(max1(0.0f, 1.0f - ct * ct));
    float sp, cp; sincos1((2.0f * PT_PI) * xi2, sp, cp);
    const float sg = __builtin_copysignf(1.0f, d.z);
    const float A = -1.0f / (sg + d.z);
    const float B = d.x * d.y * A;
    const v3 T = mk3(1.0f + sg * d.x * d.x * A, sg * B, -sg * d.x);
    const v3 U = mk3(B, sg + d.y * d.y * A, -d.y);
    cos_out = ct;
    return normalize3(lincomb3(T, st * cp, U, st * sp, d, ct));
}

// ---- the density grid: sigma_t * rho(x), rho in [0, 1], so that sigma_t is the majorant everywhere ------------------------------------
// The lookup is under the arithmetic contract: float32 in the order written, the quotient a plain '/', no fused step (the contract
// build compiles with contraction off). The tracking decisions are outside it, like the free-flight draw they replace.
//
// Both tracking loops stop after PT_MED_TRACK_CAP iterations: a delta-tracking segment then ends its path, a ratio-tracking sample
// gives T = 0. The cap is a guard for a shared machine and nothing a render or a test may reach: a grid is accepted only while
// sigma_t * |box diagonal| <= PT_MED_MAX_DEPTH, which bounds the expected number of tentative collisions of a segment by 256 and makes
// 65 536 of them an event of probability below e^-60000.
#define PT_MED_TRACK_CAP 65536u
#define PT_MED_MAX_DEPTH 256.0
enum { PT_TRACK_PASSED = 0, PT_TRACK_SCATTERED = 1, PT_TRACK_CAPPED = 2 };

// a cell index from a floored coordinate: clamped to [0, n - 1]; NaN gives 0 (v_max_f32 returns the other operand)
PT_DEV uint32_t med_cell(float f, uint32_t n) { return (uint32_t)min1(max1(f, 0.0f), (float)(n - 1u)); }
PT_DEV float med_grid_coord(float p, float lo, float hi, uint32_t n) { return (p - lo) / (hi - lo) * (float)n; }
// rho at p. Cell (i, j, k) is entry (k * ny + j) * nx + i and covers box_min + (i .. i + 1) / nx * extent on x, likewise on y and z.
// filter 0: the cell that holds p. filter 1: trilinear over the cell centres, the taps clamped at the faces, along x, then y, then z.
PT_DEV float med_density(const DevMedium &m, v3 p) {
    const float ux = med_grid_coord(p.x, m.box_min[0], m.box_max[0], m.nx);
    const float uy = med_grid_coord(p.y, m.box_min[1], m.box_max[1], m.ny);
    const float uz = med_grid_coord(p.z, m.box_min[2], m.box_max[2], m.nz);
    const float *__restrict__ g = m.grid;
    if (m.filter == 0u) {
        const uint32_t i = med_cell(__builtin_floorf(ux), m.nx), j = med_cell(__builtin_floorf(uy), m.ny), k = med_cell(__builtin_floorf(uz), m.nz);
        return g[(k * m.ny + j) * m.nx + i];
    }
    const float vx = ux - 0.5f, vy = uy - 0.5f, vz = uz - 0.5f;
    const float bx = __builtin_floorf(vx), by = __builtin_floorf(vy), bz = __builtin_floorf(vz);
    const float fx = vx - bx, fy = vy - by, fz = vz - bz;
    const uint32_t i0 = med_cell(bx, m.nx), i1 = med_cell(bx + 1.0f, m.nx);
    const uint32_t j0 = med_cell(by, m.ny), j1 = med_cell(by + 1.0f, m.ny);
    const uint32_t k0 = med_cell(bz, m.nz), k1 = med_cell(bz + 1.0f, m.nz);
    const uint32_t r00 = (k0 * m.ny + j0) * m.nx, r10 = (k0 * m.ny + j1) * m.nx;
    const uint32_t r01 = (k1 * m.ny + j0) * m.nx, r11 = (k1 * m.ny + j1) * m.nx;
    const float c000 = g[r00 + i0], c100 = g[r00 + i1], c010 = g[r10 + i0], c110 = g[r10 + i1];
    const float c001 = g[r01 + i0], c101 = g[r01 + i1], c011 = g[r11 + i0], c111 = g[r11 + i1];
    const float gx = 1.0f - fx, gy = 1.0f - fy, gz = 1.0f - fz;
    const float c00 = c000 * gx + c100 * fx, c10 = c010 * gx + c110 * fx;
    const float c01 = c001 * gx + c101 * fx, c11 = c011 * gx + c111 * fx;
    const float c0 = c00 * gy + c10 * fy, c1 = c01 * gy + c11 * fy;
    return c0 * gz + c1 * fz;
}
// Delta (Woodcock) tracking of the segment (a, b) of the ray (o, d), b > a: tentative collisions at the majorant's rate, each real with
// probability rho. Two draws per tentative collision, the second also where rho is 0 or 1; the last free flight takes one.
// PT_TRACK_SCATTERED: at t_out. steps: the tentative collisions (lookups).
PT_DEV int med_delta_track(const DevMedium &m, v3 o, v3 d, float a, float b, uint32_t &rng, float &t_out, uint32_t &steps) {
    float t = a;
    t_out = 0.0f; steps = 0u;
    for (uint32_t k = 0u; k < PT_MED_TRACK_CAP; k++) {
        t += med_free_flight(m, rng_f(rng));
        if (!(t < b)) return PT_TRACK_PASSED;
        steps++;
        const float rho = med_density(m, madd3(d, t, o));
        if (rng_f(rng) < rho) { t_out = t; return PT_TRACK_SCATTERED; }
    }
    return PT_TRACK_CAPPED;
}
// Ratio tracking of a next-event sample from o towards wi, dist away (dist < 0: directional or sky, to the box's far side): the
// product of 1 - rho over the tentative collisions of (max(near, 0), end), near / far / end as med_tr has them. One draw per tentative
// collision and one for the flight that leaves the segment (also where the segment is empty). A product of exactly 0 stops the loop.
PT_DEV float med_ratio_track(const DevMedium &m, v3 o, v3 wi, float dist, uint32_t &rng, uint32_t &steps, float &end_out) {
    const MedInterval iv = med_interval(m, o, wi, __builtin_inff());
    const float end = dist < 0.0f ? iv.far : min1(iv.far, dist);
    float t = iv.a, T = 1.0f;
    end_out = end; steps = 0u;
    for (uint32_t k = 0u; k < PT_MED_TRACK_CAP; k++) {
        t += med_free_flight(m, rng_f(rng));
        if (!(t < end)) return T;
        steps++;
        T *= 1.0f - med_density(m, madd3(wi, t, o));
        if (T == 0.0f) return T;
    }
    return 0.0f;
}
PT_DEV float med_ratio_track(const DevMedium &m, v3 o, v3 wi, float dist, uint32_t &rng) {
    uint32_t steps; float end;
    return med_ratio_track(m, o, wi, dist, rng, steps, end);
}
