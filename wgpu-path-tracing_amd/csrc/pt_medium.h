// pt_medium.h — the homogeneous participating medium on the device: the interval a ray spends inside the box, free-flight sampling,
// transmittance, the Henyey-Greenstein phase value and its sampling (include/ptmi.h ptmi_set_medium).
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
