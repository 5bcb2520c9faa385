// frame_scissor.cpp — which pixels of a frame can see a box at all: the rectangle a plain dispatch restricts its camera paths to.
//
// A pixel outside the rectangle has no camera ray that meets the box, whatever its RNG draws, so its paths end at bounce 0 with radiance
// 0 and need not be traced (dispatch.hip; DESIGN.md §25 has the argument in full). Everything here is double precision and errs
// towards the larger rectangle; where it cannot promise, it answers "whole frame".
//
// The pinhole ray of the image-plane point (px, py), in pixels, has the direction fw + a rt + b up with a = (2 px / W - 1) th aspect,
// b = (2 py / H - 1) th, th = tan(fov / 2) (pipeline.hip camera_dir). A point pos + q lies on it iff q = s fw + (s a) rt + (s b) up with
// s > 0: (s, s a, s b) = M^-1 q, M = [fw rt up]. M^-1 maps the box to a convex polytope; while s > 0 on all eight corners it is > 0 on
// all of it, and a = u / s, b = v / s are ratios of linear functions: each face of the box maps to the convex quadrilateral of its four
// projected corners. The camera is outside the box, so a ray that meets the box meets a face: the six quadrilaterals, clipped to the
// frame, hold every (px, py) on the frame whose pinhole ray meets the box, and the rectangle is their bounds.
//
// The lens (pipeline.hip camera_ray): origin pos + off, |off| <= A, through the focal point pos + f d (d the unit pinhole direction, f
// the focus distance). Its point at parameter l >= 0 is pos + l f d + (1 - l) off: the pinhole ray's point at distance l f, displaced by
// at most |1 - l| A. If that point is in the box, whose farthest corner is D from pos, then l f <= D + |1 - l| A; for l > 1 and f > A
// this gives l <= (D - A) / (f - A), a displacement of at most A (D - f) / (f - A). So the lens ray meets the box only if the pinhole
// ray meets the box inflated by A max(1, (D - f) / (f - A)) on every axis. (l = 0 is the camera inside the inflated box: whole frame.)
#include "frame_scissor.h"

#include <algorithm>
#include <cmath>

namespace {

struct d3 { double x, y, z; };
d3 sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
d3 of(const float v[3]) { return {(double)v[0], (double)v[1], (double)v[2]}; }
bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

struct p2 { double x, y; };

constexpr double kPixelMargin = 2.0;            // the float32 rounding of the device's ray, in pixels, on every side
// ... and across the frame's edge, where the image of the box is clipped. The device's image-plane coordinate is good to a few ulp of
// its largest value, W / 2 pixels times 2^-21 or so: 0.03 pixels at the largest frame taken here.
constexpr double kClipMargin = 1.0 / 16.0;
constexpr uint32_t kMaxSide = 65536u;
constexpr double kBoxMargin = 1.0 / 65536.0;    // ... and of its box tests: relative to the largest coordinate (the own tree's padding)
constexpr double kFront = 1e-6;                 // a corner is in front while its depth is above this share of its distance
constexpr double kMaxFov = 3.0;                 // tan(fov / 2) in float32 is good to a few ulp up to here

// pixels [lo, hi) that the interval [pmin, pmax] of image-plane coordinates, widened by the margin, touches; clipped to [0, n)
void pixel_range(double pmin, double pmax, uint32_t n, uint32_t &lo, uint32_t &hi) {
    const double a = std::floor(std::max(pmin, -8.0)) - kPixelMargin, b = std::floor(std::min(pmax, (double)n + 8.0)) + 1.0 + kPixelMargin;
    lo = (uint32_t)std::min(std::max(a, 0.0), (double)n);
    hi = (uint32_t)std::min(std::max(b, 0.0), (double)n);
}

}  // namespace

extern "C" int pt_frame_scissor(const ptmi_camera *cam, const float box_min[3], const float box_max[3],
                                uint32_t *x0, uint32_t *x1, uint32_t *y0, uint32_t *y1) {
    const uint32_t W = cam->width, H = cam->height;
    *x0 = 0u; *x1 = W; *y0 = 0u; *y1 = H;                       // the whole frame, until the rectangle is a promise
    if (W == 0u || H == 0u) return PT_SCISSOR_NOT_FINITE;
    if (W > kMaxSide || H > kMaxSide) return PT_SCISSOR_DEGENERATE;
    if (!finite3(cam->position) || !finite3(cam->forward) || !finite3(cam->right) || !finite3(cam->up) || !std::isfinite(cam->fov) ||
        !std::isfinite(cam->aspect) || !std::isfinite(cam->aperture) || !std::isfinite(cam->focus_distance) || !finite3(box_min) ||
        !finite3(box_max))
        return PT_SCISSOR_NOT_FINITE;
    if (ptmi_camera_projection(cam) != PTMI_PROJ_PERSPECTIVE) return PT_SCISSOR_PROJECTION;
    d3 lo = of(box_min), hi = of(box_max);
    if (lo.x > hi.x || lo.y > hi.y || lo.z > hi.z) return PT_SCISSOR_NOT_FINITE;
    if (!(cam->fov > 0.0f) || (double)cam->fov > kMaxFov || !(cam->aspect > 0.0f)) return PT_SCISSOR_DEGENERATE;
    const double th = std::tan((double)cam->fov * 0.5), tx = th * (double)cam->aspect;
    const d3 pos = of(cam->position), fw = of(cam->forward), rt = of(cam->right), up = of(cam->up);

    // the box the kernels test, and a little more
    double big = 0.0;
    for (double v : {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}) big = std::max(big, std::fabs(v));
    double grow = big * kBoxMargin;
    auto corner = [&](int i, double g) { return d3{(i & 1 ? hi.x + g : lo.x - g), (i & 2 ? hi.y + g : lo.y - g), (i & 4 ? hi.z + g : lo.z - g)}; };
    if (cam->aperture > 0.0f) {
        const double r2 = dot(rt, rt), u2 = dot(up, up);
        const double A = (double)cam->aperture * std::sqrt(std::max(r2, u2) + std::fabs(dot(rt, up)));      // |up r sin + rt r cos| <= A
        const double f = (double)cam->focus_distance;
        if (!(f > A)) return PT_SCISSOR_DEGENERATE;
        double D = 0.0;
        for (int i = 0; i < 8; i++) { const d3 q = sub(corner(i, grow), pos); D = std::max(D, std::sqrt(dot(q, q))); }
        grow += A * std::max(1.0, (D - f) / (f - A));
    }
    if (!std::isfinite(grow)) return PT_SCISSOR_NOT_FINITE;
    lo = corner(0, grow); hi = corner(7, grow);
    if (pos.x >= lo.x && pos.x <= hi.x && pos.y >= lo.y && pos.y <= hi.y && pos.z >= lo.z && pos.z <= hi.z) return PT_SCISSOR_INSIDE;

    // M^-1 by cofactors
    const d3 c_s = cross(rt, up), c_u = cross(up, fw), c_v = cross(fw, rt);
    const double det = dot(fw, c_s);
    const double scale = std::sqrt(dot(fw, fw) * dot(rt, rt) * dot(up, up));
    if (!(scale > 0.0) || !(std::fabs(det) > 1e-6 * scale)) return PT_SCISSOR_DEGENERATE;
    const double fwl = std::sqrt(dot(fw, fw));
    p2 at[8];
    for (int i = 0; i < 8; i++) {
        const d3 q = sub(corner(i, grow), pos);
        const double s = dot(q, c_s) / det, u = dot(q, c_u) / det, v = dot(q, c_v) / det;
        if (!(s * fwl > kFront * std::sqrt(dot(q, q)))) return PT_SCISSOR_BEHIND;
        at[i] = {(u / s / tx + 1.0) * 0.5 * (double)W, (v / s / th + 1.0) * 0.5 * (double)H};
        if (!std::isfinite(at[i].x) || !std::isfinite(at[i].y)) return PT_SCISSOR_NOT_FINITE;
    }
    // The image of the box is the union of its six faces' images, each a convex quadrilateral. Only what lies on the frame counts (a
    // corner far off the frame must not widen the rectangle on it), so each is clipped to the frame — a little more than the frame,
    // for the device's rounding across the clip line — before the bounds are taken.
    static const int kFaces[6][4] = {{0, 2, 6, 4}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 5, 7, 6}};
    double pxmin = INFINITY, pxmax = -INFINITY, pymin = INFINITY, pymax = -INFINITY;
    for (const auto &face : kFaces) {
        p2 poly[16], next[16];
        int n = 4;
        for (int k = 0; k < 4; k++) poly[k] = at[face[k]];
        // Sutherland-Hodgman against x >= -m, x <= W + m, y >= -m, y <= H + m: side e keeps sign * (coordinate) <= bound
        for (int e = 0; e < 4 && n > 0; e++) {
            const bool is_x = e < 2;
            const double sign = (e & 1) ? 1.0 : -1.0, bound = (e & 1) ? (double)(is_x ? W : H) + kClipMargin : kClipMargin;
            auto dist = [&](p2 p) { return sign * (is_x ? p.x : p.y) - bound; };       // <= 0: kept
            int m = 0;
            for (int k = 0; k < n; k++) {
                const p2 a = poly[k], b = poly[(k + 1) % n];
                const double da = dist(a), db = dist(b);
                if (da <= 0.0) next[m++] = a;
                if ((da <= 0.0) != (db <= 0.0)) { const double t = da / (da - db); next[m++] = {a.x + t * (b.x - a.x), a.y + t * (b.y - a.y)}; }
            }
            n = m;
            for (int k = 0; k < n; k++) poly[k] = next[k];
        }
        for (int k = 0; k < n; k++) {
            pxmin = std::min(pxmin, poly[k].x); pxmax = std::max(pxmax, poly[k].x);
            pymin = std::min(pymin, poly[k].y); pymax = std::max(pymax, poly[k].y);
        }
    }
    if (!(pxmin <= pxmax)) { *x0 = *x1 = *y0 = *y1 = 0u; return PT_SCISSOR_RECT; }      // the box is off the frame
    pixel_range(pxmin, pxmax, W, *x0, *x1);
    pixel_range(pymin, pymax, H, *y0, *y1);
    if (*x0 >= *x1 || *y0 >= *y1) *x0 = *x1 = *y0 = *y1 = 0u;
    return PT_SCISSOR_RECT;
}
