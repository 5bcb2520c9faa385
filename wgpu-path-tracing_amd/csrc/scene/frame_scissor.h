// frame_scissor.h — the conservative frame scissor of a plain dispatch (frame_scissor.cpp). Host code, no GPU: built
// into libptmi_scene.so, where the tests reach it, and into libptmi.so, where dispatch() calls it.
#pragma once
#include <stdint.h>
#include "ptmi_layout.h"

// why pt_frame_scissor answered "whole frame" (0: it did not)
enum {
    PT_SCISSOR_RECT = 0,            // the rectangle is a promise
    PT_SCISSOR_NOT_FINITE = 1,      // a field of the camera or the box is not finite, or the box is inverted, or the frame is empty
    PT_SCISSOR_PROJECTION = 2,      // the camera's projection word is not PTMI_PROJ_PERSPECTIVE
    PT_SCISSOR_INSIDE = 3,          // the camera's position lies inside the inflated box (or on it)
    PT_SCISSOR_BEHIND = 4,          // a corner of the inflated box is not strictly in front of the camera
    PT_SCISSOR_DEGENERATE = 5,      // fov outside (0, 3], aspect <= 0, a singular basis, a lens as wide as its focus distance, or a
                                    // frame side above 65 536
};

#ifdef __cplusplus
extern "C" {
#endif
// The pixel rectangle [*x0, *x1) x [*y0, *y1) of cam's width x height frame outside which every camera ray misses the box
// [box_min, box_max]: every jitter in [0, 1]^2, every lens sample. Returns PT_SCISSOR_RECT with the rectangle (x0 = x1 = y0 = y1 = 0:
// no pixel can meet the box), or the reason it cannot promise anything, with the whole frame as the rectangle. The projection words of
// the camera are read: a caller whose context leaves them unread passes a copy with the words zeroed.
int pt_frame_scissor(const ptmi_camera *cam, const float box_min[3], const float box_max[3],
                     uint32_t *x0, uint32_t *x1, uint32_t *y0, uint32_t *y1);
#ifdef __cplusplus
}
#endif
