"""What the frame-scissor GPU tests share (tests/test_gpu_frame_scissor.py and the files beside it): two handles in one process, the
second created under PTMI_SCISSOR=0, every call given to both, and the scissored one's output and counters required to be the other's
bit for bit. The scissor-off handle is the reference and never the code under test: what it computes is pinned against the oracle
elsewhere (tests/test_gpu_parity.py and the files beside it)."""
import ctypes
import os

import numpy as np

from ptmi import native, scene_host

W, H, FRAMES = 96, 54, 5


def make_pair(create=lambda: native.Context(0)):
    """(scissored, full): two handles from create(), the second made with the scissor switched off; the environment is left as found"""
    old = os.environ.pop("PTMI_SCISSOR", None)
    on = create()
    os.environ["PTMI_SCISSOR"] = "0"
    try:
        off = create()
    finally:
        if old is None:
            del os.environ["PTMI_SCISSOR"]
        else:
            os.environ["PTMI_SCISSOR"] = old
    return on, off


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counters(ctx):
    st = ctx.stats()
    return (int(st.paths), int(st.segments), [int(v) for v in st.segments_by_bounce], int(st.shadow_rays), int(st.frames_per_batch_used))


def render(ctx, scene, cam, dispatch=None, frames=FRAMES, fill=0.25, **opt):
    """one dispatch of `frames` frames on a frame of the camera's size; fill None: the output buffer keeps what it holds"""
    w, h = int(cam["width"]), int(cam["height"])
    o = dict(max_bounces=3, do_mis=1, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0, frames_per_batch=2, timing=0)
    o.update(opt)
    ctx.set_options(**o)
    if getattr(ctx, "_scissor_scene", None) is not scene:
        ctx.upload_scene(scene)
        ctx._scissor_scene = scene
    if fill is not None or (ctx.width, ctx.height) != (w, h):
        ctx.resize(w, h)
    if fill is not None:
        ctx.write_output(np.full((h, w, 4), fill, np.float32))   # rows of another part keep this; frame 0 overwrites the rest
    ctx.reset_stats()
    (dispatch or (lambda: ctx.dispatch(cam, frames)))()
    return ctx.read_output(), counters(ctx), ctx.scissor_status().as_dict()


def both(pair, scene, cam, **kw):
    """renders on both contexts; asserts equal frames and counters; returns the scissored context's status, counters and frame"""
    on, off = pair
    w, h = int(cam["width"]), int(cam["height"])
    a, ca, sa = render(on, scene, cam, **kw)
    b, cb, sb = render(off, scene, cam, **kw)
    assert sb["applied"] == 0 and sb["reason"] == native.SCISSOR_OFF and sb["skipped"] == 0
    assert (sb["x0"], sb["x1"], sb["y0"], sb["y1"]) == (0, w, 0, h)
    assert ca == cb, (ca, cb)
    assert np.array_equal(bits(a), bits(b)), np.argwhere((bits(a) != bits(b)).any(-1))[:8]
    return sa, ca, a


def forget_scene(pair):
    """the next render() uploads again: after an edit of the loaded scene, or a change of an option that an upload reads"""
    for c in pair:
        c._scissor_scene = None


def rect(st):
    return st["x0"], st["x1"], st["y0"], st["y1"]


def contains(outer, inner):
    """rectangles (x0, x1, y0, y1): every pixel of inner is one of outer"""
    if inner[0] >= inner[1] or inner[2] >= inner[3]:
        return True
    return outer[0] <= inner[0] and inner[1] <= outer[1] and outer[2] <= inner[2] and inner[3] <= outer[3]


def host_rect(cam, lo, hi):
    """csrc/scene/frame_scissor.cpp pt_frame_scissor on the box [lo, hi]: (answer, (x0, x1, y0, y1)); answer 0 is a rectangle"""
    f = scene_host.lib().pt_frame_scissor
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.POINTER(ctypes.c_uint32)] * 4
    lo, hi = (np.ascontiguousarray(b, np.float32) for b in (lo, hi))
    r = [ctypes.c_uint32(7) for _ in range(4)]
    why = f(cam.ctypes.data, lo.ctypes.data, hi.ctypes.data, *[ctypes.byref(v) for v in r])
    return why, tuple(int(v.value) for v in r)


def triangle_bounds(tris):
    """the exact min / max of the vertices of TRIANGLE records"""
    v = np.concatenate([tris[k] for k in ("v0", "v1", "v2")])
    return v.min(0), v.max(0)


def slab_hits(o, d, lo, hi):
    """(n,) bool: the ray o + t d, t >= 0, meets the box [lo, hi]; float64; the slab test of tests/test_frame_scissor_host.py rays_hit"""
    o, d, lo, hi = (np.asarray(a, np.float64) for a in (o, d, lo, hi))
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    par = d == 0.0                                              # parallel to a slab: inside it for all t, or never
    inside = (o >= lo) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    return tf.min(-1) >= np.maximum(tn.max(-1), 0.0)
