"""Every per-pixel plane of a context at once (include/ptmi.h): the output buffer, the three first-hit planes, the moments plane, the
denoiser's, the adaptive sampler's and the blit staging, across ptmi_resize to a larger, a smaller and an unchanged size, and the
caller-owned output binding (ptmi_bind_output_device). Only bit equality and exact error codes are asserted."""
import numpy as np
import pytest

from ptmi import layout, native

pytestmark = pytest.mark.gpu

E_STATE = -4
W, H = 24, 16
BIG = (W + 8, H + 4)
AOVS = ("albedo", "normal", "id")
ADAPTIVE = dict(threshold=1e-3, min_frames=4, step=2)        # after 2 frames every pixel is below min_frames: the list is the frame


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def at(cam, frame):
    c = cam.copy()
    c["frame_index"] = frame
    return c


def setup(c, sc, size):
    c.set_options(max_bounces=8, do_mis=1, frames_per_batch=0, leaves=0, timing=0)
    c.upload_scene(sc)
    c.resize(*size)
    c.set_aovs(*AOVS)
    c.set_moments(True)


def render(c):
    """2 frames, the denoiser, one adaptive round and both blits on a context whose planes hold zeros; every read-back by name"""
    cam = layout.make_camera(c.width, c.height)
    c.dispatch(at(cam, 0), 2)
    got = {"denoised": c.denoise()}
    c.dispatch_adaptive(at(cam, 2), 1, **ADAPTIVE)
    got["blit_f32"], got["blit_u8"] = c.blit()
    got["blit_denoised_f32"], got["blit_denoised_u8"] = c.blit_denoised()
    got["output"], got["moments"] = c.read_output(), c.read_moments()
    for name in AOVS:
        got[name] = c.read_aov(name)
    st = c.adaptive_status().as_dict()
    assert st["rounds"] == 1 and st["max_count"] == 4           # the round ran, on top of the two frames
    got["status"] = np.array([st[k] for k in sorted(st)], np.uint64)
    return got


_fresh = {}


def fresh(sc, size):
    """render() on a context created at `size`, once per size"""
    if size not in _fresh:
        with native.Context(0) as c:
            setup(c, sc, size)
            _fresh[size] = render(c)
    return _fresh[size]


@pytest.mark.parametrize("start,target", [((W, H), BIG), (BIG, (W, H)), ((W, H), (W, H))], ids=["grow", "shrink", "same"])
def test_all_planes_across_resize(ctx, scene_factory, start, target):
    sc = scene_factory("cornell")
    setup(ctx, sc, start)
    before = render(ctx)
    assert before["output"].any() and before["moments"].any() and all(before[n].any() for n in AOVS)
    ctx.resize(*target)
    shape = (target[1], target[0])
    planes = {"output": ctx.read_output(), "moments": ctx.read_moments(), **{n: ctx.read_aov(n) for n in AOVS}}
    for name, a in planes.items():
        assert a.shape[:2] == shape, name
        assert not bits(a).any(), f"{name} is not zero after the resize"
    assert ctx.aovs() == AOVS and ctx.moments()
    assert ctx.denoised_device_ptr() is None
    with pytest.raises(native.PtmiError) as e:
        ctx.blit_denoised()
    assert e.value.code == E_STATE
    assert not any(ctx.adaptive_status().as_dict().values())
    got, want = render(ctx), fresh(sc, target)
    assert got.keys() == want.keys()
    for name in want:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(bits(got[name]), bits(want[name])), f"{name} differs from a context created at {target}"


def test_caller_owned_output(ctx, scene_factory):
    import torch
    sc = scene_factory("cornell")
    setup(ctx, sc, (W, H))
    cam = layout.make_camera(W, H)
    own = ctx.output_device_ptr()
    frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    assert own is not None and own != frame.data_ptr()
    ctx.bind_output_device(frame.data_ptr(), frame.numel() * 4)
    assert ctx.output_device_ptr() == frame.data_ptr()
    ctx.dispatch(at(cam, 0), 2)
    ctx.synchronize()
    rendered = frame.cpu().numpy().reshape(H, W, 4)
    assert rendered.any()
    assert np.array_equal(bits(rendered), bits(ctx.read_output()))
    assert np.array_equal(bits(rendered), bits(fresh_output(sc)))          # what the context's own buffer gets from the same frames
    ctx.bind_output_device(0, 0)
    assert ctx.output_device_ptr() == own != frame.data_ptr()
    assert not ctx.read_output().any()                                     # the dispatch wrote the bound buffer only
    ctx.bind_output_device(frame.data_ptr(), frame.numel() * 4)
    ctx.resize(*BIG)
    assert ctx.output_device_ptr() not in (None, frame.data_ptr())
    assert ctx.read_output().shape == (BIG[1], BIG[0], 4) and not ctx.read_output().any()
    assert np.array_equal(bits(frame.cpu().numpy().reshape(H, W, 4)), bits(rendered)), "the resize touched the caller's buffer"


def fresh_output(sc):
    with native.Context(0) as c:
        setup(c, sc, (W, H))
        c.dispatch(at(layout.make_camera(W, H), 0), 2)
        return c.read_output()
