"""The context's two blocks of counter and control words (csrc/pt_device.h CounterWord, ControlWord), seen through the calls that read
them: ptmi_get_stats, ptmi_adaptive_status, ptmi_reproject_status. Every word has one owner: nothing reads as used before its first
use, the queue lengths of 65 bounces and the two shadow-queue lengths do not meet, a reset or a resize clears its own words and no
others, and two contexts on one device keep their words apart. Cornell at 16 x 16, a fresh context per case."""
import numpy as np
import pytest

from ptmi import layout, native

pytestmark = pytest.mark.gpu

W, H, FRAMES = 16, 16, 2
COUNTERS = ("paths", "segments", "shadow_rays", "shadow_traced", "verify_failed", "frames", "dispatches")
ADAPTIVE = dict(rounds=1, threshold=1e-6, min_frames=4, max_frames=8, step=2)


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS) + tuple(int(v) for v in st.segments_by_bounce)


def at(cam, frame):
    c = cam.copy()
    c["frame_index"] = frame
    return c


def fresh(sc, aovs=(), moments=False, **opt):
    ctx = native.Context(0)
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    ctx.set_aovs(*aovs)
    ctx.set_moments(moments)
    ctx.set_options(**opt)
    return ctx


def test_nothing_used_yet(scene_factory):
    with fresh(scene_factory("cornell"), moments=True) as ctx:
        assert ctx.reproject_status().as_dict() == dict(carried=0, disoccluded=0, missed=0, samples=0)
        assert ctx.adaptive_status().as_dict() == dict(active=0, samples=0, min_count=0, max_count=0, rounds=0)
        st = ctx.stats()
        assert (st.paths, st.segments, st.shadow_rays, st.verify_failed) == (0, 0, 0, 0)


def test_deepest_bounce_one_and_two_streams(scene_factory):
    """max_bounces = 64: the queue lengths use their run to its last word, and with overlap both shadow-queue lengths are in use"""
    sc, cam = scene_factory("cornell"), layout.make_camera(W, H)
    got = []
    for overlap in (0, 1):
        with fresh(sc, max_bounces=64, do_mis=1, frames_per_batch=2, overlap=overlap) as ctx:
            ctx.dispatch(cam, FRAMES)
            out, st = ctx.read_output(), ctx.stats()
        by = [int(v) for v in st.segments_by_bounce]
        print("overlap", overlap, "segments", st.segments, "shadow", st.shadow_rays, st.shadow_traced, "by bounce", by)
        assert sum(by) == st.segments and by[0] == W * H * FRAMES
        assert all(a >= b for a, b in zip(by, by[1:]))
        assert st.shadow_traced <= st.shadow_rays
        got.append((out.view(np.uint32), counters(st)))
    assert np.array_equal(got[0][0], got[1][0]), "one and two streams gave other bits"
    assert got[0][1] == got[1][1], "one and two streams gave other counters"


def sequence(ctx, cam, between=lambda: None):
    """a dispatch, an adaptive round and a reprojection, then a reset and a resize: asserts what each may touch, returns the three reads"""
    ctx.dispatch(cam, FRAMES)
    between()
    ctx.dispatch_adaptive(at(cam, FRAMES), **ADAPTIVE)
    between()
    ctx.reproject(cam, cam)
    between()
    st, ad, rp = counters(ctx.stats()), ctx.adaptive_status().as_dict(), ctx.reproject_status().as_dict()
    print("stats", st[:len(COUNTERS)], "adaptive", ad, "reproject", rp)
    # every pixel has 2 frames, fewer than min_frames: the round lists all of them, and its paths are counted on the device
    assert ad["active"] == W * H and ad["rounds"] == 1
    assert st[COUNTERS.index("paths")] == W * H * (FRAMES + ADAPTIVE["step"]) and st[COUNTERS.index("segments")] > 0
    assert rp["carried"] + rp["disoccluded"] + rp["missed"] == W * H

    ctx.reset_stats()
    between()
    zeroed = ctx.stats()
    assert counters(zeroed)[:5] == (0, 0, 0, 0, 0) and not any(zeroed.segments_by_bounce)
    n = ctx.read_moments()[..., 2].astype(np.uint64)
    assert ctx.adaptive_status().as_dict() == dict(ad, samples=int(n.sum()), min_count=int(n.min()), max_count=int(n.max()))
    assert ctx.reproject_status().as_dict() == rp

    ctx.resize(W, H)
    ctx.set_aovs("normal")                      # (the planes that were on stay on)
    ctx.set_moments(True)
    between()
    after = ctx.adaptive_status()
    assert (after.rounds, after.active) == (0, 0)
    assert ctx.reproject_status().as_dict() == rp
    return st, ad, rp


@pytest.fixture(scope="module")
def alone(scene_factory):
    """the sequence in a context by itself, and a plain dispatch in a context by itself: what the interleaved case must reproduce"""
    sc, cam = scene_factory("cornell"), layout.make_camera(W, H)
    with fresh(sc, aovs=("normal",), moments=True) as a:
        reads = sequence(a, cam)
    with fresh(sc) as b:
        b.dispatch(cam, FRAMES)
        plain = counters(b.stats())
    return reads, plain


def test_blocks_do_not_bleed(alone):
    (st, ad, rp), _ = alone                     # what each call may touch is asserted in `sequence`
    assert 0 < ad["samples"] and ad["min_count"] <= ad["max_count"] <= ADAPTIVE["max_frames"]


def test_two_contexts_interleaved(scene_factory, alone):
    sc, cam = scene_factory("cornell"), layout.make_camera(W, H)
    reads, plain = alone
    with fresh(sc, aovs=("normal",), moments=True) as a, fresh(sc) as b:
        seen = []

        def between():
            b.dispatch(cam, FRAMES)             # the same frames again: every counter grows by what one dispatch alone gives
            seen.append(counters(b.stats()))
        assert sequence(a, cam, between) == reads
        assert seen == [tuple(k * v for v in plain) for k in range(1, len(seen) + 1)]
