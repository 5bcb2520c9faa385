"""First-hit planes, sample moments, adaptive rounds and the denoiser over several devices (include/ptmi.h ptmi_multi_set_aovs ...
ptmi_multi_blit_denoised). One GPU stands in for N through PTMI_MULTI_LOOPBACK, as in tests/test_gpu_multi.py; the reference is the
single-device native.Context on the same GPU given the same options and calls - itself pinned against the oracle and the numpy models
by tests/test_gpu_aov.py, test_gpu_adaptive*.py and test_gpu_denoise.py - and every comparison is on the bits.

The N > 1 RCCL legs (the grouped ncclGather of the fused share, the ncclAllGather of the flags) run only in the last test, which skips
itself below two GPUs: they have never run on the machines this suite was written on."""
import ctypes

import numpy as np
import pytest

import adaptive_ref
from ptmi import layout, native, shard
from test_gpu_parity import assert_same_floats, bits

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
AOVS = ("albedo", "normal", "id")
RAGGED = [(2, 64, 48, 0), (3, 80, 50, 0), (8, 40, 67, 3), (5, 33, 4, 1)]       # (n, W, H, strip): the radiance test's ragged frames
# tests/test_gpu_adaptive.py's own parameters
P = dict(threshold=0.35, floor=0.05, min_frames=4, max_frames=64, step=4, neighbourhood=1)
OPT = dict(max_bounces=8, do_mis=1, frames_per_batch=2)


@pytest.fixture(scope="module")
def ctx():
    """the single-device reference: a context of this module's own"""
    c = native.Context(0)
    yield c
    c.close()


def at(W, H, frame):
    return layout.make_camera(W, H, frame_index=frame)


def err(fn, *a, **kw):
    with pytest.raises(native.PtmiError) as e:
        fn(*a, **kw)
    return e.value.code


def single(ctx, sc, W, H, aovs=AOVS, moments=True, **opt):
    ctx.set_aovs()
    ctx.set_moments(False)
    ctx.set_options(**dict(dict(OPT, tile_y0=0, tile_y1=0, tile_parts=0, tile_part=0, tile_strip=0), **opt))
    ctx.upload_scene(sc)
    ctx.resize(W, H)
    ctx.set_aovs(*aovs)
    ctx.set_moments(moments)
    return ctx


def multi(n, sc, W, H, strip=0, aovs=AOVS, moments=True, loopback=True, devices=None, **opt):
    m = native.MultiContext(devices or [0] * n, loopback=loopback)
    m.upload_scene(sc)
    m.resize(W, H)
    m.set_options(**dict(OPT, tile_strip=strip, **opt))
    m.set_aovs(*aovs)
    m.set_moments(moments)
    return m


def planes_of(h, aovs=AOVS, moments=True):
    """every plane of a handle, read through its own read calls (a MultiContext gathers what is stale)"""
    out = {"output": h.read_output()}
    for k in aovs:
        out[k] = h.read_aov(k)
    if moments:
        out["moments"] = h.read_moments()
    return out


def assert_planes(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if k == "id":
            assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), f"{what}: ids"
        else:
            assert_same_floats(got[k], want[k], f"{what}: {k}")


def context_of(m, i, W, H):
    """device i's own context behind a MultiContext, as a Context that does not own its handle (set .h = None before it goes)"""
    c = native.Context.__new__(native.Context)
    c.L, c.h, c.width, c.height = m.L, ctypes.c_void_p(m.L.ptmi_multi_context(m.h, i)), W, H
    return c


def uniform(h, W, H):
    """2 frames, then 1 from frame 2"""
    h.dispatch(at(W, H, 0), 2)
    h.dispatch(at(W, H, 2), 1)


@pytest.mark.parametrize("name,n,W,H,strip", [("cornell",) + s for s in RAGGED] + [("feature_box", 3, 80, 50, 0)])
def test_planes_assemble_the_single_device_planes(ctx, scene_factory, name, n, W, H, strip):
    sc = scene_factory(name)
    uniform(single(ctx, sc, W, H), W, H)
    want = planes_of(ctx)
    assert want["albedo"].any() and want["normal"].any() and want["moments"][..., 2].min() == 3
    with multi(n, sc, W, H, strip) as m:
        assert m.aovs() == AOVS and m.moments()
        uniform(m, W, H)
        assert_planes(planes_of(m), want, f"{name} {W}x{H} from {n} shards")
        assert m.gather_ms() >= 0.0
        # nothing is stale now: a second read gathers nothing and gives the same planes
        assert_planes(planes_of(m), want, "read again")


def test_a_subset_gathers_only_itself(ctx, scene_factory):
    sc = scene_factory("cornell")
    n, W, H = 3, 80, 50
    uniform(single(ctx, sc, W, H), W, H)
    want = planes_of(ctx)
    with multi(n, sc, W, H) as m:
        uniform(m, W, H)
        m.gather_planes("normal", "moments")
        m.gather_planes()                                       # no plane: nothing
        m.synchronize()
        c0 = context_of(m, 0, W, H)
        try:
            own = shard.strip_rows(H, n, 0, m.options().tile_strip)
            others = sorted(set(range(H)) - set(own))
            albedo, ids, out = c0.read_aov("albedo"), c0.read_aov("id"), c0.read_output()
            assert not albedo[others].any() and not ids[others].any() and not out[others].any()
            assert np.array_equal(bits(albedo[own]), bits(want["albedo"][own]))
            assert_same_floats(c0.read_aov("normal"), want["normal"], "NORMAL after a gather of NORMAL | moments")
            assert_same_floats(c0.read_moments(), want["moments"], "moments after a gather of NORMAL | moments")
        finally:
            c0.h = None                                         # owned by the multi handle
        assert_planes(planes_of(m), want, "the rest, gathered by the reads")


@pytest.mark.parametrize("n,W,H,strip", [(3, 80, 50, 0), (5, 33, 4, 1)])      # the second: an odd width, and a device without rows
def test_gather_assembles_the_output_and_nothing_else(ctx, scene_factory, n, W, H, strip):
    """gather() is gather_planes("output"): device 0 then holds the whole output and, of every other plane, its own rows alone"""
    sc = scene_factory("cornell")
    uniform(single(ctx, sc, W, H), W, H)
    want = planes_of(ctx)
    with multi(n, sc, W, H, strip) as m:
        uniform(m, W, H)
        m.gather()
        m.synchronize()
        c0 = context_of(m, 0, W, H)
        try:
            own = shard.strip_rows(H, n, 0, m.options().tile_strip)
            others = sorted(set(range(H)) - set(own))
            assert others
            assert_same_floats(c0.read_output(), want["output"], "the output after gather()")
            for k in AOVS:
                assert not c0.read_aov(k)[others].any(), f"{k} after gather()"
            assert not c0.read_moments()[others].any(), "moments after gather()"
        finally:
            c0.h = None                                         # owned by the multi handle
        assert m.gather_ms() >= 0.0
        assert_planes(planes_of(m), want, "the rest, gathered by the reads")
        m.gather()
        m.gather_planes("output")
        assert np.array_equal(bits(m.read_output()), bits(want["output"])), "the output, gathered again both ways"


def test_resize_with_planes_on_reallocates_the_buffers(ctx, scene_factory):
    sc = scene_factory("cornell")
    with multi(3, sc, 16, 16) as m:
        for W, H in ((64, 48), (128, 48), (40, 48)):
            uniform(single(ctx, sc, W, H), W, H)
            want = planes_of(ctx)
            m.resize(W, H)
            uniform(m, W, H)
            assert_planes(planes_of(m), want, f"{W}x{H} after a resize")
        # a plane turned on later widens the shares: 40x48 with the ids off, then on again
        for aovs in (("normal",), AOVS):
            uniform(single(ctx, sc, 40, 48, aovs=aovs), 40, 48)
            m.set_aovs(*aovs)
            uniform(m, 40, 48)
            assert_planes(planes_of(m, aovs), planes_of(ctx, aovs), f"planes {aovs}")


def adaptive_calls(h, W, H, p, call):
    """5 rounds as calls of 1, 2 and 2; the first restarts"""
    for i, rounds in enumerate((1, 2, 2)):
        call(h)(at(W, H, 0 if i == 0 else 7), rounds, **p)


def dispatch_adaptive_of(h):
    return h.dispatch_adaptive if isinstance(h, native.Context) else h.dispatch_adaptive_rounds


def test_one_device_through_rccl(ctx, scene_factory):
    """a one-rank ncclGather of the fused share and a one-rank ncclAllGather of the flags: the unsharded bits"""
    sc = scene_factory("cornell")
    W, H = 64, 48
    uniform(single(ctx, sc, W, H), W, H)
    want = planes_of(ctx)
    adaptive_calls(ctx, W, H, P, dispatch_adaptive_of)
    want_ad, want_st = planes_of(ctx), ctx.adaptive_status().as_dict()
    with multi(1, sc, W, H, loopback=False) as m:
        uniform(m, W, H)
        m.gather_planes("albedo", "normal", "id", "moments", "output")
        assert_planes(planes_of(m), want, "planes through a one-rank gather")
        adaptive_calls(m, W, H, P, dispatch_adaptive_of)
        assert_planes(planes_of(m), want_ad, "adaptive rounds through a one-rank all-gather")
        assert m.adaptive_status().as_dict() == want_st


@pytest.mark.parametrize("n,W,H,strip,nb", [(2, 64, 48, 4, 1), (3, 40, 26, 4, 1), (8, 40, 67, 3, 1), (3, 40, 26, 4, 0)])
def test_adaptive_rounds_equal_one_devices(ctx, scene_factory, n, W, H, strip, nb):
    sc = scene_factory("cornell")
    p = dict(P, neighbourhood=nb)
    adaptive_calls(single(ctx, sc, W, H), W, H, p, dispatch_adaptive_of)
    want, want_st = planes_of(ctx), ctx.adaptive_status().as_dict()
    print("single device:", want_st)
    # not vacuous: the last round listed some pixels and not all ...
    assert 0 < want_st["active"] < W * H
    if nb:
        # ... and selecting shard by shard - what N plain ptmi_dispatch_adaptive calls would do - is wrong on these inputs: from the
        # moments before the last round (rounds split 1, 2, 1 + 1: a single context's result does not depend on the split)
        single(ctx, sc, W, H)
        for i, rounds in enumerate((1, 2, 1)):
            ctx.dispatch_adaptive(at(W, H, 0 if i == 0 else 7), rounds, **p)
        before = ctx.read_moments()
        whole = adaptive_ref.select(before, p, None)
        by_shard = np.zeros_like(whole)
        for i in range(n):
            by_shard |= adaptive_ref.select(before, p, adaptive_ref.band_rows(H, parts=n, part=i, strip=strip))
        print("active", int(whole.sum()), "of which only through another device's row", int((whole & ~by_shard).sum()))
        assert int(whole.sum()) == want_st["active"] and (whole & ~by_shard).any()
        ctx.dispatch_adaptive(at(W, H, 7), 1, **p)
        assert_planes(planes_of(ctx), want, "the reference, with its last call split")
    with multi(n, sc, W, H, strip) as m:
        adaptive_calls(m, W, H, p, dispatch_adaptive_of)
        assert_planes(planes_of(m), want, f"adaptive rounds over {n} shards, neighbourhood {nb}")
        assert m.adaptive_status().as_dict() == want_st


def test_uniform_frames_then_adaptive_rounds(ctx, scene_factory):
    sc = scene_factory("cornell")
    n, W, H, strip = 3, 40, 26, 4

    def calls(h):
        h.dispatch(at(W, H, 0), 4)
        dispatch_adaptive_of(h)(at(W, H, 4), 3, **P)
    calls(single(ctx, sc, W, H))
    want, want_st = planes_of(ctx), ctx.adaptive_status().as_dict()
    assert 0 < want_st["active"] < W * H and want_st["min_count"] < want_st["max_count"]
    with multi(n, sc, W, H, strip) as m:
        calls(m)
        assert_planes(planes_of(m), want, "4 uniform frames, then 3 adaptive rounds")
        assert m.adaptive_status().as_dict() == want_st


@pytest.mark.parametrize("n,W,H,strip,demodulate", [(2, 64, 48, 0, 0), (8, 40, 67, 3, 0), (2, 64, 48, 0, 1)])
def test_denoise_on_the_assembled_frame(ctx, scene_factory, n, W, H, strip, demodulate):
    sc = scene_factory("cornell")
    aovs = ("albedo", "normal")
    single(ctx, sc, W, H, aovs=aovs).dispatch(at(W, H, 0), 8)
    want = ctx.denoise(demodulate=demodulate)
    want_f, want_b = ctx.blit_denoised()
    assert want[..., :3].any()
    with multi(n, sc, W, H, strip, aovs=aovs) as m:
        m.dispatch(at(W, H, 0), 8)
        assert_same_floats(m.denoise(demodulate=demodulate), want, f"denoised frame of {n} shards")
        f, b = m.blit_denoised()
        assert_same_floats(f, want_f, "float canvas")
        assert np.array_equal(b, want_b)


def test_errors_are_loud_and_leave_the_state(ctx, scene_factory):
    sc = scene_factory("cornell")
    n, W, H = 2, 64, 48
    uniform(single(ctx, sc, W, H), W, H)
    want = planes_of(ctx)
    cam = at(W, H, 0)
    with multi(n, sc, W, H, aovs=(), moments=False) as m:
        def still_renders():
            m.set_aovs(*AOVS)
            m.set_moments(True)
            uniform(m, W, H)
            assert_planes(planes_of(m), want, "a render after the error")

        assert err(m.dispatch_adaptive_rounds, cam, 1, **P) == E_STATE                   # moments off
        assert err(m.read_moments) == E_STATE
        still_renders()
        m.set_aovs("albedo")
        assert err(m.denoise) == E_STATE                                                 # NORMAL off
        assert err(m.gather_planes, "normal") == E_STATE and err(m.gather_planes, native.AOV_ID) == E_STATE
        assert err(m.read_aov, "normal") == E_STATE
        assert err(m.gather_planes, 8) == E_INVALID and err(m.gather_planes, 0x400) == E_INVALID
        assert err(m.set_aovs, 8) == E_INVALID and m.aovs() == ("albedo",)
        still_renders()
        m.set_moments(False)
        assert err(m.gather_planes, "moments") == E_STATE and err(m.denoise) == E_STATE
        still_renders()
        for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(reserved=(0, 1)), dict(reserved=(2, 0)),
                    dict(min_frames=9, max_frames=8), dict(max_frames=(1 << 24) + 1), dict(neighbourhood=2), dict(floor=-1.0)):
            assert err(m.dispatch_adaptive_rounds, cam, 1, **dict(P, **bad)) == E_INVALID, bad
        assert err(m.dispatch_adaptive_rounds, at(W + 1, H, 0), 1, **P) == E_INVALID
        still_renders()


def test_two_devices_over_rccl(ctx, scene_factory):
    """The real N > 1 legs: one grouped ncclGather of the fused share, the ncclAllGather of the flags, the denoiser behind them.
    Skipped on a one-GPU box, like tests/test_gpu_multi.py's two-device test."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the N > 1 RCCL legs have never run)")
    sc = scene_factory("cornell")
    W, H = 96, 70
    s = single(ctx, sc, W, H)
    uniform(s, W, H)
    want = planes_of(ctx)
    ctx.dispatch_adaptive(at(W, H, 0), 3, **P)
    want_ad, want_st, want_dn = planes_of(ctx), ctx.adaptive_status().as_dict(), ctx.denoise()
    with multi(2, sc, W, H, loopback=False, devices=[0, 1]) as m:
        uniform(m, W, H)
        assert_planes(planes_of(m), want, "planes gathered from two devices over RCCL")
        m.dispatch_adaptive_rounds(at(W, H, 0), 3, **P)
        assert_planes(planes_of(m), want_ad, "adaptive rounds over two devices")
        assert m.adaptive_status().as_dict() == want_st
        assert_same_floats(m.denoise(), want_dn, "denoised over two devices")
