"""The frame scissor behind a multi-device handle (include/ptmi.h ptmi_multi_*): every device's context works out
the rectangle for its own rows, and a shard whose rows lie wholly above or below it traces nothing. Three loopback shards on one device,
twice: the second handle created under PTMI_SCISSOR=0 (tests/scissor_pair.py). The gathered frames must be equal bit for bit and the
summed statistics equal, and both equal to one scissored Context that renders the whole frame. There is no ptmi_multi_scissor_status,
so no status is asserted here.

Cornell, 96 x 54, the far camera (rows 19 .. 34), 4 frames: with the automatic strip height the strips interleave through the
rectangle; with strips of 18 rows the first and the last shard own no row of it."""
import numpy as np
import pytest

from ptmi import layout, native, scenes, shard
from scissor_pair import H, W, bits, counters, make_pair, render

pytestmark = pytest.mark.gpu

FRAMES, N = 4, 3
OPTIONS = dict(max_bounces=3, do_mis=1, frames_per_batch=2)


@pytest.fixture(scope="module")
def whole():
    """(frame, counters, status) of one scissored context that renders every row"""
    with native.Context(0) as ctx:
        return render(ctx, scenes.make("cornell"), layout.make_camera(W, H, position=(0.07, 1.0, 9.0)), frames=FRAMES, **OPTIONS)


@pytest.mark.parametrize("strip", (0, 18))
def test_loopback_shards_with_and_without_the_scissor(whole, strip):
    scene = scenes.make("cornell")
    cam = layout.make_camera(W, H, position=(0.07, 1.0, 9.0))
    ref, ref_counters, st = whole
    assert st["applied"] == 1 and (st["y0"], st["y1"]) == (19, 35)
    rows = strip or shard.strip_rows_for(H, N)
    owners = {(y // rows) % N for y in range(st["y0"], st["y1"])}
    assert owners == ({1} if strip == 18 else {0, 1, 2})        # 18 rows: shards 0 and 2 lie wholly outside the rectangle
    on, off = make_pair(lambda: native.MultiContext([0] * N, loopback=True))
    try:
        got = []
        for m in (on, off):
            m.upload_scene(scene)
            m.resize(W, H)
            m.set_options(tile_strip=strip, **OPTIONS)
            assert m.options().tile_parts == N and m.options().tile_strip == rows
            m.reset_stats()
            m.dispatch(cam, FRAMES)
            m.gather()
            got.append((m.read_output(), counters(m)))
    finally:
        on.close()
        off.close()
    (a, ca), (b, cb) = got
    assert ca == cb, (ca, cb)
    assert np.array_equal(bits(a), bits(b)), np.argwhere((bits(a) != bits(b)).any(-1))[:8]
    assert ca[:4] == ref_counters[:4], (ca, ref_counters)      # paths, segments, segments by bounce, shadow rays: summed over the shards
    assert np.array_equal(bits(a), bits(ref)), np.argwhere((bits(a) != bits(ref)).any(-1))[:8]
    assert a[..., :3].max() > 0.0
