"""Adaptive sampling without a GPU (include/ptmi.h ptmi_dispatch_adaptive): the ABI surface, the selection rule of
tests/adaptive_ref.py on synthetic planes, the model against the oracle's plain renders, its quality at equal budget, and the model's
whole-plane form (run_planes over Oracle.trace_paths) against its per-pixel statement (run over Oracle.trace_path)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["ptmi_dispatch_adaptive", "ptmi_adaptive_status"]

# Quality at equal budget on the 64x64 Cornell box of test_denoise_host._cornell: MSE against the oracle's 1024-spp render of the
# model's adaptive image and of the uniform render with the adaptive run's total samples / pixels, rounded up. Measured with this
# module's model and the oracle, rounds until a round lists nothing (gain = MSE uniform / MSE adaptive):
#   threshold floor neighbourhood min_frames step max_frames -> samples, uniform frames, gain
#   0.05  1.0  0  16 16 4096 ->   112 112   28  1.314   <- the library's defaults (threshold has none)
#   0.08  1.0  0  16 16  512 ->    82 496   21  1.453      0.06  1.0  0   8  8  512 ->    57 336   14  1.653
#   0.05  1.0  0   4  4  512 ->    45 032   11  1.556      0.05  2.5  1   8  8  512 ->    68 352   17  1.256
#   0.10  1.0  1   4  4  512 ->    73 120   18  1.238      0.08  1.0  1  16 16  512 ->   141 696   35  1.203
#   0.10  1.0  1   8  8  256 ->    87 952   22  1.183      0.08  1.0  1   4  4  512 ->   103 772   26  1.162
#   0.10  1.0  1  16 16  512 ->   116 480   29  1.142      0.05  1.0  1  32 16  512 ->   287 200   71  1.121
#   0.08  1.0  1   8  8  512 ->   115 720   29  1.110      0.05  1.0  1  16 16 4096 ->   268 496   66  1.055
#   0.04  1.0  1  16 16  512 ->   368 352   90  1.048      0.03  1.0  1  32 16  512 ->   588 384  144  1.043
#   0.05  1.0  1   8  8  128 ->   235 640   58  1.041      0.05  1.0  1   8  8  256 ->   242 320   60  1.017
#   0.03  1.0  1  16 16  512 ->   579 824  142  1.016      0.05  1.0  1   8  8  512 ->   245 920   61  1.003
#   0.05  1.0  1   4  4  512 ->   230 548   57  0.998      0.02  1.0  1  16 16  512 -> 1 066 576  261  0.994
#   0.02  1.0  1   8  8 1024 -> 1 035 776  253  0.984      0.03  1.0  1   8  8  512 ->   556 568  136  0.973
#   0.05  0.5  1   8  8  512 ->   742 840  182  0.973      0.10  0.3  1   8  8  512 ->   485 984  119  0.972
#   0.05  0.3  1   8  8  512 -> 1 426 000  349  0.952      0.03  1.0  1   4  4  512 ->   546 780  134  0.950
#   0.15  0.2  1   8  8  512 ->   374 576   92  0.924      0.30  0.05 1   8  8  512 ->   225 752   56  0.630
#   0.10  0.1  0   8  8  512 ->   516 432  127  0.350
# The gain is largest while most pixels stop at min_frames and the budget goes to the few that are noisy; it falls towards 1 as the
# threshold tightens and every pixel receives frames in proportion to its variance, and under 1 with a small floor, which spends
# the budget on dark pixels that carry little of the absolute error. neighbourhood = 1 costs MSE per sample (it keeps quiet pixels
# going); it is there against the stopping bias, and stays off by default. The library's default floor (1) follows this
# table. The test runs the library's defaults; its bar is half the measured gain, the rule tests/test_denoise_host.py uses.
K_MEASURED = 1.314
K = K_MEASURED / 2
QUALITY = dict(threshold=0.05)                              # everything else: adaptive_ref.DEFAULTS = the library's defaults


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)


def test_header_library_and_binding(tmp_path):
    h = _header()
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, h), f
    assert re.search(r"struct ptmi_adaptive_params\s*\{", h) and re.search(r"struct ptmi_adaptive_status\s*\{", h)
    assert re.search(r"#define PTMI_ABI_VERSION 4\b", h)
    from ptmi import native
    L = native.load()
    assert L.ptmi_abi_version() == 4
    for f in FUNCS:
        assert hasattr(L, f), f
        assert f in native.EXPORTS
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ptmi_adaptive_params), sizeof(struct ptmi_adaptive_status),\n'
                   '       offsetof(ptmi_adaptive_params, step), offsetof(ptmi_adaptive_params, reserved),\n'
                   '       offsetof(struct ptmi_adaptive_status, samples), offsetof(struct ptmi_adaptive_status, rounds));\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == ctypes.sizeof(native.AdaptiveParams) == 32
    assert got[1] == ctypes.sizeof(native.AdaptiveStatus) == 32
    assert got[2:] == [native.AdaptiveParams.step.offset, native.AdaptiveParams.reserved.offset, native.AdaptiveStatus.samples.offset,
                       native.AdaptiveStatus.rounds.offset]
    assert hasattr(native.Context, "dispatch_adaptive") and hasattr(native.Context, "adaptive_status")
    assert not hasattr(native.MultiContext, "dispatch_adaptive")


def _plane(H, W, m1=0.5, m2=0.25, n=32):
    m = np.zeros((H, W, 4), np.float32)
    m[..., 0], m[..., 1], m[..., 2] = m1, m2, n
    return m


def test_select_rule_on_synthetic_planes():
    p = dict(threshold=0.1, floor=0.05, min_frames=8, max_frames=64, step=4, neighbourhood=0)
    H, W = 6, 7
    quiet = _plane(H, W)                                    # variance 0: converged
    assert not adaptive_ref.select(quiet, p).any()
    m = quiet.copy()
    m[1, 1, 2] = 7                                          # below min_frames: always active, whatever its moments
    m[2, 2, 1] = 0.5                                        # variance 0.25 against a bound of (0.05)^2 * 32: noisy
    m[3, 3, 1], m[3, 3, 2] = 0.5, 64                        # as noisy, but at max_frames: never
    m[4, 4, 0] = np.nan                                     # NaN moments: noisy until max_frames
    m[4, 5, 1] = np.nan
    m[5, 6, :2], m[5, 6, 2] = np.nan, 64
    want = np.zeros((H, W), bool)
    want[1, 1] = want[2, 2] = want[4, 4] = want[4, 5] = True
    assert np.array_equal(adaptive_ref.select(m, p), want)
    # the bound itself: var <= e * e * n converges, the next float above does not
    e = np.float32(0.1) * np.float32(0.5)
    bound = e * e * np.float32(32)
    edge = _plane(1, 2)
    edge[0, 0, 1] = np.float32(0.25) + bound
    edge[0, 1, 1] = np.nextafter(np.float32(0.25) + bound, np.float32(1))
    v = edge[0, :, 1] - np.float32(0.25)
    assert np.array_equal(adaptive_ref.select(edge, p)[0], ~(v <= bound))
    # floor: under it the error is relative to the floor
    dark = _plane(1, 1, m1=0.001, m2=0.0001, n=32)
    assert adaptive_ref.select(dark, dict(p, floor=0.0001))[0, 0] and not adaptive_ref.select(dark, dict(p, floor=1.0))[0, 0]


def test_neighbourhood_stops_at_image_and_band_edges():
    p = dict(threshold=0.1, floor=0.05, min_frames=8, max_frames=64, step=4, neighbourhood=1)
    H, W = 8, 6
    m = _plane(H, W)
    m[0, 0, 1] = 0.5                                        # a noisy corner
    m[4, 5, 1] = 0.5                                        # a noisy pixel on the right edge, row 4
    m[3, 4, 2] = 64                                         # a neighbour at max_frames: not active
    got = adaptive_ref.select(m, p)
    want = np.zeros((H, W), bool)
    want[0:2, 0:2] = True
    want[3:6, 4:6] = True
    want[3, 4] = False
    assert np.array_equal(got, want)
    # rows 4..7 as the band: row 3 is outside, and a noisy pixel outside the band reaches nobody inside
    rows = adaptive_ref.band_rows(H, 4, 8)
    m[3, 1, 1] = 0.5
    got = adaptive_ref.select(m, p, rows)
    want = np.zeros((H, W), bool)
    want[4:6, 4:6] = True
    assert np.array_equal(got, want)
    # interleaved strips of 2 rows, part 1 of 2: rows 2, 3, 6, 7; the noisy pixel of row 4 is not theirs
    rows = adaptive_ref.band_rows(H, 0, 0, 2, 1, 2)
    assert rows.tolist() == [False, False, True, True, False, False, True, True]
    got = adaptive_ref.select(m, p, rows)
    want = np.zeros((H, W), bool)
    want[2:4, 0:3] = True                                   # around (3, 1), inside rows 2..3 only
    assert np.array_equal(got, want)


def test_model_equals_plain_renders_at_each_count(oracle, scene_factory):
    from ptmi import layout
    sc = scene_factory("cornell")
    W, H = 20, 16
    cam = layout.make_camera(W, H)
    p = dict(threshold=0.35, floor=0.05, min_frames=4, max_frames=64, step=4, neighbourhood=1)
    st = adaptive_ref.run(oracle, sc, cam, p, 5)
    counts = st.counts
    assert counts.min() == 4 and counts.max() == 20 and len(np.unique(counts)) >= 3
    for n in np.unique(counts):
        ref, _ = oracle.render(sc, cam, int(n), max_bounces=8, do_mis=1)
        sel = counts == n
        assert np.array_equal(st.image[sel].view(np.uint32), ref[sel].view(np.uint32)), int(n)
    assert st.paths == int(counts.sum()) == adaptive_ref.status(st)["samples"]
    # continuing in two calls is one call
    a = adaptive_ref.run(oracle, sc, cam, p, 2)
    a = adaptive_ref.run(oracle, sc, cam, p, 3, state=a, restart=False)
    assert np.array_equal(a.image.view(np.uint32), st.image.view(np.uint32)) and np.array_equal(a.moments.view(np.uint32), st.moments.view(np.uint32))


def test_quality_at_equal_budget(oracle, scene_factory):
    """MSE of the model's adaptive image against MSE of the uniform render with the same (rounded-up) total samples; see K_MEASURED"""
    from ptmi import layout
    sc = scene_factory("cornell")
    W = H = 64
    cam = layout.make_camera(W, H)
    gt, _ = oracle.render(sc, cam, 1024, max_bounces=8, do_mis=1)
    st = adaptive_ref.run(oracle, sc, cam, QUALITY, 60)
    assert st.active[-1] == 0                               # it stopped by itself
    total = int(st.counts.sum())
    uni, _ = oracle.render(sc, cam, -(-total // (W * H)), max_bounces=8, do_mis=1)

    def mse(a):
        return float(np.mean((a[..., :3].astype(np.float64) - gt[..., :3]) ** 2))

    print("samples", total, "uniform frames", -(-total // (W * H)), "mse adaptive", mse(st.image), "uniform", mse(uni),
          "gain", mse(uni) / mse(st.image))
    assert mse(st.image) * K < mse(uni), (mse(st.image), mse(uni))


# the cases tests/test_gpu_adaptive.py compares with the GPU at 24 x 20 (its P and ROUNDS), here through both forms of the model
P_GPU = dict(threshold=0.35, floor=0.05, min_frames=4, max_frames=64, step=4, neighbourhood=1)
BANDS = [None, dict(tile_y0=5, tile_y1=14), dict(tile_parts=3, tile_part=1, tile_strip=2),
         dict(tile_y0=2, tile_y1=19, tile_parts=2, tile_part=0, tile_strip=3)]


def _same_state(a, b, rows=None):
    assert np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32))
    assert np.array_equal(a.moments.view(np.uint32), b.moments.view(np.uint32))
    assert a.active == b.active and a.paths == b.paths and a.segments == b.segments and a.rounds == b.rounds
    assert adaptive_ref.status(a, rows) == adaptive_ref.status(b, rows)


@pytest.mark.parametrize("name", ["cornell", "feature_box"])
@pytest.mark.parametrize("neighbourhood", [0, 1])
@pytest.mark.parametrize("band", range(len(BANDS)))
def test_run_planes_equals_run(oracle, scene_factory, name, neighbourhood, band):
    from ptmi import layout
    sc = scene_factory(name)
    W, H = 24, 20
    cam = layout.make_camera(W, H)
    p = dict(P_GPU, neighbourhood=neighbourhood)
    t = BANDS[band]
    rows = None if t is None else adaptive_ref.band_rows(H, t.get("tile_y0", 0), t.get("tile_y1", 0), t.get("tile_parts", 1),
                                                         t.get("tile_part", 0), t.get("tile_strip", 1))
    a = adaptive_ref.run(oracle, sc, cam, p, 6, rows=rows)
    b = adaptive_ref.run_planes(oracle, sc, cam, p, 6, rows=rows)
    assert len(set(a.active)) > 1 and 0 < a.active[-1] < a.active[0]          # rounds with lists of their own
    _same_state(a, b, rows)
    # continued without a restart, from a state of the other form's making
    a2 = adaptive_ref.run(oracle, sc, cam, p, 2, rows=rows, state=a, restart=False)
    b2 = adaptive_ref.run_planes(oracle, sc, cam, p, 2, rows=rows, state=b, restart=False)
    _same_state(a2, b2, rows)


@pytest.mark.parametrize("name,dof", [("cornell", False), ("feature_box", True)])
def test_trace_paths_equals_trace_path(oracle, scene_factory, name, dof):
    from ptmi import layout
    sc = scene_factory(name)
    W, H = 257, 131
    cam = layout.make_camera(W, H, aperture=0.05, focus_distance=2.5) if dof else layout.make_camera(W, H)
    rng = np.random.default_rng(20 + dof)
    n = 3000
    xs, ys = rng.integers(0, W, n, dtype=np.uint32), rng.integers(0, H, n, dtype=np.uint32)
    frames = rng.integers(0, 5000, n, dtype=np.uint32)
    for mb, mis in ((8, 1), (3, 0)):
        L, seg = oracle.trace_paths(sc, cam, xs, ys, frames, max_bounces=mb, do_mis=mis)
        assert L.shape == (n, 3) and seg.shape == (n,)
        for i in range(n):
            r, log = oracle.trace_path(sc, cam, int(xs[i]), int(ys[i]), int(frames[i]), max_bounces=mb, do_mis=mis)
            assert np.array_equal(r.view(np.uint32), L[i].view(np.uint32)), i
            assert int((log[:, 15] == 1).sum()) == seg[i], i
        assert 1 <= seg.min() and seg.max() <= mb and len(np.unique(seg)) > 1
        # one thread or all: the same paths
        L1, seg1 = oracle.trace_paths(sc, cam, xs, ys, frames, max_bounces=mb, do_mis=mis, threads=1)
        assert np.array_equal(L1.view(np.uint32), L.view(np.uint32)) and np.array_equal(seg1, seg)
    L0, seg0 = oracle.trace_paths(sc, cam, xs[:0], ys[:0], frames[:0])
    assert L0.shape == (0, 3) and seg0.shape == (0,)
