"""Adaptive sampling, the plane folds and the denoiser on frames of many tiles (include/ptmi.h ptmi_dispatch_adaptive, ptmi_set_aovs,
ptmi_set_moments, ptmi_denoise). tests/test_gpu_adaptive.py, test_gpu_aov.py and test_gpu_denoise.py compare with their models on
thumbnails, where the list build of a round (csrc/pipeline.hip k_ad_select -> k_ad_tile_sums -> k_ad_scatter) is one quarter-empty
tile of 1 024 ballot words = 65 536 pixels. Here:

  1. one round under synthetic moments planes that list exactly the pixels the test names, on bands of 1 to 32 tiles with full and
     ragged last words: every listed pixel holds the plain render of its own count afterwards, every other pixel its bits;
  2. natural rounds at 1920 x 1080 and 1921 x 1080, round by round against adaptive_ref.select, however they are cut into rounds
     and batches (an automatic batch below `step` included);
  3. adaptive_ref.run_planes, and the moments and first-hit folds of a plain dispatch, against the oracle above one tile;
  4. the denoiser against denoise_ref.denoise on whole 1080p frames.

Everything is bit for bit, except the denoiser (test_gpu_denoise.close_to_ref) and the first-hit planes against tests/aov_ref.py
(test_gpu_aov's own tolerances, imported)."""
import ctypes
import time

import numpy as np
import pytest

import adaptive_ref
import aov_ref
import denoise_ref
from ptmi import layout, native
from test_gpu_adaptive import P, ROUNDS, at, check_partly_converged, setup, write_moments
from test_gpu_aov import check_one_frame
from test_gpu_denoise import close_to_ref, per_path_rows

pytestmark = pytest.mark.gpu

ALL = ("albedo", "normal", "id")
TILE = 65536                                                # pixels per tile of the list build: 1 024 ballot words x 64


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: the planes and options it sets never reach the session's shared context"""
    c = native.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def write_plane(ctx, name, plane):
    """the caller's way to write a first-hit plane: a copy to ptmi_aov_device_ptr (as test_gpu_adaptive.write_moments)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    plane = np.ascontiguousarray(plane, native.AOVS[name][1])
    assert plane.shape == (ctx.height, ctx.width, native.AOVS[name][2])
    ctx.synchronize()
    assert hip.hipMemcpy(ctx.aov_device_ptr(name), plane.ctypes.data, plane.nbytes, 1) == 0             # host to device


def band_of(H, tile):
    return adaptive_ref.band_rows(H, tile.get("tile_y0", 0), tile.get("tile_y1", 0), tile.get("tile_parts", 1), tile.get("tile_part", 0),
                                  tile.get("tile_strip", 1))


def assert_same(got, want, what, rows, W, only=None):
    """got == want bit for bit on the band's rows (`only`: a (rows, W) mask of the band pixels compared); the message names the first
    pixel that differs by its band-local index (what a list entry is), its tile and word, and its place in the frame"""
    g, w = bits(got)[rows], bits(want)[rows]
    bad = (g != w).reshape(g.shape[0], W, -1).any(axis=-1)
    if only is not None:
        bad &= only
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        y = int(np.flatnonzero(rows)[i // W])
        raise AssertionError(f"{what}: {int(bad.sum())} band pixels differ, first at band index {i} (tile {i // TILE}, word {i // 64}, "
                             f"bit {i % 64}) = frame pixel (x {i % W}, y {y}): got {got[y, i % W]}, want {want[y, i % W]}")


def read_planes(ctx):
    d = dict(image=ctx.read_output(), moments=ctx.read_moments())
    d.update({k: ctx.read_aov(k) for k in ALL})
    return d


def plain_renders(ctx, cam, counts):
    """{n: the five planes after a plain dispatch of frames 0 .. n - 1} on the context as it is set up"""
    out = {}
    for n in counts:
        ctx.dispatch(at(cam, 0), int(n))
        out[int(n)] = read_planes(ctx)
    return out


def at_counts(counts, by_n, key):
    return adaptive_ref.planes_at_counts(counts, {n: v[key] for n, v in by_n.items()})


# 1 -----------------------------------------------------------------------------------------------------------------------------------
# neighbourhood 0 and m1 = m2 = 0 (variance 0 under any bound): a pixel is listed iff its count is under min_frames. Listed pixels
# are at 0, 3 or 7 frames, the others at 8; one round of step 2 takes the listed ones to 2, 5 or 9.
SYN = dict(threshold=0.5, floor=0.05, min_frames=8, max_frames=64, step=2, neighbourhood=0)
Z_LISTED, Z_OTHER = (0, 3, 7), 8
SENTINEL = np.float32(12345678.0)                          # bits 0x4B3C614E: no render writes it
SENTINEL_ID = np.uint32(0xABCD1234)

# name: (W, H, tile options, band pixels, tiles, ballot words of the last tile, bits of the last word)
SIZES = {
    "256x256": (256, 256, {}, 65536, 1, 1024, 64),
    "257x255": (257, 255, {}, 65535, 1, 1024, 63),
    "260x253": (260, 253, {}, 65780, 2, 4, 52),
    "512x257": (512, 257, {}, 131584, 3, 8, 64),
    "1920x1080": (1920, 1080, {}, 2073600, 32, 656, 64),
    "1921x1080": (1921, 1080, {}, 2074680, 32, 673, 56),
    "1920x1080/part1of4": (1920, 1080, dict(tile_parts=4, tile_part=1, tile_strip=3), 518400, 8, 932, 64),
}
PATTERNS = ("all", "none", "first", "last", "tile_ends", "hole", "last_word", "half", "sparse")


def pattern(name, npix, seed):
    """(npix,) bool over band-local pixel indices; asserts the property it is named for"""
    nwords = -(-npix // 64)
    ntiles = -(-nwords // 1024)
    tile_of = np.arange(npix) // TILE
    m = np.zeros(npix, bool)
    rng = np.random.default_rng(seed)
    if name == "all":
        m[:] = True
    elif name == "none":
        assert not m.any()
    elif name == "first":
        m[0] = True
        assert m.sum() == 1
    elif name == "last":
        m[npix - 1] = True
        assert m.sum() == 1 and (ntiles == 1 or np.flatnonzero(m)[0] >= 1 << 16)
    elif name == "tile_ends":
        for t in range(ntiles):
            m[t * TILE] = m[min((t + 1) * TILE, npix) - 1] = True
        assert m.sum() == 2 * ntiles and len(np.unique(tile_of[m])) == ntiles
        assert ntiles == 1 or np.flatnonzero(m).max() >= 1 << 16
    elif name == "hole":
        assert ntiles >= 3
        m[:] = True
        m[tile_of == ntiles // 2] = False
        per_tile = np.bincount(tile_of[m], minlength=ntiles)
        assert per_tile[ntiles // 2] == 0 and (np.delete(per_tile, ntiles // 2) > 0).all()          # an empty tile between full ones
    elif name == "last_word":
        m[(nwords - 1) * 64:] = True
        assert m.sum() == npix - (nwords - 1) * 64 > 0 and not m[:(nwords - 1) * 64].any()
    elif name == "half":
        m = rng.random(npix) < 0.5
        assert (np.bincount(tile_of[m], minlength=ntiles) > 0).all() and 0.45 < m.mean() < 0.55
    elif name == "sparse":
        m = rng.random(npix) < 1e-3
        for t in range(ntiles):                                             # ... and one in every tile, however short the last is
            m[rng.integers(t * TILE, min((t + 1) * TILE, npix))] = True
        words = np.bincount(np.flatnonzero(m) // 64, minlength=nwords)
        assert m.any() and (words == 0).mean() > 0.9                        # most words zero
        assert ntiles == 1 or len(np.unique(tile_of[m])) >= 2
    if m.any() and ntiles >= 2 and name not in ("first", "last_word"):
        assert np.flatnonzero(m).max() >= 1 << 16                           # a list entry that needs more than 16 bits
    return m


_plain = {}


def plain_cached(ctx, key, cam):
    """the plain renders of one set-up: kept for the patterns that follow on the same size (one size at a time)"""
    if key not in _plain:
        _plain.clear()
        _plain[key] = plain_renders(ctx, cam, (2, 3, 5, 7, 9))
    return _plain[key]


def one_synthetic_round(ctx, cam, rows, listed, z, plain):
    """presets every plane, runs one round, returns the planes, the stats and the status"""
    H, W = listed.shape
    zf = np.where(listed, z, Z_OTHER)
    # a listed pixel: the plain render of its z frames (z = 0: the sentinel too, frame 0 overwrites); an unlisted one: the sentinel
    before = dict(image=np.full((H, W, 4), SENTINEL, np.float32), albedo=np.full((H, W, 4), SENTINEL, np.float32),
                  normal=np.full((H, W, 4), SENTINEL, np.float32), id=np.full((H, W, 2), SENTINEL_ID, np.uint32))
    for n in Z_LISTED[1:]:
        sel = listed & (z == n)
        for k in before:
            before[k][sel] = plain[n][k][sel]
    mom = np.zeros((H, W, 4), np.float32)
    mom[..., 2] = zf
    ctx.write_output(before["image"])
    for k in ALL:
        write_plane(ctx, k, before[k])
    write_moments(ctx, mom)
    before["moments"] = mom
    ctx.reset_stats()
    ctx.dispatch_adaptive(at(cam, 7), 1, **SYN)                               # frame_index != 0: nothing restarts
    return before, read_planes(ctx), ctx.stats(), ctx.adaptive_status()


def check_synthetic(ctx, sc, size, pat, scene_opts, key):
    W, H, tile, npix, ntiles, last_tile_words, last_word_bits = SIZES[size]
    rows = band_of(H, tile)
    nwords = -(-npix // 64)
    # the table's facts about the size
    assert rows.sum() * W == npix and -(-nwords // 1024) == ntiles and nwords - (ntiles - 1) * 1024 == last_tile_words
    assert npix - (nwords - 1) * 64 == last_word_bits
    flat = pattern(pat, npix, seed=len(size) * 131 + PATTERNS.index(pat))
    listed = np.zeros((H, W), bool)
    listed[rows] = flat.reshape(-1, W)
    z = np.random.default_rng(7).choice(np.array(Z_LISTED, np.uint32), size=(H, W))
    if flat.sum() >= 3:                                                     # every start count occurs among the listed pixels
        z[tuple(np.argwhere(listed)[:3].T)] = Z_LISTED
        assert set(np.unique(z[listed]).tolist()) == set(Z_LISTED)
    n_listed = int(flat.sum())
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, aovs=ALL, max_bounces=2, **scene_opts, **tile)
    plain = plain_cached(ctx, key, cam)
    before, got, st, ast = one_synthetic_round(ctx, cam, rows, listed, z, plain)
    counts = np.where(listed, z + 2, Z_OTHER).astype(np.uint32)
    only = listed[rows]
    # listed pixels: the plain render of z + 2 frames
    for k in ("image", "albedo", "normal", "id"):
        assert_same(got[k], at_counts(np.where(listed, counts, 0), plain, k), f"{k} at listed pixels", rows, W, only)
    fresh = (listed & (z == 0))[rows]
    assert_same(got["moments"], plain[2]["moments"], "moments where frame 0 overwrote", rows, W, fresh)
    # every other pixel of the band, and every row of other parts: untouched
    for k in ("image", "albedo", "normal", "id", "moments"):
        assert_same(got[k], before[k], f"{k} at unlisted pixels", rows, W, ~only)
        assert np.array_equal(bits(got[k])[~rows], bits(before[k])[~rows]), f"{k}: rows outside the band were written"
    want_z = np.zeros((H, W, 1), np.float32)
    want_z[..., 0] = np.where(rows[:, None], counts, Z_OTHER)
    assert_same(got["moments"][..., 2:3], want_z, "moments.z", rows, W)
    assert not got["moments"][..., 3].any()
    # counters
    c = counts[rows].astype(np.uint64)
    assert ast.active == n_listed, f"active {ast.active}, listed {n_listed} in {ntiles} tiles"
    assert st.paths == 2 * n_listed
    assert (ast.samples, ast.min_count, ast.max_count) == (int(c.sum()), int(c.min()), int(c.max()))
    if n_listed == 0:
        assert st.segments == 0
    # ... and a second, identical run
    _, again, st2, ast2 = one_synthetic_round(ctx, cam, rows, listed, z, plain)
    assert st2.segments == st.segments and st2.paths == st.paths
    assert dict(ast2.as_dict(), rounds=0) == dict(ast.as_dict(), rounds=0)
    for k in got:
        assert_same(again[k], got[k], f"{k}, second run", rows, W)
    return st


@pytest.mark.parametrize("size,pat", [(s, p) for s in SIZES for p in PATTERNS if p != "hole" or SIZES[s][4] >= 3])     # a hole: three tiles
def test_one_round_lists_exactly_the_named_pixels(ctx, scene_factory, size, pat):
    check_synthetic(ctx, scene_factory("cornell"), size, pat, dict(traversal=native.TRAVERSAL_AUTO), ("cornell", size))


def test_listed_folds_with_the_16_byte_radiance_stride(ctx, scene_factory):
    """cornell_spheres walked from memory: the per-path radiance is a float4 (DevPaths::l_stride == 4) under the listed folds"""
    st = check_synthetic(ctx, scene_factory("cornell_spheres"), "1920x1080", "half", dict(traversal=native.TRAVERSAL_GLOBAL),
                         ("cornell_spheres", "1920x1080"))
    assert st.radiance_stride_bytes == 16 and st.traversal_used == native.TRAVERSAL_GLOBAL
    ctx.set_options(traversal=native.TRAVERSAL_AUTO)
    _plain.clear()


# 2 -----------------------------------------------------------------------------------------------------------------------------------
# test_gpu_adaptive.P at 1080p. A pixel's moments at count n are the plain render's of n frames, so the shares can be had from plain
# dispatches alone: the test prints them (simulated_shares) before it asserts on the planes it read back.
def simulated_shares(plain, p, rounds):
    """the rule run in numpy on plain-dispatch moments: (converged share after `rounds` rounds, list lengths)"""
    ns = sorted(plain)
    counts = np.zeros(plain[ns[0]]["moments"].shape[:2], np.uint32)
    active = []
    for _ in range(rounds):
        mom = at_counts(counts, plain, "moments")
        act = adaptive_ref.select(mom, p)
        active.append(int(act.sum()))
        counts = counts + np.where(act, np.uint32(p["step"]), np.uint32(0))
    mom = at_counts(counts, plain, "moments")
    return 1.0 - adaptive_ref.select(mom, p).mean(), active


def rounds_one_by_one(ctx, cam, p, rounds):
    """each round a dispatch of its own, checked against adaptive_ref.select on the moments read back before it"""
    H, W = int(cam["height"]), int(cam["width"])
    rows = np.ones(H, bool)
    active = []
    for r in range(rounds):
        before = ctx.read_moments()
        if r == 0:
            before[..., 2] = 0                                              # frame_index 0 restarts
        paths = ctx.stats().paths
        ctx.dispatch_adaptive(at(cam, 0 if r == 0 else 7), 1, **p)
        after = ctx.read_moments()
        want = adaptive_ref.select(before, p)
        want_z = before[..., 2:3] + np.where(want, np.float32(p["step"]), np.float32(0))[..., None]
        assert_same(after[..., 2:3], want_z, f"round {r}: the counts that advanced", rows, W)
        assert ctx.adaptive_status().active == int(want.sum()), r
        assert ctx.stats().paths - paths == int(want.sum()) * p["step"], r
        active.append(int(want.sum()))
    return active


@pytest.mark.parametrize("W,H", [(1920, 1080), (1921, 1080)])
def test_natural_rounds_at_full_size(ctx, scene_factory, W, H):
    sc = scene_factory("cornell")
    cam = layout.make_camera(W, H)
    rows = np.ones(H, bool)
    setup(ctx, sc, W, H, aovs=ALL)
    active = rounds_one_by_one(ctx, cam, P, ROUNDS)
    got, st, ast = read_planes(ctx), ctx.stats(), ctx.adaptive_status()
    counts = got["moments"][..., 2].astype(np.uint32)
    assert ast.rounds == ROUNDS and st.paths == int(counts.sum(dtype=np.uint64)) == ast.samples
    # partly converged (test_gpu_adaptive.check_partly_converged on the planes read back)
    state = adaptive_ref.State(H, W, got["image"], got["moments"])
    state.active = active
    check_partly_converged(state, P)
    # every plane at every pixel: the plain render of its own count
    plain = plain_renders(ctx, cam, sorted(set(counts.ravel().tolist())))
    print("simulated on plain renders", simulated_shares(plain, P, ROUNDS))
    for k in got:
        assert_same(got[k], at_counts(counts, plain, k), f"{k} against plain renders of each pixel's count", rows, W)
    del plain
    # the same six rounds as one dispatch, and in batches of 3 + 1 frames
    for fpb in (0, 3):
        setup(ctx, sc, W, H, aovs=ALL, frames_per_batch=fpb)
        ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **P)
        again = read_planes(ctx)
        if fpb:
            assert ctx.stats().frames_per_batch_used == 3 < P["step"]
        for k in got:
            assert_same(again[k], got[k], f"{k}, one dispatch of {ROUNDS} rounds, frames_per_batch {fpb}", rows, W)
        assert ctx.stats().segments == st.segments and ctx.stats().paths == st.paths
        assert ctx.adaptive_status().as_dict() == ast.as_dict()


def test_automatic_batch_below_step(ctx, scene_factory):
    """dispatch()'s automatic batch size with all planes on, under a step above it: the rounds are cut into batches by the library, and
    the listed pixels' counts move on between the batches of one round"""
    sc = scene_factory("cornell")
    W, H = 1920, 1080
    setup(ctx, sc, W, H, aovs=ALL)
    ctx.dispatch(at(layout.make_camera(W, H), 0), 64)
    auto = ctx.stats().frames_per_batch_used
    if auto >= 64:
        W, H = 3840, 2160                                   # tests/test_gpu_full_size.py sees 16 here without the planes
        setup(ctx, sc, W, H, aovs=ALL)
        ctx.dispatch(at(layout.make_camera(W, H), 0), 64)
        auto = ctx.stats().frames_per_batch_used
    print("automatic frames_per_batch", auto, "at", W, H)
    assert auto < 64
    cam = layout.make_camera(W, H)
    rows = np.ones(H, bool)
    p = dict(P, step=auto + 3, min_frames=auto + 3, max_frames=4 * (auto + 3))
    outs = []
    for fpb in (0, auto + 3):
        setup(ctx, sc, W, H, aovs=ALL, frames_per_batch=fpb)
        ctx.dispatch_adaptive(at(cam, 0), 2, **p)
        outs.append((read_planes(ctx), ctx.stats().segments, ctx.stats().paths, ctx.adaptive_status().as_dict(),
                     ctx.stats().frames_per_batch_used))
    assert outs[0][4] == auto < p["step"] and outs[1][4] == p["step"]
    c = outs[1][0]["moments"][..., 2]
    assert c.min() == p["step"] and c.max() == 2 * p["step"]                # the second round listed some pixels, not all
    for k in outs[0][0]:
        assert_same(outs[0][0][k], outs[1][0][k], f"{k}: automatic batches of {auto} against one batch per round", rows, W)
    assert outs[0][1:4] == outs[1][1:4]
    ctx.resize(16, 16)                                      # give the large batch back


# 3 -----------------------------------------------------------------------------------------------------------------------------------
_model = {}


def model(oracle, sc, name, cam, band):
    key = (name, tuple(sorted(band.items())))
    if key not in _model:
        rows = band_of(int(cam["height"]), band) if band else None
        _model[key] = (adaptive_ref.run_planes(oracle, sc, cam, P, ROUNDS, rows=rows), rows)
    return _model[key]


BAND = dict(tile_y0=2, tile_y1=251, tile_parts=2, tile_part=0, tile_strip=3)


@pytest.mark.parametrize("name,leaves,band", [("cornell", 1, {}), ("cornell", 2, {}), ("feature_box", 1, {}), ("feature_box", 2, {}),
                                               ("cornell", 2, BAND)])
def test_two_tiles_match_the_model(ctx, oracle, scene_factory, name, leaves, band):
    sc = scene_factory(name)
    W, H = 260, 253
    cam = layout.make_camera(W, H)
    want, rows = model(oracle, sc, name, cam, band)
    check_partly_converged(want, P, rows)
    assert want.active[0] > TILE or band                                    # lists of more than one tile
    setup(ctx, sc, W, H, leaves=leaves, **band)
    ctx.dispatch_adaptive(at(cam, 0), ROUNDS, **P)
    got, mom, st, ast = ctx.read_output(), ctx.read_moments(), ctx.stats(), ctx.adaptive_status()
    every = np.ones(H, bool)
    assert_same(mom, want.moments, "moments against the model", every, W)
    assert_same(got, want.image, "radiance against the model", every, W)
    assert st.segments == want.segments and st.paths == want.paths and st.dispatches == 1
    assert ast.as_dict() == adaptive_ref.status(want, rows)


ROWS_1080 = np.array([0, 1, 539, 540, 1078, 1079], np.uint32)              # rows (0, 2), (539, 541), (1078, 1080)


@pytest.mark.parametrize("name", ["cornell", "feature_box"])
def test_plain_folds_at_1080p_against_the_oracle(ctx, oracle, scene_factory, name):
    """the moments and first-hit folds of a plain dispatch of 7 frames at 1920 x 1080 (batches of 3, two dispatches), on six rows"""
    sc = scene_factory(name)
    W, H = 1920, 1080
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, aovs=ALL, frames_per_batch=3)
    ctx.dispatch(at(cam, 0), 1)
    s0 = aov_ref.samples(oracle, sc, cam, 0, rows=ROWS_1080)
    n_hit, _ = check_one_frame(sc, s0, {k: ctx.read_aov(k)[ROWS_1080] for k in ALL}, W, len(ROWS_1080))
    assert n_hit > 0.1 * W * len(ROWS_1080)                                 # the box fills the middle rows of a 16:9 frame only
    ctx.dispatch(at(cam, 0), 4)
    ctx.dispatch(at(cam, 4), 3)
    assert ctx.stats().frames_per_batch_used == 3
    # moments
    got = ctx.read_moments()
    want = denoise_ref.fold_moments(per_path_rows(oracle, sc, cam, range(7), rows=ROWS_1080), list(range(7)))
    sel = np.zeros(H, bool)
    sel[ROWS_1080] = True
    full = np.zeros((H, W, 4), np.float32)
    full[sel] = want.reshape(len(ROWS_1080), W, 4)
    assert_same(got, full, "moments against the oracle's per-path radiance", sel, W)
    assert (got[..., 2] == 7).all() and not got[..., 3].any()
    # first-hit planes: the bars written above test_gpu_aov.test_many_frames_fold
    per = [s0] + [aov_ref.samples(oracle, sc, cam, f, rows=ROWS_1080) for f in range(1, 7)]
    ra, rn, rid, exact = aov_ref.fold(per, list(range(7)))
    assert exact.mean() > 0.9
    a, n = ctx.read_aov("albedo")[ROWS_1080].reshape(-1, 4), ctx.read_aov("normal")[ROWS_1080].reshape(-1, 4)
    assert np.array_equal(ctx.read_aov("id")[ROWS_1080].reshape(-1, 2), rid), "ID is not the last frame's"
    assert np.abs(a[exact] - ra[exact]).max() < 1e-6
    t_err = np.abs(n[:, 3] - rn[:, 3]) / np.maximum(np.abs(rn[:, 3]), 1e-30)
    assert t_err[exact & (rn[:, 3] != 0)].max() < 1e-6 and (n[rn[:, 3] == 0, 3] == 0).all()
    mapped = np.zeros(len(a), bool)
    for s in per:
        mapped |= s["normal_mapped"]
    assert np.abs(n[exact & ~mapped, :3] - rn[exact & ~mapped, :3]).max() < 1e-5
    assert np.abs(n[exact & mapped, :3] - rn[exact & mapped, :3]).max(initial=0) < 2e-4


# 4 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1920, 1080), (1921, 1083)])
@pytest.mark.parametrize("dm", [1, 2])
def test_denoiser_at_full_size(ctx, scene_factory, W, H, dm):
    """ptmi_denoise on whole frames: pixels whose 25 taps at step 16 all lie inside, a grid of many 64-pixel block columns, an odd
    width. tests/denoise_ref.py takes 2 s (1 iteration) and 10 - 12 s (5 iterations) for one 1920 x 1080 frame on the GPU host
    (8 s and 38 s on an 8-thread build host): under the minute, so the frames are compared whole."""
    assert W > 64 and H > 64                                # some pixel has every tap at offsets up to 2 * 16 inside
    sc = scene_factory("cornell_spheres")
    cam = layout.make_camera(W, H)
    setup(ctx, sc, W, H, aovs=("albedo", "normal"))
    ctx.dispatch(at(cam, 0), 6)
    rad, nrm, alb, mom = ctx.read_output(), ctx.read_aov("normal"), ctx.read_aov("albedo"), ctx.read_moments()
    for it in (1, 5):
        t0 = time.time()
        got = ctx.denoise(iterations=it, demodulate=dm)
        ref = denoise_ref.denoise(rad, nrm, alb, mom, iterations=it, demodulate=dm == 2)
        print("denoise_ref", W, H, "iterations", it, "seconds", round(time.time() - t0, 1))
        close_to_ref(got, ref)
    ctx.resize(16, 16)
