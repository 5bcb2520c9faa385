"""The own-leaf hierarchy built on the GPU (ptmi_options.leaves = 2, tree_builder = 2; csrc/own_tree_gpu.hip), through the C ABI.

Any topology over conservative padded boxes gives the reference traversal's results, so the device tree
must: be reported (ptmi_stats.tree_builder_used), be a sound image (every listed triangle once, boxes holding their triangles with
the padding to spare, the quantised planes holding the padded boxes), share with the host build what depends on the triangle set
only (pad, safe origin, root box, leaf boxes) bit for bit, be the same bytes on every upload, replay on the CPU exactly as the
reference traversal, cost about as much per ray as the host tree, and give the oracle's hits, shadow predicates and frames on the GPU."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from ptmi import layout, native, scenes
from test_gpu_parity import assert_same_floats, bits
from test_gpu_own_leaves import more_rays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import own_leaf_gate as gate            # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEAF = 0x80000000
_cache = {}


def scene(name):
    if name not in _cache:
        if name == "grid96":
            _cache[name] = scenes.grid_1m(n=96)                         # the 1 M-triangle scene's construction at 18 050 triangles
        elif name == "grid48":
            _cache[name] = scenes.grid_1m(n=48)                         # ... at a few thousand, above the 4 096 the host keeps
        elif name == "soup20k":
            _cache[name] = scenes.random_soup(5, n_tris=20000)
        elif name == "deep3":                                           # 3 000 triangles, an uploaded BVH of 60 levels
            parts = []
            for c in range(3):
                t = scenes.deep_chain(n=1000).tris.copy()
                for k in ("v0", "v1", "v2"):
                    t[k][:, 1] += np.float32(c * 1e-3)
                parts.append(t)
            base = scenes.deep_chain(n=1000)
            _cache[name] = scenes._finish("deep3", parts, list(base.mats))
        else:
            _cache[name] = scenes.make(name)
    return _cache[name]


@pytest.fixture()
def ctx(gpu_ctx):
    before = gpu_ctx.options()
    gpu_ctx.set_options(leaves=2, leaf_tris=0, keep_reference_tree=0, tree_builder=2, traversal=native.TRAVERSAL_AUTO, cull=1)
    yield gpu_ctx
    gpu_ctx.set_options(leaves=before.leaves, leaf_tris=before.leaf_tris, keep_reference_tree=0, tree_builder=before.tree_builder,
                        traversal=native.TRAVERSAL_AUTO, cull=1, max_bounces=8, do_mis=1, frames_per_batch=0, tile_y0=0, tile_y1=0)


def upload(ctx, sc, builder, leaf_tris=0, leaves=2):
    ctx.set_options(tree_builder=builder, leaf_tris=leaf_tris, leaves=leaves)
    ctx.upload_scene(sc)
    return ctx.stats()


def info_bytes(info):
    return ctypes.string_at(ctypes.addressof(info), ctypes.sizeof(info))


def same_arrays(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and
                                         np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


# -- 1. the option is honoured ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid48", "grid96", "soup20k", "grid_1m"])
def test_device_builds_the_own_tree(ctx, name):
    st = upload(ctx, scene(name), 2)
    assert (st.tree_builder_used, st.leaves_used) == (2, 2), name
    st = upload(ctx, scene(name), 1)
    assert (st.tree_builder_used, st.leaves_used) == (1, 2), name


def test_small_scenes_and_bad_scenes_stay_on_the_host(ctx):
    assert len(scene("grid48").tris) > 4096
    for name in ("cornell", "cornell_spheres"):                         # 634 listed triangles; 3 876: at or below 4 096
        st = upload(ctx, scene(name), 2)
        assert (st.tree_builder_used, st.leaves_used) == (1, 2), name
    sc = scene("grid48")
    tris = sc.tris.copy()
    tris["v1"][5, 1] = np.inf
    bad = scenes.Scene("bad", tris, sc.mats, sc.nodes, sc.lights, sc.atlas, sc.bvh_depth)
    st = upload(ctx, bad, 2)
    assert st.leaves_used == 1
    ctx.set_options(keep_reference_tree=1)
    try:
        st = upload(ctx, sc, 2)
        assert (st.tree_builder_used, st.leaves_used) == (0, 1)
    finally:
        ctx.set_options(keep_reference_tree=0)


def nested_line(n):
    """Triangles (0,0,0), (i,0,0), (i,1,0): every box holds all the smaller ones, so the smallest union of any triangle is with the
    lowest one in reach, only the bottom pair is ever mutual, and PLOC would merge one pair per pass into a chain n levels deep. The
    uploaded BVH over their distinct centroids stays shallow, so the scene is accepted."""
    i = np.arange(1, n + 1, dtype=np.float64)
    v = np.zeros((n, 3, 3), np.float64)
    v[:, 1, 0] = i
    v[:, 2, 0] = i; v[:, 2, 1] = 1.0
    nrm = np.zeros((n, 3, 3), np.float32)
    nrm[..., 2] = 1.0
    tris = scenes._tri_array(v.astype(np.float32), nrm, np.zeros((n, 3, 2), np.float32), np.arange(n) % 2)
    base = scenes.deep_chain(n=8)
    return scenes._finish("nested_line", [tris], list(base.mats))


def test_a_tree_too_deep_for_the_device_falls_back_to_the_host(ctx):
    sc = nested_line(5000)
    assert sc.bvh_depth <= 40
    st = upload(ctx, sc, 2)
    assert (st.tree_builder_used, st.leaves_used) == (1, 2)             # refused within depth_limit + leaf_tris passes, then the host
    assert st.upload_tree_ms < 2000
    info = ctx.read_image()[0]
    assert info.depth <= 60


# -- 2. the read-back is faithful ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_spheres", "grid96"])
@pytest.mark.parametrize("leaves", [1, 2])
def test_read_image_equals_the_host_build(ctx, name, leaves):
    sc = scene(name)
    upload(ctx, sc, 1, leaves=leaves)
    got = ctx.read_image()
    want = native.build_image(sc, leaves=leaves)
    assert info_bytes(got[0]) == info_bytes(want[0])
    for g, w, what in zip(got[1:], want[1:], ("wnodes", "qnodes", "tripos", "leafbox")):
        assert same_arrays(g, w), (name, leaves, what)


# -- 3. the device image is sound -------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """f32 fma(a, b, c) with one rounding: a * b is exact in f64 (24 + 24 bits), the sum's f64 rounding error is recovered exactly
    (two-sum), and an f64 sum that lands on the midpoint of two f32 values is rounded by the sign of that error (ties to even only
    when it is zero)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bp = s - c
    err = (p - bp) + (c - (s - bp))
    f = s.astype(np.float32)
    lo = np.where(f.astype(np.float64) > s, np.nextafter(f, np.float32(-np.inf)), f)
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2.0
    on_mid = s == mid
    f = np.where(on_mid & (err > 0), hi, np.where(on_mid & (err < 0), lo, f))
    return f.astype(np.float32)


def check_image(sc, img, k):
    info, wn, qn, tp, lb = img
    assert info.leaves_used == 2 and 1 <= info.max_leaf_tris <= k and info.pad > 0
    listed = np.zeros(len(sc.tris), bool)
    for n in sc.nodes[sc.nodes["triangle_count"] > 0]:
        listed[n["triangle_offset"]:n["triangle_offset"] + n["triangle_count"]] = True
    orig = tp[:, 3].copy().view(np.uint32)
    assert len(orig) == listed.sum() and np.array_equal(np.sort(orig), np.flatnonzero(listed))
    T = sc.tris[orig]
    assert np.array_equal(tp[:, 0:3], T["v0"]) and np.array_equal(tp[:, 4:7], T["v1"] - T["v0"]) and np.array_equal(tp[:, 8:11], T["v2"] - T["v0"])
    seen = np.zeros(len(tp), np.int32)
    verts = np.stack([T["v0"], T["v1"], T["v2"]], axis=1).astype(np.float64)
    u = wn.view(np.uint32)
    lo_n = np.empty((len(wn), 3)); hi_n = np.empty((len(wn), 3))
    # iterative post-order walk (device trees may be deep)
    order, st = [], [(info.root_ref, 1)]
    while st:
        ref, d = st.pop()
        if ref & REF_LEAF:
            continue
        order.append((ref, d))
        st.append((int(u[ref, 12]), d + 1)); st.append((int(u[ref, 13]), d + 1))
    max_depth = 1
    for ref, d in reversed(order):
        bounds = []
        for side in (0, 1):
            c = int(u[ref, 12 + side])
            if c & REF_LEAF:
                first, cnt = c & ((1 << 26) - 1), ((c >> 26) & 31) + 1
                assert cnt <= k
                seen[first:first + cnt] += 1
                v = verts[first:first + cnt].reshape(-1, 3)
                bounds.append((v.min(axis=0), v.max(axis=0)))
                max_depth = max(max_depth, d + 1)
            else:
                bounds.append((lo_n[c], hi_n[c]))
        for (lo, hi), blo, bhi in zip(bounds, (wn[ref, 0:3], wn[ref, 6:9]), (wn[ref, 3:6], wn[ref, 9:12])):
            assert (blo.astype(np.float64) <= lo - 0.99 * info.pad).all() and (bhi.astype(np.float64) >= hi + 0.99 * info.pad).all()
        lo_n[ref] = np.minimum(bounds[0][0], bounds[1][0]); hi_n[ref] = np.maximum(bounds[0][1], bounds[1][1])
    assert (seen == 1).all()
    assert max_depth == info.depth and info.depth <= 60
    assert info.n_leaves == len(wn) + 1
    if qn is not None:                   # the quantised planes, decoded with the kernel's fmaf, hold the padded boxes
        qo = np.array(info.q_origin[:], np.float32); qs = np.array(info.q_scale[:], np.float32)
        todo, visited = [(0, 0)], 0
        while todo:
            i, qi = todo.pop()
            visited += 1
            for side in (0, 1):
                q = qn[qi, 4 * side:4 * side + 4]
                pl = np.array([q[0] & 0xFFFF, q[0] >> 16, q[1] & 0xFFFF, q[1] >> 16, q[2] & 0xFFFF, q[2] >> 16], np.float32)
                dlo, dhi = fmaf(qs, pl[0:3], qo), fmaf(qs, pl[3:6], qo)
                assert (dlo <= wn[i, 6 * side:6 * side + 3]).all() and (dhi >= wn[i, 6 * side + 3:6 * side + 6]).all()
                r = int(u[i, 12 + side])
                assert (int(q[3]) & REF_LEAF) == (r & REF_LEAF)
                if r & REF_LEAF:
                    assert int(q[3]) == r
                else:
                    todo.append((r, int(q[3])))
        assert visited == len(wn)


@pytest.mark.parametrize("name", ["grid48", "grid96"])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_device_image_is_sound_and_shares_the_host_padding(ctx, name, k):
    sc = scene(name)
    st = upload(ctx, sc, 2, leaf_tris=k)
    assert st.tree_builder_used == 2
    img = ctx.read_image()
    check_image(sc, img, k)
    host = native.build_image(sc, leaves=2, leaf_tris=k)
    for f in ("pad", "safe_origin"):
        assert bits(getattr(img[0], f)) == bits(getattr(host[0], f)), f
    for f in ("root_min", "root_max"):
        assert np.array_equal(bits(np.array(getattr(img[0], f)[:])), bits(np.array(getattr(host[0], f)[:]))), f
    assert same_arrays(img[4], host[4])


def requantised_words(info, wn):
    """The three plane words of both children of every wide node [n, 2, 3], from the rule itself: on each axis the LARGEST plane
    number whose plane fma(scale, k, origin), in float32, is <= the box's lower bound, and the SMALLEST whose plane is >= its upper
    bound (an axis of scale 0 has plane 0 only). The double-precision quotient is a first guess that is then moved either way."""
    qo = np.array(info.q_origin[:], np.float32); qs = np.array(info.q_scale[:], np.float32)
    lo = np.stack([wn[:, 0:3], wn[:, 6:9]], axis=1)
    hi = np.stack([wn[:, 3:6], wn[:, 9:12]], axis=1)

    def plane(k):
        return fmaf(qs, k.astype(np.float32), qo)

    def search(v, below):
        x = (v.astype(np.float64) - qo) / np.where(qs > 0, qs, np.float32(1)).astype(np.float64)
        k = np.clip(np.floor(x) if below else np.ceil(x), 0, 65535).astype(np.int64)
        for _ in range(16):
            if below:
                down = (k > 0) & (plane(k) > v)
                up = ~down & (k < 65535) & (plane(np.minimum(k + 1, 65535)) <= v)
            else:
                up = (k < 65535) & (plane(k) < v)
                down = ~up & (k > 0) & (plane(np.maximum(k - 1, 0)) >= v)
            if not (down | up).any():
                break
            k = k - down + up
        else:
            raise AssertionError("the plane search did not settle")
        return np.where(qs > 0, k, 0).astype(np.uint32)

    ql, qh = search(lo, True), search(hi, False)
    return np.stack([ql[..., 0] | (ql[..., 1] << 16), ql[..., 2] | (qh[..., 0] << 16), qh[..., 1] | (qh[..., 2] << 16)], axis=-1)


def quantised_numbers(wn, qn):
    """perm[i]: the quantised node that stands for wide node i, by the child references of both arrays walked together from the
    roots; asserts that they describe one tree (leaf references equal, every node of either array reached exactly once)."""
    u = wn.view(np.uint32)
    perm = np.full(len(wn), -1, np.int64)
    taken = np.zeros(len(qn), bool)
    todo = [(0, 0)]
    while todo:
        i, qi = todo.pop()
        assert perm[i] < 0 and not taken[qi]
        perm[i] = qi; taken[qi] = True
        for side in (0, 1):
            r, q = int(u[i, 12 + side]), int(qn[qi, 4 * side + 3])
            if r & REF_LEAF:
                assert q == r
            else:
                assert not (q & REF_LEAF) and r < len(wn) and q < len(qn)
                todo.append((r, q))
    assert (perm >= 0).all() and taken.all()
    return perm


@pytest.mark.parametrize("k", [1, 2, 4])
def test_device_planes_are_the_shared_definitions(ctx, k):
    """The device builder's quantised nodes are pinned to the one definition (csrc/wide_node.h), not merely to soundness: its own
    wide nodes, quantised again here on the grid it reports, give its plane words bit for bit. grid48 is the smallest scene the
    device builder accepts. Its renumbering is not recomputed, only checked to be a renumbering of the same tree.

    (The rule asks for the nearest plane. The library stops one plane short of it where that plane rounds onto the bound itself while
    the double-precision quotient stays below the integer — 40 to 100 words of cornell_spheres' host images, none of this scene's:
    every bound of either builder's tree here is a padded triangle coordinate, and the host image at leaf_tris = 1, which holds every
    triangle's box as a child, meets the rule throughout.)"""
    sc = scene("grid48")
    assert upload(ctx, sc, 2, leaf_tris=k).tree_builder_used == 2
    info, wn, qn, _, _ = ctx.read_image()
    assert info.quantised == 1 and qn is not None and len(qn) == len(wn) == info.n_wnodes
    perm = quantised_numbers(wn, qn)
    got = qn[perm].reshape(len(wn), 2, 4)[..., 0:3]
    assert np.array_equal(got, requantised_words(info, wn))


# -- 4. the build is deterministic --------------------------------------------------------------------------------------------------
def test_device_build_is_deterministic(ctx):
    sc = scene("grid96")
    upload(ctx, sc, 2)
    a = ctx.read_image()
    upload(ctx, sc, 2)
    b = ctx.read_image()
    assert info_bytes(a[0]) == info_bytes(b[0]) and all(same_arrays(x, y) for x, y in zip(a[1:], b[1:]))
    with native.MultiContext([0, 0], loopback=True) as m:
        m.set_options(leaves=2, tree_builder=2)
        m.upload_scene(sc)
        for i in range(2):
            got = m.read_image(i)
            assert info_bytes(got[0]) == info_bytes(a[0])
            assert all(same_arrays(x, y) for x, y in zip(got[1:], a[1:]))


# -- 4b. the device image keeps its bits ----------------------------------------------------------------------------------------------
# Nothing above pins the device tree's topology against a model, so its bytes are: tests/golden/own_tree_gpu_digests.json (written by
# tests/golden/make_own_tree_gpu_digests.py) holds a SHA-256 of each array of read_image() for the smallest scenes the builder accepts.
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_tree_gpu_digests.json")
DIGEST_CASES = [("grid48", 1), ("grid48", 2), ("grid48", 4), ("soup20k", 0)]          # (scene, leaf_tris)


def digest_key(name, leaf_tris):
    return f"{name}/leaf_tris={leaf_tris}"


def device_image_digests(ctx, name, leaf_tris):
    """(ptmi_stats of the upload, {array: SHA-256}) of the image the device builder makes"""
    st = upload(ctx, scene(name), 2, leaf_tris=leaf_tris, leaves=2)
    info, wn, qn, tp, lb = ctx.read_image()

    def sha(a):
        return None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    return st, {"info": hashlib.sha256(info_bytes(info)).hexdigest(), "wnodes": sha(wn), "qnodes": sha(qn), "tripos": sha(tp), "leafbox": sha(lb)}


@pytest.mark.parametrize("name,leaf_tris", DIGEST_CASES)
def test_device_image_is_the_recorded_one(ctx, name, leaf_tris):
    st, got = device_image_digests(ctx, name, leaf_tris)
    assert st.tree_builder_used == 2                                    # a fallback to the host must not pass
    with open(DIGESTS) as f:
        want = json.load(f)
    assert got == want[digest_key(name, leaf_tris)]


# -- 5, 6. CPU replay of the device image: the reference traversal's results, and the work per ray ----------------------------------
def tapped_rays(oracle, sc, W, H):
    from test_own_leaves_host import special_rays
    cam = layout.make_camera(W, H, aperture=0.01, focus_distance=2.8)
    rec, _ = gate.tap_rays(oracle, sc, cam, 2, 0, H, 1 << 21)
    sp = special_rays(sc, 20_000, 17)
    t, tri, _, _, _ = oracle.intersect(sc, sp[:, 0:3], sp[:, 3:6])
    sp[:, 7] = t
    sp[:, 8] = tri.view(np.float32)
    return np.ascontiguousarray(np.concatenate([rec, sp]))


QUALITY = {}


@pytest.mark.parametrize("name,W,H", [("grid48", 160, 96), ("grid96", 160, 96), ("grid_1m", 96, 54)])
def test_cpu_replay_matches_the_reference_and_costs_about_the_host_tree(ctx, oracle, name, W, H, record_property):
    sc = scene(name)
    L = gate.sim_lib()
    rec = tapped_rays(oracle, sc, W, H)
    assert upload(ctx, sc, 2).tree_builder_used == 2
    dev = gate.Image(sc, 2, arrays=ctx.read_image())
    for quant in ((0, 1) if dev.qn is not None else (0,)):
        for cull, deferred in ((1, 0), (1, 1), (0, 0)):
            sums, diff = gate.run(L, dev, rec, quant, cull, deferred, want_diff=8)
            assert int(sums[8]) == 0 and int(sums[9]) == 0, (name, quant, cull, deferred, sums.tolist(), rec[diff.astype(np.int64)])
    host, _ = gate.run(L, gate.Image(sc, 2), rec, 0)
    devs, _ = gate.run(L, dev, rec, 0)
    rays = int(host[6]) + int(host[7])
    boxes = (int(devs[0]) + int(devs[3])) / (int(host[0]) + int(host[3]))
    tris = (int(devs[2]) + int(devs[5])) / (int(host[2]) + int(host[5]))
    record_property("box_steps_ratio", boxes)
    record_property("triangle_tests_ratio", tris)
    print(f"\n{name}: {rays} rays, device / host tree: box steps {boxes:.3f}, triangle tests {tris:.3f}")
    assert boxes <= 1.15 and tris <= 1.10, (name, boxes, tris)


# -- 7. GPU parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid48", "grid96", "soup20k", "grid_1m", "deep3"])
def test_device_tree_gives_the_oracles_hits(ctx, oracle, name):
    sc = scene(name)
    st = upload(ctx, sc, 2)
    assert st.leaves_used == 2
    assert st.tree_builder_used in ((2,) if name != "deep3" else (1, 2))
    o, d = more_rays(sc, 100_000, 43)
    ot, otri, ou, ov, _ = oracle.intersect(sc, o, d)
    dist = (np.random.default_rng(9).random(len(o)) * 2.5).astype(np.float32)
    dist[::5] = -1.0
    occ_ref = oracle.occluded(sc, o, d, dist)
    for trav in (native.TRAVERSAL_AUTO, native.TRAVERSAL_GLOBAL, native.TRAVERSAL_GLOBAL_EXACT):
        for cull in (1, 0):
            ctx.set_options(traversal=trav, cull=cull)
            gt, gtri, gu, gv = ctx.debug_intersect(o, d)
            assert np.array_equal(gtri, otri), (name, trav, cull, int((gtri != otri).sum()))
            assert_same_floats(gt, ot, "t"); assert_same_floats(gu, ou, "u"); assert_same_floats(gv, ov, "v")
            assert np.array_equal(ctx.debug_occluded(o, d, dist), occ_ref), (name, trav, cull)


def render(ctx, sc, builder, W, H, frames, cam):
    upload(ctx, sc, builder)
    ctx.resize(W, H)
    ctx.set_options(max_bounces=8, do_mis=1, tile_y0=0, tile_y1=0, frames_per_batch=0, cull=1, traversal=native.TRAVERSAL_AUTO)
    ctx.reset_stats()
    ctx.dispatch(cam, frames)
    return ctx.read_output(), ctx.stats()


@pytest.mark.parametrize("name,W,H,frames", [("grid48", 64, 48, 3), ("soup20k", 64, 48, 2), ("deep3", 64, 48, 2)])
def test_render_with_the_device_tree_equals_the_oracle(ctx, oracle, name, W, H, frames):
    sc = scene(name)
    cam = layout.make_camera(W, H, aperture=0.001, focus_distance=2.8)
    ref, ost = oracle.render(sc, cam, frames, max_bounces=8, do_mis=1)
    got, st = render(ctx, sc, 2, W, H, frames, cam)
    assert (st.segments, st.shadow_rays, st.paths) == (ost.segments, ost.shadow_rays, ost.paths)
    assert_same_floats(got, ref, f"radiance {name}")


def test_grid_1m_frame_is_the_same_under_both_builders(ctx):
    sc = scene("grid_1m")
    cam = layout.make_camera(480, 270, aperture=0.001, focus_distance=2.8)
    a, sa = render(ctx, sc, 1, 480, 270, 4, cam)
    b, sb = render(ctx, sc, 2, 480, 270, 4, cam)
    assert (sa.tree_builder_used, sb.tree_builder_used) == (1, 2)
    assert (sa.segments, sa.shadow_rays, sa.shadow_traced, sa.paths) == (sb.segments, sb.shadow_rays, sb.shadow_traced, sb.paths)
    assert list(sa.segments_by_bounce) == list(sb.segments_by_bounce)
    assert np.array_equal(bits(a), bits(b))


# -- 8. the same kernel variants are chosen -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_spheres", "grid_1m"])
def test_both_builders_choose_the_same_variants(ctx, name):
    sc = scene(name)
    cam = layout.make_camera(32, 24)
    got = []
    for builder in (1, 2):
        _, st = render(ctx, sc, builder, 32, 24, 1, cam)
        got.append((st.extend_variant, st.shadow_variant))
    assert got[0] == got[1], (name, got)
