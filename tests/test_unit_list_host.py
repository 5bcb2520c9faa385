"""tests/unit_list_ref.py on the host: the model of the rebuild's unit list, the tree surgery, and the census of the scenes that
tests/test_gpu_rebuild_units.py rebuilds. No GPU.

The census test is what keeps the GPU test honest: every scene is there for a path of csrc/scene_rebuild.hip (a word with holes, a
32-triangle leaf across a word edge, the count written by thread 1023, a second tile, an empty tile, ...), and a change to
scenes.grid_1m, to the seeds or to the helpers that loses that path fails HERE instead of silently thinning the GPU test. Beside it
stands a numpy restatement of the three kernels with a switch per plausible mistake (FAULTS): each mistake gives the right list on
every tree the suite rebuilt before and a wrong one on the scenes it names."""
import dataclasses

import numpy as np
import pytest

import unit_list_ref as U
from ptmi import native, scenes
from test_gpu_edge_cases import tiny_scene

_base = {}


def base(name):
    if name not in _base:
        _base[name] = (tiny_scene(int(name[4:])) if name.startswith("tiny") else scenes.grid_1m(n=int(name[4:])) if name.startswith("grid")
                       else scenes.make(name))
    return _base[name]


def walk(nodes, n_tris):
    """the unit list by a plain recursive walk, sharing nothing with unit_list_ref"""
    seen = set()

    def visit(i):
        n = nodes[i]
        if n["triangle_count"] > 0:
            seen.update(range(int(n["triangle_offset"]), int(n["triangle_offset"]) + int(n["triangle_count"])))
        else:
            visit(int(n["left"]))
            visit(int(n["right"]))
    if len(nodes):
        visit(0)
    assert all(t < n_tris for t in seen)
    return np.array(sorted(seen), np.uint32)


def small_surgery():
    """cornell widened to 9-triangle leaves, every third leaf dropped (but the emissive ones)"""
    s = base("cornell")
    turn = iter(range(1 << 30))
    keep = U.keeping(lambda first, end: next(turn) % 3 != 1, U.emissive_triangles(s.lights))
    return dataclasses.replace(s, nodes=U.drop(U.widen(s.nodes, 9), keep))


def assert_uploadable(s, what):
    """what csrc/scene_image.hip build_image asks of a tree before it builds own leaves over it"""
    nodes, n_tris = s.nodes, len(s.tris)
    end, seen, stack = 0, set(), [(0, 1)]
    while stack:
        i, depth = stack.pop()
        assert i not in seen and depth <= 62, what
        seen.add(i)
        n = nodes[i]
        if n["triangle_count"] > 0:
            first, cnt = int(n["triangle_offset"]), int(n["triangle_count"])
            assert cnt <= 32 and first >= end and first + cnt <= n_tris, f"{what}: leaf {i} lists [{first}, +{cnt}) after {end}"
            end = first + cnt
            continue
        for ch in (int(n["right"]), int(n["left"])):                 # (popped left first)
            assert (nodes["aabb_min"][ch] >= n["aabb_min"]).all() and (nodes["aabb_max"][ch] <= n["aabb_max"]).all(), f"{what}: node {ch} is not nested"
            stack.append((ch, depth + 1))
    assert nodes["triangle_count"][0] == 0, f"{what}: the root is a leaf"
    assert np.isfinite(nodes["aabb_min"][sorted(seen)]).all() and np.isfinite(nodes["aabb_max"][sorted(seen)]).all(), what
    assert U.listed(nodes, n_tris)[U.emissive_triangles(s.lights)].all(), f"{what}: an emissive triangle is unlisted"


@pytest.mark.parametrize("name", ["tiny5", "cornell", "surgery"])
def test_units_is_the_brute_force_walk(name):
    s = small_surgery() if name == "surgery" else base(name)
    got = U.units(s.nodes, len(s.tris))
    assert got.dtype == np.uint32 and np.array_equal(got, walk(s.nodes, len(s.tris)))
    if name == "surgery":
        c = U.census(s.nodes, len(s.tris))
        assert 0 < c.units < len(s.tris) and 4 < c.max_leaf <= 9, c
    else:
        assert np.array_equal(got, np.arange(len(s.tris)))           # a tree as scene_host.build_bvh makes it lists everything
    # scene_update_ref.leaf_boxes agrees about who is listed: an unlisted triangle's row stays zero, a listed one's does not
    lb = U.ref.leaf_boxes(s.nodes, len(s.tris))
    assert np.array_equal(np.flatnonzero(lb.any(axis=1)), got)


def test_surgery_that_changes_nothing_returns_the_nodes():
    for name in ("tiny5", "cornell", "grid48"):
        nodes = base(name).nodes
        assert U.drop(nodes, lambda first, end: True).tobytes() == nodes.tobytes(), name
        assert U.widen(nodes, limit=4).tobytes() == nodes.tobytes(), name


def test_the_root_must_survive():
    nodes = base("cornell").nodes
    with pytest.raises(ValueError):
        U.drop(nodes, lambda first, end: False)
    half = int(U._spans(nodes)[1][int(nodes["left"][0])])               # where the root's left subtree ends
    with pytest.raises(ValueError):                                    # nothing left on the root's left side
        U.drop(nodes, lambda first, end: first >= half)


def test_surgery_keeps_what_an_upload_asks():
    s = small_surgery()
    assert_uploadable(s, "cornell widened and thinned")
    before, after = base("cornell").nodes, s.nodes
    assert np.array_equal(before["aabb_min"], after["aabb_min"]) and np.array_equal(before["aabb_max"], after["aabb_max"])   # boxes stay
    assert len(after) == len(before)
    # the host-only upload admits it and lists exactly the model's triangles
    info, wn, qn, tp, lb = native.build_image(s, leaves=2)
    assert info.leaves_used == 2 and info.n_tris == len(U.units(s.nodes, len(s.tris))) < len(s.tris)
    assert np.array_equal(np.sort(tp.view(np.uint32)[:, 3]), U.units(s.nodes, len(s.tris)))


def test_widen_makes_maximal_contiguous_leaves():
    s = base("grid48")
    wide = U.widen(s.nodes)
    assert np.array_equal(U.units(wide, len(s.tris)), np.arange(len(s.tris)))
    first, end, total = U._spans(s.nodes)
    leaves = U.reachable_leaves(wide)
    assert len(leaves) < len(U.reachable_leaves(s.nodes)) // 4
    parent = {int(s.nodes[k][i]): i for i in np.flatnonzero(s.nodes["triangle_count"] == 0) for k in ("left", "right")}
    for i in leaves:
        assert wide["triangle_offset"][i] == first[i] and wide["triangle_count"][i] == total[i] <= 32
        assert parent[int(i)] == 0 or total[parent[int(i)]] > 32       # maximal: the parent would not fit (or is the root)


# what each scene must reach in csrc/scene_rebuild.hip, as conditions on its census (the figures of tests/test_gpu_rebuild_units.py's
# docstring are one measurement of them)
CONDITIONS = {
    "grid48/wide": lambda c: c.max_leaf == 32 and c.wide_word_straddles >= 1 and c.units == 4428,
    "grid48/sparse": lambda c: 1 <= c.units <= 2048 and c.partial_words == c.words and c.zero_words == 0,
    "grid182/wide+holes": lambda c: c.words == 1024 and c.tiles == 1 and c.last_word_bits == 60 and c.partial_words >= 100,
    "grid183/plain": lambda c: c.tiles == 2 and c.words == 1036 and c.tile_popcounts[0] == 65536 and c.units == 66258 and c.tile_straddles == 1,
    "grid183/edge": lambda c: c.tiles == 2 and 0 < 65536 - c.tile_popcounts[0] < 128 and c.tile_straddles >= 1,
    "grid183/wide+holes": lambda c: c.tiles == 2 and c.wide_word_straddles >= 100 and c.units < 66258,
    "grid320/empty-tile": lambda c: c.tiles == 4 and c.tile_popcounts[1] == 0 and c.zero_words >= 1024 and c.longest_zero_run > 1000
    and min(c.tile_popcounts[0], c.tile_popcounts[2], c.tile_popcounts[3]) > 0,
    "grid320/wide+empty-tile": lambda c: c.tiles == 4 and c.tile_popcounts[1] < 64 and c.tile_straddles >= 1 and c.max_leaf == 32,
}


# ---- the evidence that the scenes can tell a wrong kernel from a right one -------------------------------------------------------------
# No deliberately broken kernel runs on a GPU: a wrong list hands the builders uninitialised indices. Instead the three kernels are
# restated here in numpy, word for word, with a switch for each way of getting them subtly wrong; a faulty restatement must give the
# model's list on every tree of tests/test_gpu_rebuild_tree.py (the gap) and a different one on the scenes named (the gap closed).
FAULTS = {
    "offsets_of_full_words": ("grid48/sparse", "grid182/wide+holes"),   # my_off = 64 * word: no scan at all
    "full_words_within_a_wave": ("grid48/sparse", "grid183/edge"),      # my_off = base0 + wbase + 64 * lane: only the wave's scan gone
    "no_tile_base": ("grid183/plain", "grid183/edge", "grid320/empty-tile"),   # the totals of the tiles in front left out
    "only_the_tile_before": ("grid320/empty-tile", "grid320/wide+empty-tile"),  # pre = tile_sums[tile - 1]: right for two tiles
    "w0_without_the_tile": ("grid183/plain", "grid320/wide+empty-tile"),        # w0 = wave * 64
    "count_by_tile_0": ("grid183/plain", "grid183/edge", "grid320/empty-tile"),  # thread 1023 of tile 0 writes the count
    "count_without_its_word": ("grid182/wide+holes",),                  # *count = my_off: right while thread 1023's word is past the end
    "mask_in_32_bits": ("grid48/wide", "grid320/wide+empty-tile"),      # (1u << cnt) - 1u: nothing for cnt = 32
    "spill_in_16_bits": ("grid48/wide", "grid182/wide+holes"),          # the part for the second word held in a uint16_t
}
BLIND = ("grid48", "grid80", "cornell", "cornell_spheres", "tiny5")      # the trees tests/test_gpu_rebuild_tree.py rebuilds
NOTHING = np.uint32(0xFFFFFFFF)


def kernels(nodes, n_tris, fault=None):
    """(which [n_tris], count) as k_flag_leaves, k_unit_tile_sums and k_unit_scatter of csrc/scene_rebuild.hip leave them"""
    leaf = U.reachable_leaves(nodes)
    first, cnt = nodes["triangle_offset"][leaf].astype(np.uint64), nodes["triangle_count"][leaf].astype(np.uint64)
    nwords = (n_tris + 63) // 64
    tiles = (nwords + U.TILE_WORDS - 1) // U.TILE_WORDS
    words = np.zeros(tiles * U.TILE_WORDS, np.uint64)                  # (the words past nwords read as 0 in the kernels)
    one, lo = np.uint64(1), first & np.uint64(63)
    with np.errstate(over="ignore"):
        m = (one << cnt) - one
        if fault == "mask_in_32_bits":
            m = np.where(cnt == 32, np.uint64(0), m)
        np.bitwise_or.at(words, (first >> np.uint64(6)).astype(np.int64), m << lo)
        two = lo + cnt > 64
        spill = m[two] >> (np.uint64(64) - lo[two])
        if fault == "spill_in_16_bits":
            spill &= np.uint64(0xFFFF)
        np.bitwise_or.at(words, (first[two] >> np.uint64(6)).astype(np.int64) + 1, spill)
    bits = np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little").reshape(-1, 64).astype(bool)
    c = bits.sum(axis=1).astype(np.int64).reshape(tiles, U.TILE_WORDS)
    sums = c.sum(axis=1)
    front = np.concatenate([[0], np.cumsum(sums)[:-1]])                 # tile_base
    if fault == "no_tile_base":
        front[:] = 0
    if fault == "only_the_tile_before":
        front = np.concatenate([[0], sums[:-1]])
    inc = np.cumsum(c, axis=1)
    my_off = front[:, None] + inc - c
    writer = 0 if fault == "count_by_tile_0" else tiles - 1
    count = int(my_off[writer, -1] + (0 if fault == "count_without_its_word" else c[writer, -1]))
    if fault == "offsets_of_full_words":                               # (the count is left right: such a kernel would count otherwise)
        my_off = 64 * np.arange(tiles * U.TILE_WORDS, dtype=np.int64).reshape(tiles, U.TILE_WORDS)
    if fault == "full_words_within_a_wave":
        waves = c.reshape(tiles, -1, 64).sum(axis=2)
        wbase = np.repeat(np.cumsum(waves, axis=1) - waves, 64, axis=1)
        my_off = front[:, None] + wbase + 64 * (np.arange(U.TILE_WORDS) % 64)[None, :]
    word, lane = np.nonzero(bits)
    rank = (np.cumsum(bits, axis=1) - bits)[word, lane]
    at = my_off.reshape(-1)[word] + rank
    w_named = word % U.TILE_WORDS if fault == "w0_without_the_tile" else word
    which = np.full(n_tris, NOTHING, np.uint32)
    ok = (at >= 0) & (at < n_tris)
    which[at[ok]] = (w_named[ok] * 64 + lane[ok]).astype(np.uint32)
    return which, count


def right(nodes, n_tris, fault):
    want = U.units(nodes, n_tris)
    which, count = kernels(nodes, n_tris, fault)
    return count == len(want) and np.array_equal(which[:len(want)], want)


def test_the_restated_kernels_give_the_models_list():
    for name in BLIND:
        assert right(base(name).nodes, len(base(name).tris), None), name
    for name in U.SCENES:
        s = U.operated(name, base)
        assert right(s.nodes, len(s.tris), None), name


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_faulty_kernels_pass_the_old_scenes_and_fail_the_new(fault):
    for name in BLIND:
        assert right(base(name).nodes, len(base(name).tris), fault), f"{fault} shows on {name}: it was no gap"
    caught = [name for name in U.SCENES if not right(U.operated(name, base).nodes, len(base(name.split("/")[0]).tris), fault)]
    print(fault, caught)
    assert set(FAULTS[fault]) <= set(caught), (fault, caught)


def test_every_scene_has_a_condition():
    assert set(CONDITIONS) == set(U.SCENES)


@pytest.mark.parametrize("name", U.SCENES)
def test_census_and_preconditions_of_the_rebuilt_scenes(name):
    s = U.operated(name, base)
    c = U.census(s.nodes, len(s.tris))
    print(name, c)
    assert CONDITIONS[name](c), (name, c)
    assert c.units == len(U.units(s.nodes, len(s.tris))) == sum(c.tile_popcounts)
    assert_uploadable(s, name)
    assert s.tris is base(name.split("/")[0]).tris                     # only the nodes are operated on
