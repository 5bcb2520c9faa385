"""The unit list of ptmi_rebuild_tree (csrc/scene_rebuild.hip: k_flag_leaves, k_unit_tile_sums, k_unit_scatter), modelled,
and the tree surgery that makes uploaded trees whose list is not the identity. Pure numpy over layout.BVH_NODE arrays: no GPU, no
library call.

  units     the model: the ascending indices of the triangles in the range of a leaf reached from node 0 (scene_update_ref.leaf_boxes
            leaves zeros for exactly the others)
  widen     every maximal subtree below the root that lists at most `limit` triangles over one contiguous range becomes a leaf
            (its box stays): leaves of up to PT_LEAF_MAX_TRIS = 32 triangles, which scene_host.build_bvh (max_leaf = 4) never makes
  drop      the reachable leaves a predicate refuses disappear; a node with one child left is replaced by that child, a node with none
            disappears. The triangles of a dropped leaf become UNLISTED: they stay in the triangle array and no ray can hit them.
  census    what a tree exercises in the three kernels: words, tiles of 1024 words, popcounts, straddling leaves
  poisoned  the unlisted triangles moved about 64 scene extents away: a list that leaks one shows in the root box and in the traces
  operated  the scenes of tests/test_unit_list_host.py and tests/test_gpu_rebuild_units.py, by name

Both operations keep what scene_image.hip build_image asks of an upload: leaf ranges ascend along the left-first DFS without overlap
and stay within n_tris, a leaf holds at most 32 triangles, the tree stays nested (a box that contained a subtree contains every part
of it). Nodes that are no longer reachable stay in the array: an upload numbers only the reachable ones."""
import dataclasses

import numpy as np

import scene_update_ref as ref

WORD = 64                             # triangles per ballot word
TILE_WORDS = 1024                     # csrc/pt_ballot_list.h TILE_WORDS
TILE = WORD * TILE_WORDS              # 65 536 triangles per tile
LEAF_MAX_TRIS = ref.LEAF_MAX_TRIS
LIGHT_EMISSIVE = 0                    # ptmi.layout.LIGHT_EMISSIVE


def reachable_leaves(nodes):
    """indices of the leaves a walk from node 0 reaches, in left-first DFS order"""
    out, stack = [], [0] if len(nodes) else []
    cnt, left, right = nodes["triangle_count"], nodes["left"], nodes["right"]
    while stack:
        i = stack.pop()
        if cnt[i] > 0:
            out.append(i)
        else:
            stack.append(int(right[i]))
            stack.append(int(left[i]))
        assert len(out) <= len(nodes) and len(stack) <= len(nodes), "the nodes are not a tree"
    return np.array(out, np.int64)


def listed(nodes, n_tris):
    """[n_tris] bool: some reachable leaf lists the triangle"""
    flags = np.zeros(n_tris, bool)
    reach = np.concatenate(ref.node_levels(nodes)) if len(nodes) else np.zeros(0, np.int64)
    leaf = reach[nodes["triangle_count"][reach] > 0]
    first, cnt = nodes["triangle_offset"][leaf].astype(np.int64), nodes["triangle_count"][leaf].astype(np.int64)
    assert not len(leaf) or int((first + cnt).max()) <= n_tris, "a leaf reaches beyond the triangles"
    for k in range(int(cnt.max()) if len(leaf) else 0):
        flags[first[cnt > k] + k] = True
    return flags


def units(nodes, n_tris):
    """the unit list: ascending indices of the triangles some reachable leaf lists"""
    return np.flatnonzero(listed(nodes, n_tris)).astype(np.uint32)


def _spans(nodes):
    """per node reachable from node 0: (first triangle, end, number of triangles listed) of its subtree; -1 for the others"""
    n = len(nodes)
    first, end, total = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for lvl in reversed(ref.node_levels(nodes)):
        cnt = nodes["triangle_count"][lvl].astype(np.int64)
        leaf, inner = lvl[cnt > 0], lvl[cnt == 0]
        first[leaf] = nodes["triangle_offset"][leaf]
        total[leaf] = cnt[cnt > 0]
        end[leaf] = first[leaf] + total[leaf]
        l, r = nodes["left"][inner].astype(np.int64), nodes["right"][inner].astype(np.int64)
        first[inner], end[inner], total[inner] = np.minimum(first[l], first[r]), np.maximum(end[l], end[r]), total[l] + total[r]
    return first, end, total


def widen(nodes, limit=LEAF_MAX_TRIS):
    """a copy in which every maximal subtree below the root with at most `limit` triangles over one contiguous range is a leaf"""
    assert 1 <= limit <= LEAF_MAX_TRIS
    out = nodes.copy()
    if not len(nodes) or nodes["triangle_count"][0] > 0:
        return out
    first, end, total = _spans(nodes)
    stack = [int(nodes["right"][0]), int(nodes["left"][0])]
    while stack:
        i = stack.pop()
        if nodes["triangle_count"][i] > 0:
            continue
        if total[i] <= limit and end[i] - first[i] == total[i]:      # (ranges do not overlap: equal means no gap)
            out["triangle_offset"][i], out["triangle_count"][i] = first[i], total[i]
            out["left"][i] = out["right"][i] = 0xFFFFFFFF            # as scene_host.build_bvh leaves a leaf's links
            continue
        stack.append(int(nodes["right"][i]))
        stack.append(int(nodes["left"][i]))
    return out


def drop(nodes, keep):
    """a copy without the reachable leaves for which keep(first, end) is false. keep is asked once per reachable leaf, in left-first
    DFS order (ascending ranges), so a predicate that draws random numbers is reproducible. ValueError: the root would not survive
    (it must keep something on both sides)."""
    out = nodes.copy()
    n = len(nodes)
    if not n:
        return out
    stands = np.full(n, -1, np.int64)                                # the node that stands for this subtree afterwards; -1: nothing
    for i in reachable_leaves(nodes):
        f = int(nodes["triangle_offset"][i])
        if keep(f, f + int(nodes["triangle_count"][i])):
            stands[i] = i
    for lvl in reversed(ref.node_levels(nodes)):
        inner = lvl[nodes["triangle_count"][lvl] == 0]
        l, r = stands[nodes["left"][inner]], stands[nodes["right"][inner]]
        both = (l >= 0) & (r >= 0)
        stands[inner] = np.where(both, inner, np.maximum(l, r))      # one side left: that side's node takes this node's place
        out["left"][inner[both]], out["right"][inner[both]] = l[both], r[both]
    if stands[0] != 0:
        raise ValueError("drop: the root does not survive")
    return out


def keeping(keep, protected):
    """keep, but true for every leaf that holds one of the triangles `protected` (the emissive ones: the light list derived from the
    triangles then still describes what rays can see). keep is asked first either way, so its random draws do not depend on them."""
    protected = np.sort(np.asarray(protected, np.int64))

    def k(first, end):
        wanted = bool(keep(first, end))
        return wanted or bool(np.searchsorted(protected, end) - np.searchsorted(protected, first))
    return k


def emissive_triangles(lights):
    return np.unique(lights["triangle_index"][lights["light_type"] == LIGHT_EMISSIVE]).astype(np.int64)


@dataclasses.dataclass
class Census:
    units: int
    words: int
    tiles: int
    tile_popcounts: list              # one per tile of 1024 words
    zero_words: int
    partial_words: int                # neither empty nor full (the last word is full when all the triangles it covers are listed)
    max_leaf: int
    word_straddles: int               # leaves with first % 64 + count > 64
    wide_word_straddles: int          # ... and count >= 17: the shifts m << lo and m >> (64 - lo) with more than 16 bits on one side
    tile_straddles: int               # leaves whose first and last triangle lie in different tiles
    last_word_bits: int
    longest_zero_run: int             # consecutive empty words


def census(nodes, n_tris):
    flags = listed(nodes, n_tris)
    words = (n_tris + WORD - 1) // WORD
    tiles = (words + TILE_WORDS - 1) // TILE_WORDS
    padded = np.zeros(tiles * TILE, bool)
    padded[:n_tris] = flags
    pop = padded.reshape(-1, WORD).sum(axis=1)[:words]
    room = np.full(words, WORD, np.int64)
    if n_tris % WORD:
        room[-1] = n_tris % WORD
    leaf = reachable_leaves(nodes)
    first, cnt = nodes["triangle_offset"][leaf].astype(np.int64), nodes["triangle_count"][leaf].astype(np.int64)
    straddle = first % WORD + cnt > WORD
    run = best = 0
    for z in pop == 0:
        run = run + 1 if z else 0
        best = max(best, run)
    return Census(units=int(flags.sum()), words=words, tiles=tiles,
                  tile_popcounts=[int(x) for x in padded.reshape(tiles, TILE).sum(axis=1)],
                  zero_words=int((pop == 0).sum()), partial_words=int(((pop > 0) & (pop < room)).sum()),
                  max_leaf=int(cnt.max()) if len(cnt) else 0, word_straddles=int(straddle.sum()),
                  wide_word_straddles=int((straddle & (cnt >= 17)).sum()),
                  tile_straddles=int((first // TILE != (first + cnt - 1) // TILE).sum()),
                  last_word_bits=int(pop[-1]) if words else 0, longest_zero_run=best)


# ---------------------------------------------------------------------------------------------------------------------- the poison --
POISON = 64.0                         # extents


def extent(tris):
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).reshape(-1, 3).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


def poisoned(tris, nodes, ext):
    """tris with every unlisted triangle turned and carried about POISON * ext away (finite, so an update admits them)"""
    away = np.flatnonzero(~listed(nodes, len(tris)))
    if not len(away):
        return tris
    return ref.move_part(tris, away, ref.rot_y(0.7), (POISON * ext, 0.5 * POISON * ext, -0.75 * POISON * ext))


# ---------------------------------------------------------------------------------------------------------------------- the scenes --
SEED = 3
# "<base scene>/<what is done to its tree>" (_recipe). Every random predicate draws from default_rng(SEED).
SCENES = ("grid48/wide", "grid48/sparse", "grid182/wide+holes", "grid183/plain", "grid183/edge", "grid183/wide+holes",
          "grid320/empty-tile", "grid320/wide+empty-tile")


def _random(p_keep):
    rng = np.random.default_rng(SEED)
    return lambda first, end: rng.random() < p_keep


def _recipe(name, n_tris):
    """(widen first, keep or None)"""
    base, how = name.split("/")
    wide = "wide" in how
    if how in ("wide", "plain"):
        return wide, None
    if how == "sparse":
        return wide, _random(0.4)
    if how == "edge":                                                # the leaves within 64 triangles of the first tile's end, but for one that crosses it
        return wide, lambda first, end: end <= TILE - WORD or first >= TILE + WORD or first < TILE < end
    if how == "wide+holes":
        rnd = _random(0.9)
        tail = WORD * ((n_tris - 1) // WORD)                          # the last word stays whole: its bit count is a census condition
        return wide, lambda first, end: bool(rnd(first, end)) or end > tail
    if how in ("empty-tile", "wide+empty-tile"):
        rnd = _random(0.9)
        return wide, lambda first, end: bool(rnd(first, end)) and not (first >= TILE and end <= 2 * TILE)
    raise ValueError(name)


_made = {}


def operated(name, base_scene):
    """the scene `name` of SCENES: base_scene(its part before the slash) with the nodes operated on. The triangles are the base's."""
    if name not in _made:
        s = base_scene(name.split("/")[0])
        wide, keep = _recipe(name, len(s.tris))
        nodes = widen(s.nodes) if wide else s.nodes.copy()
        if keep is not None:
            nodes = drop(nodes, keeping(keep, emissive_triangles(s.lights)))
        _made[name] = dataclasses.replace(s, name=name, nodes=nodes)
    return _made[name]
