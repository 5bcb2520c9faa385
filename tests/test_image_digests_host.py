"""Every buffer the host builds for a scene keeps its bits — host logic, no GPU.

tests/golden/image_digests.json (written by tests/golden/make_image_digests.py) holds, per scene and leaf mode, a SHA-256 of each
buffer ptmi_debug_build_image returns (the header's bytes, the wide nodes, the quantised nodes, the triangles, the leaf boxes) and,
per scene, the eight values of ptmi_debug_image_stats, whose stream counts and mismatch check cover the leaf stream the ABI does not
return. The scenes reach every path of the quantisers (csrc/quantise.hip): a grid that is refused for its area growth (deep_chain), a
zero scale on one axis (flat), and, per leaf mode, an image of at least 65 536 wide nodes, from where the fill runs on several threads."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from ptmi import native, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_digests.json")
THREADED_NODES = 65536                     # the quantisers' fill runs on one thread below this many wide nodes

SMALL = ["cornell", "cornell_spheres", "feature_box", "soup3", "soup8", "grid96", "deep_chain", "flat"]
MODES = [(1, 0), (2, 1), (2, 2), (2, 4)]   # (leaves, leaf_tris)
BIG = [("grid450", 1, 0), ("grid260", 2, 1)]
CASES = [(s, l, k) for s in SMALL for l, k in MODES] + BIG
STATS = SMALL + ["grid450"]

_scenes = {}


def flat():
    """tests/test_traversal_image.py: six quads in one plane, so that one axis has extent 0"""
    t = scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0), 0)
    parts = []
    for i in range(6):
        q = t.copy()
        for k in ("v0", "v1", "v2"):
            q[k][:, 0] += 3.0 * i
        parts.append(q)
    return scenes._finish("flat", parts, [scenes._material()])


def scene(name):
    if name not in _scenes:
        if name.startswith("soup"):
            _scenes[name] = scenes.random_soup(int(name[4:]), n_tris=900)
        elif name.startswith("grid"):
            _scenes[name] = scenes.grid_1m(n=int(name[4:]))
        elif name == "flat":
            _scenes[name] = flat()
        else:
            _scenes[name] = scenes.make(name)
    return _scenes[name]


def key(name, leaves, leaf_tris):
    return f"{name}/leaves={leaves}/leaf_tris={leaf_tris}"


def sha(a):
    return None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def image_digests(name, leaves, leaf_tris):
    info, wn, qn, tp, lb = native.build_image(scene(name), leaves=leaves, leaf_tris=leaf_tris)
    d = {"info": hashlib.sha256(ctypes.string_at(ctypes.addressof(info), ctypes.sizeof(info))).hexdigest(),
         "wnodes16": sha(wn), "qnodes8": sha(qn), "tripos12": sha(tp), "leafbox8": sha(lb)}
    return d, info


def stats_values(name):
    r = native.image_stats(scene(name))
    return [float(v).hex() for v in r.values()]          # the doubles themselves, not a rounded print of them


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,leaves,leaf_tris", CASES)
def test_image_buffers_keep_their_bits(golden, name, leaves, leaf_tris):
    got, info = image_digests(name, leaves, leaf_tris)
    assert info.leaves_used == leaves
    if (name, leaves, leaf_tris) in BIG:
        assert info.n_wnodes >= THREADED_NODES and info.quantised == 1, (info.n_wnodes, info.quantised)
    assert got == golden["images"][key(name, leaves, leaf_tris)]


@pytest.mark.parametrize("name", STATS)
def test_image_stats_keep_their_values(golden, name):
    assert stats_values(name) == golden["stats"][name]


def test_the_refused_and_the_flat_grids_are_among_the_cases(golden):
    assert golden["images"][key("deep_chain", 1, 0)]["qnodes8"] is None
    assert golden["images"][key("flat", 1, 0)]["qnodes8"] is not None
    info = native.build_image(scene("flat"), leaves=1)[0]
    assert info.quantised == 1 and info.q_scale[1] == 0.0
