"""The glTF loader's morph targets (host/gltf.js, host/scene_prep.js, host/animation.js): a primitive's targets and the default weights
are read (node.weights wins over mesh.weights), `weights` channels are sampled (LINEAR and STEP: at, between, before and after the
keys), the morph list names the morphed triangles in the uploaded order with their sparse rows, and the deltas arrive in the uploaded
space: under the collar's rotated, uniformly scaled node they match a direct computation. The file is tests/gltf_morph_scene.py's.
Every number in it is a binary fraction and the collar's matrix is a permutation times 0.5, so the comparisons are exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import gltf_morph_scene as face
import gltf_skin_scene as bar
from ptmi import layout
from test_gltf_host import HOST, NODE, _build, prepare, synthetic_glb

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

SCRIPT = """
var prep = require(%(prep)s), anim = require(%(anim)s), gltf = require(%(gltf)s).loadGLB(%(glb)s);
var plain = prep.prepareScene(gltf, { morphs: false });
var s = prep.prepareScene(gltf);
var info = { plainHasMorph: plain.morphTriangles !== undefined || plain.morphs !== undefined,
  sameBlobs: Object.keys(s.blobs).every(function (k) { return Buffer.from(s.blobs[k]).equals(Buffer.from(plain.blobs[k])); }),
  targets: gltf.meshes.map(function (m) { return m.primitives[0].targets ? m.primitives[0].targets.map(function (t) {
    return { position: !!t.POSITION, normal: !!t.NORMAL, count: t.POSITION ? t.POSITION.value.length / 3 : 0 }; }) : null; }),
  meshWeights: gltf.meshes.map(function (m) { return m.weights || null; }),
  nodeWeights: gltf.nodes.map(function (n) { return n.weights || null; }),
  defaults: gltf.nodes.map(function (n) { return anim.defaultWeights(n) || null; }) };
info.samples = %(times)s.map(function (t) { return anim.sample(gltf, 0, t); });
info.other = anim.sample(gltf, 1, 0.5);
info.poseDefault = Array.from(prep.morphPose(s, null));
info.poseAtOne = Array.from(prep.morphPose(s, anim.sample(gltf, 0, 1.0)));
console.log(JSON.stringify(info));
"""
TIMES = [-1.0, 0.0, 0.5, 0.99, 1.0, 1.5, 2.0, 3.0]


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    _build()
    d = tmp_path_factory.mktemp("face")
    rod, box = face.write_face(d / "face.glb")
    sc, info = prepare(d / "face.glb", d / "out")
    script = d / "morph.js"
    script.write_text(SCRIPT % dict(prep=json.dumps(os.path.join(HOST, "scene_prep.js")), anim=json.dumps(os.path.join(HOST, "animation.js")),
                                    gltf=json.dumps(os.path.join(HOST, "gltf.js")), glb=json.dumps(str(d / "face.glb")),
                                    times=json.dumps(TIMES)))
    js = json.loads(subprocess.check_output([NODE, str(script)], text=True).strip().splitlines()[-1])
    listed = np.fromfile(d / "out" / "morph_triangles.bin", np.uint32)
    rows = np.fromfile(d / "out" / "morph_rows.bin", np.uint32)
    deltas = np.fromfile(d / "out" / "morph_deltas.bin", layout.MORPH_DELTA)
    return d, rod, box, sc, info, js, listed, rows, deltas


def test_the_loader_reads_targets_and_default_weights(prepared):
    d, rod, box, sc, info, js, listed, rows, deltas = prepared
    n_rod, n_box = len(rod["positions"]), len(box["positions"])
    assert js["targets"] == [None, None, [dict(position=True, normal=True, count=n_rod), dict(position=True, normal=False, count=n_rod)],
                             [dict(position=True, normal=True, count=n_box)]]
    assert js["meshWeights"] == [None, None, face.BAR_DEFAULT, face.COLLAR_MESH_DEFAULT]
    assert js["nodeWeights"] == [None, None, None, None, None, face.COLLAR_NODE_DEFAULT]
    # node.weights wins over mesh.weights; a node without targets has no weights
    assert js["defaults"] == [None, None, face.BAR_DEFAULT, None, None, face.COLLAR_NODE_DEFAULT]
    assert js["poseDefault"] == face.BAR_DEFAULT + face.COLLAR_NODE_DEFAULT
    assert js["poseAtOne"] == face.BAR_KEYS[1] + face.COLLAR_KEYS[1]
    assert info["morphTargets"] == face.N_TARGETS
    assert info["morphs"] == [dict(node=face.BAR_NODE, targetBase=0, nTargets=2, weights=face.BAR_DEFAULT),
                              dict(node=face.COLLAR_NODE, targetBase=2, nTargets=1, weights=face.COLLAR_NODE_DEFAULT)]


def test_weights_channels_are_sampled(prepared):
    d, rod, box, sc, info, js, listed, rows, deltas = prepared
    at = dict(zip(TIMES, js["samples"]))
    for t, want in ((-1.0, [0, 0]), (0.0, [0, 0]), (0.5, [0.5, 0.25]), (1.0, [1, 0.5]), (1.5, [0.5, 0.75]), (2.0, [0, 1]), (3.0, [0, 1])):
        assert at[t][face.BAR_NODE]["weights"] == want, t                # LINEAR: the keys, between them, and the ends held
    assert np.allclose(at[0.99][face.BAR_NODE]["weights"], [0.99, 0.495], rtol=0, atol=1e-15)
    for t, want in ((-1.0, 0), (0.0, 0), (0.5, 0), (0.99, 0), (1.0, 1), (1.5, 1), (3.0, 1)):
        assert at[t][face.COLLAR_NODE]["weights"] == face.COLLAR_KEYS[want], t   # STEP: the key at or before t
    # what sample() returns otherwise is unchanged: the joints' channels, and no `weights` on a node without targets
    assert at[1.0][bar.JOINT1]["rotation"] == bar.Q120 and at[1.0][bar.JOINT0]["translation"] == bar.KEY_T[1]
    assert at[0.5][0] == dict(translation=[0, 0, 0], rotation=[0, 0, 0, 1], scale=[1, 1, 1], matrix=None)
    assert "weights" not in at[0.5][bar.JOINT0]
    # an animation without weights channels: the defaults
    assert js["other"][face.BAR_NODE]["weights"] == face.BAR_DEFAULT and js["other"][face.COLLAR_NODE]["weights"] == face.COLLAR_NODE_DEFAULT


def test_morph_list_survives_the_reorder(prepared):
    d, rod, box, sc, info, js, listed, rows, deltas = prepared
    n_bar, n_box = len(rod["indices"]) // 3, len(box["indices"]) // 3
    assert len(listed) == n_bar + n_box and len(rows) == len(listed) + 1 and rows[0] == 0 and rows[-1] == len(deltas)
    assert np.all(np.diff(listed.astype(np.int64)) > 0)
    mat = sc.tris["material_index"][listed]
    assert np.array_equal(listed, np.flatnonzero((sc.tris["material_index"] == 2) | (sc.tris["material_index"] == 3)))
    # the file lists the bar's triangles segment by segment, bottom to top: the build's reorder has not kept that order
    low = np.min([sc.tris[f][listed[mat == 2], 1] for f in ("v0", "v1", "v2")], axis=0)
    assert (np.diff(low) < 0).any(), "the reorder left the bar's triangles in the file's order: nothing was tested"
    assert not deltas["reserved0"].any() and not deltas["reserved4"].any()
    assert js["plainHasMorph"] is False and js["sameBlobs"] is True          # the ride through the build leaves no trace in the blobs
    assert not sc.tris["_p5"].view(np.uint32).any() and not sc.tris["_p6"].any()
    lengths = np.diff(rows.astype(np.int64))
    for e, tri in enumerate(listed):
        t = deltas["target"][rows[e]:rows[e + 1]].tolist()
        if mat[e] == 3:
            assert t == [2]                                              # the collar's one target, behind the bar's two
            continue
        # the bar: "lean" (1) moves every triangle (none lies in the plane y = 0); "bulge" (0) those with a vertex at y >= 1 only:
        # its records of the lower triangles are all zero and were dropped
        ys = np.array([sc.tris[f][tri, 1] for f in ("v0", "v1", "v2")], np.float64) - bar.MESH_AT[1]
        assert t == ([0, 1] if (ys >= 1.0).any() else [1]), (e, ys)
    assert set(lengths.tolist()) == {1, 2}
    # the bar's deltas (a translated node: the upper 3 x 3 is the identity): a function of the uploaded vertex
    for e in np.flatnonzero(mat == 2):
        for r in range(rows[e], rows[e + 1]):
            for f, g, h in zip(("v0", "v1", "v2"), ("dv0", "dv1", "dv2"), ("dn0", "dn1", "dn2")):
                p = sc.tris[f][listed[e]].astype(np.float64) - np.array(bar.MESH_AT)
                if deltas["target"][r] == 1:
                    assert deltas[g][r].tolist() == [p[1] / 8.0, 0.0, 0.0] and not deltas[h][r].any()
                else:
                    up = p[1] >= 1.0
                    assert deltas[g][r].tolist() == ([p[0] / 2.0, 0.0, p[2] / 2.0] if up else [0.0, 0.0, 0.0])
                    # dn / |n| with n the file's float32 normal (x, 0, z) / |ring|, in double, one rounding
                    n = (np.array([p[0], 0.0, p[2]]) / np.linalg.norm([bar.HALF, bar.HALF])).astype(np.float32).astype(np.float64)
                    want = np.float32(0.25 / np.sqrt((n * n).sum())) if up else np.float32(0.0)
                    assert deltas[h][r].tolist() == [0.0, float(want), 0.0]


def test_world_space_deltas_under_a_rotated_scaled_node(prepared):
    """N = T R S with R a permutation and S = 0.5: a position delta dp arrives as (R * 0.5) dp; the normal matrix is 2 R, the local
    normals are unit axes, so a normal delta dn arrives as (2 R dn) / |2 R n| = R dn. The file's deltas are functions of the local
    position (dp = p / 4, dn = (p.x / 2, 0, 0)), and the local position of an uploaded vertex is N^-1 v: all exact in float64."""
    d, rod, box, sc, info, js, listed, rows, deltas = prepared
    N = face.collar_world()
    A, inv = N[:3, :3], np.linalg.inv(N)
    R = bar.quat_matrix(bar.Q120)[:3, :3]
    assert np.array_equal(A, R * 0.5) and not np.array_equal(R, np.eye(3))
    entries = np.flatnonzero(sc.tris["material_index"][listed] == 3)
    assert len(entries) == 12
    for e in entries:
        r = int(rows[e])
        assert rows[e + 1] == r + 1
        for f, g, h in zip(("v0", "v1", "v2"), ("dv0", "dv1", "dv2"), ("dn0", "dn1", "dn2")):
            local = (inv @ np.append(sc.tris[f][listed[e]].astype(np.float64), 1.0))[:3]
            assert np.array_equal(deltas[g][r].astype(np.float64), A @ (local / 4.0)), (e, f)
            assert np.array_equal(deltas[h][r].astype(np.float64), R @ np.array([local[0] / 2.0, 0.0, 0.0])), (e, f)
    assert deltas["dv0"][rows[entries[0]]].any()


def test_a_file_without_targets_returns_no_morph_fields(tmp_path):
    _build()
    synthetic_glb(tmp_path / "s.glb")
    sc, info = prepare(tmp_path / "s.glb", tmp_path / "out")
    assert "morphTargets" not in info and "morphs" not in info
    assert not os.path.exists(tmp_path / "out" / "morph_triangles.bin") and not os.path.exists(tmp_path / "out" / "morph_deltas.bin")
