"""The glTF loader's skin (host/gltf.js, host/scene_prep.js, host/animation.js): a skinned primitive's triangles are listed in the
uploaded order with their corners' joints and normalised weights, the pre-sort index that carries them through the BVH build's
reorder leaves no trace in the blobs, animations are sampled (STEP, LINEAR, slerp), and the joint matrices of the file's own pose map
the rest pose onto itself. The file is tests/gltf_skin_scene.py's two-bone bar."""
import json
import os
import subprocess

import numpy as np
import pytest

import gltf_skin_scene as bar
from ptmi import layout
from test_gltf_host import HOST, NODE, _build, prepare, synthetic_glb

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

SCRIPT = """
var fs = require('fs'), path = require('path');
var prep = require(%(prep)s), anim = require(%(anim)s), gltf = require(%(gltf)s).loadGLB(%(glb)s);
var plain = prep.prepareScene(gltf, { skins: false });
Object.keys(plain.blobs).forEach(function (k) { fs.writeFileSync(path.join(%(out)s, k + '.bin'), Buffer.from(plain.blobs[k])); });
var s = prep.prepareScene(gltf);
var info = { plainHasSkin: plain.skinTriangles !== undefined || plain.skins !== undefined, skinJoints: s.skinJoints,
  skins: s.skins.map(function (k) { return { node: k.node, joints: k.joints, jointBase: k.jointBase, meshWorldInverse: k.meshWorldInverse }; }),
  nSkins: gltf.skins.length, nAnimations: gltf.animations.length, ibm: Array.from(gltf.skins[0].inverseBindMatrices) };
info.samples = %(times)s.map(function (t) { return anim.sample(gltf, 0, t); });
try { anim.sample(gltf, 1, 0.5); info.cubic = 'no error'; } catch (e) { info.cubic = String(e.message); }
try { anim.sample(gltf, 7, 0.5); info.missing = 'no error'; } catch (e) { info.missing = String(e.message); }
info.ownPose = prep.skinPose(s, anim.worldMatrices(gltf, anim.restPose(gltf)));
info.posed = prep.skinPose(s, anim.worldMatrices(gltf, anim.sample(gltf, 0, 1.0)));
console.log(JSON.stringify(info));
"""
TIMES = [-1.0, 0.0, 0.5, 0.99, 1.0, 1.5, 2.0, 3.0]


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    _build()
    d = tmp_path_factory.mktemp("bar")
    mesh = bar.write_bar(d / "bar.glb")
    sc, info = prepare(d / "bar.glb", d / "out")
    os.makedirs(d / "plain")
    script = d / "skin.js"
    script.write_text(SCRIPT % dict(prep=json.dumps(os.path.join(HOST, "scene_prep.js")), anim=json.dumps(os.path.join(HOST, "animation.js")),
                                    gltf=json.dumps(os.path.join(HOST, "gltf.js")), glb=json.dumps(str(d / "bar.glb")),
                                    out=json.dumps(str(d / "plain")), times=json.dumps(TIMES)))
    js = json.loads(subprocess.check_output([NODE, str(script)], text=True).strip().splitlines()[-1])
    return d, mesh, sc, info, js


def test_skin_list_names_the_bars_triangles_in_uploaded_order(prepared):
    d, mesh, sc, info, js = prepared
    listed = np.fromfile(d / "out" / "skin_triangles.bin", np.uint32)
    corners = np.fromfile(d / "out" / "skin_corners.bin", layout.SKIN_CORNER).reshape(-1, 3)
    n_bar = len(mesh["indices"]) // 3
    assert len(listed) == n_bar == 64 and len(corners) == n_bar
    assert np.all(np.diff(listed.astype(np.int64)) > 0)
    # one material per primitive in node order: the bar's is 2, wherever the reorder put its triangles
    assert np.array_equal(listed, np.flatnonzero(sc.tris["material_index"] == 2))
    assert not np.array_equal(listed, np.arange(listed[0], listed[0] + n_bar)), "the reorder left the bar in one run: nothing was tested"
    assert info["skinJoints"] == 2 and info["skins"] == [dict(node=bar.BAR_NODE, skin=0, joints=[bar.JOINT0, bar.JOINT1], jointBase=0)]
    # corners follow their triangles: the file's weights rise with the height of the vertex, (1 - y / 2, y / 2) once normalised
    assert np.all(corners["joint"] == np.array([0, 1, 0, 0], np.uint32))
    for k, f in enumerate(("v0", "v1", "v2")):
        y = sc.tris[f][listed, 1].astype(np.float64) - bar.MESH_AT[1]
        assert np.array_equal(corners["weight"][:, k], np.stack([1 - y / 2, y / 2, 0 * y, 0 * y], axis=1).astype(np.float32)), f
    # normalised in double, then one rounding per weight: the float32 weights sum to 1 within two half-ulps of 1
    assert np.all(np.abs(corners["weight"].astype(np.float64).sum(axis=2) - 1.0) <= 2.0 ** -24)
    assert not sc.tris["_p5"].view(np.uint32).any() and not sc.tris["_p6"].any()


def test_blobs_are_the_bytes_of_the_file_with_skinning_ignored(prepared, tmp_path):
    d, mesh, sc, info, js = prepared
    assert js["plainHasSkin"] is False
    for k in ("triangles", "materials", "bvhNodes", "lights"):
        assert open(d / "out" / (k + ".bin"), "rb").read() == open(d / "plain" / (k + ".bin"), "rb").read(), k
    # ... and of the same geometry written without skin, joints, weights and animations
    bar.write_bar(tmp_path / "plain.glb", skinned=False)
    prepare(tmp_path / "plain.glb", tmp_path / "out")
    for k in ("triangles", "materials", "bvhNodes", "lights", "triangle_groups"):
        assert open(d / "out" / (k + ".bin"), "rb").read() == open(tmp_path / "out" / (k + ".bin"), "rb").read(), k


def test_a_file_without_skins_returns_no_skin_fields(tmp_path):
    _build()
    synthetic_glb(tmp_path / "s.glb")
    sc, info = prepare(tmp_path / "s.glb", tmp_path / "out")
    assert "skinJoints" not in info and "skins" not in info
    assert not os.path.exists(tmp_path / "out" / "skin_triangles.bin") and not os.path.exists(tmp_path / "out" / "skin_corners.bin")


def test_animation_samples(prepared):
    d, mesh, sc, info, js = prepared
    assert js["nSkins"] == 1 and js["nAnimations"] == 2
    at = dict(zip(TIMES, js["samples"]))
    ident = [0, 0, 0, 1]
    for t, want in ((-1.0, ident), (0.0, ident), (1.0, bar.Q120), (2.0, ident), (3.0, ident)):    # keys, and the ends held
        assert at[t][bar.JOINT1]["rotation"] == want, t
    # midway between identity and 120 degrees about (1, 1, 1): 60 degrees about it. The keys are exact and the interpolation is in
    # double: a few units of 2^-53 from the sines and the normalisation, far inside 1e-12
    half = [np.sin(np.pi / 6) / np.sqrt(3)] * 3 + [np.cos(np.pi / 6)]
    assert np.allclose(at[0.5][bar.JOINT1]["rotation"], half, rtol=0, atol=1e-12)
    assert np.allclose(at[1.5][bar.JOINT1]["rotation"], half, rtol=0, atol=1e-12)
    assert abs(np.linalg.norm(at[0.5][bar.JOINT1]["rotation"]) - 1.0) <= 1e-15
    for t, want in ((-1.0, 0), (0.0, 0), (0.5, 0), (0.99, 0), (1.0, 1), (1.5, 1), (3.0, 1)):      # STEP: the key at or before t
        assert at[t][bar.JOINT0]["translation"] == bar.KEY_T[want], t
    for t, want in ((0.0, 1.0), (0.5, 1.25), (1.0, 1.5), (2.0, 2.0), (3.0, 2.0)):                 # LINEAR
        assert at[t][bar.JOINT1]["scale"] == [1.0, want, 1.0], t
    # what no channel targets keeps the node's own transform
    assert at[0.5][bar.JOINT1]["translation"] == [0, 1, 0] and at[0.5][bar.BAR_NODE]["translation"] == list(bar.MESH_AT)
    assert at[0.5][0] == dict(translation=[0, 0, 0], rotation=ident, scale=[1, 1, 1], matrix=None)
    assert "CUBICSPLINE" in js["cubic"] and "not supported" in js["cubic"]
    assert "no animation 7" in js["missing"]


def test_the_files_own_pose_maps_the_rest_pose_onto_itself(prepared):
    """D_j = jointWorld_j . inverseBind_j . meshWorld^-1 composed in double, then one rounding to float32. Every factor of this
    file is a translation by binary fractions, so the products and the inverse are exact in double and D_j is the identity exactly;
    in general each of the two products and the inverse adds a few units of 2^-53 times the magnitudes (at most 4 here), and the
    rounding to float32 at most 2^-24 of an entry: |D - I| <= 2^-24 + 2^-45 per entry, which is what is asserted. A rest position r
    (|r| <= 2.5 per coordinate here) then moves by at most 4 entries' worth: 4 * 2.5 * (2^-24 + 2^-45)."""
    d, mesh, sc, info, js = prepared
    eps = 2.0 ** -24 + 2.0 ** -45
    listed = np.fromfile(d / "out" / "skin_triangles.bin", np.uint32)
    assert len(js["ownPose"]) == 2
    for j in js["ownPose"]:
        m = np.array(j["matrix"], np.float64).astype(np.float32).astype(np.float64).reshape(3, 4)
        assert np.all(np.abs(m - np.eye(4)[:3]) <= eps)
        for f in ("v0", "v1", "v2"):
            r = sc.tris[f][listed].astype(np.float64)
            assert np.all(np.abs(r @ m[:, :3].T + m[:, 3] - r) <= 4 * 2.5 * eps)
    assert np.array_equal(np.array(js["skins"][0]["meshWorldInverse"]).reshape(4, 4).T, np.linalg.inv(bar.translation(bar.MESH_AT)))
    # at the key at 1 s the matrices are the float64 model's (exact factors: the permutation rotation, binary fractions)
    want = bar.joint_matrices(bar.KEY_T[1], bar.Q120, [1.0, 1.5, 1.0])
    for j, w in zip(js["posed"], want):
        assert np.array_equal(np.array(j["matrix"], np.float64), w)
