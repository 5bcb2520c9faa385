"""The glTF loader's triangle groups (host/scene_prep.js): every triangle is tagged with the index of the node it came from, the tag
rides through the BVH build's reorder in the record's last padding word, and the blobs come out as the bytes they are without tags."""
import json
import os
import subprocess

import numpy as np
import pytest

from ptmi import glb_io, scenes
from test_gltf_host import HOST, NODE, _build, mesh_of, prepare, synthetic_glb

pytestmark = pytest.mark.skipif(NODE is None, reason="node is not installed")

UNTAGGED = """
var fs = require('fs'), path = require('path');
var s = require(%(prep)s).prepareScene(require(%(gltf)s).loadGLB(%(glb)s), { triangleGroups: false });
Object.keys(s.blobs).forEach(function (k) { fs.writeFileSync(path.join(%(out)s, k + '.bin'), Buffer.from(s.blobs[k])); });
console.log(JSON.stringify({ groups: s.triangleGroups === undefined, names: s.groupNames === undefined }));
"""


def untagged(glb, out):
    """the blobs of the path without tags: prepareScene(..., { triangleGroups: false }) never writes the padding word"""
    os.makedirs(out, exist_ok=True)
    script = os.path.join(out, "untagged.js")
    with open(script, "w") as f:
        f.write(UNTAGGED % dict(prep=json.dumps(os.path.join(HOST, "scene_prep.js")), gltf=json.dumps(os.path.join(HOST, "gltf.js")),
                                glb=json.dumps(str(glb)), out=json.dumps(str(out))))
    info = json.loads(subprocess.check_output([NODE, script], text=True).strip().splitlines()[-1])
    assert info == {"groups": True, "names": True}
    return {k: open(os.path.join(out, k + ".bin"), "rb").read() for k in ("triangles", "materials", "bvhNodes", "lights")}


def test_two_node_scene_groups_are_each_nodes_triangles(tmp_path):
    _build()
    box = scenes._box((0, 0, 0), (1, 1, 1), 0)
    sph = scenes._uv_sphere((0, 0, 0), 0.5, 0, segments=10, rings=6)
    centre = np.array([0.5, 0.5, -0.2])
    nodes = [{"name": "crate", "mesh": 0, "translation": [0.3, 0.0, 0.1]}, {"mesh": 1, "translation": centre.tolist()}]
    glb_io.write_glb(tmp_path / "two.glb", [mesh_of(box, 0), mesh_of(sph, 0)], nodes,
                     [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.5}}], [])
    sc, info = prepare(tmp_path / "two.glb", tmp_path / "out")
    groups = np.fromfile(tmp_path / "out" / "triangle_groups.bin", np.uint32)
    assert len(groups) == len(sc.tris) == len(box) + len(sph) and info["groupNames"] == ["crate", "node1"]
    assert (groups == 0).sum() == len(box) and (groups == 1).sum() == len(sph)
    # one material per primitive in node order: here a triangle's material index is its node's index, whatever the reorder did
    assert np.array_equal(groups, sc.tris["material_index"])
    assert not np.all(np.diff(groups.astype(np.int64)) >= 0), "the reorder left the nodes' triangles in two runs: nothing was tested"
    # members by position: the sphere's triangles are those whose three vertices lie 0.5 from its centre
    on_sphere = np.all([np.abs(np.linalg.norm(sc.tris[f] - centre, axis=1) - 0.5) < 1e-5 for f in ("v0", "v1", "v2")], axis=0)
    assert np.array_equal(on_sphere, groups == 1)
    assert not sc.tris["_p6"].any()
    plain = untagged(tmp_path / "two.glb", tmp_path / "plain")
    for k in plain:
        assert open(tmp_path / "out" / (k + ".bin"), "rb").read() == plain[k], k


def test_synthetic_hierarchy_blobs_are_the_untagged_bytes(tmp_path):
    _build()
    meshes, nodes, world = synthetic_glb(tmp_path / "s.glb")
    sc, info = prepare(tmp_path / "s.glb", tmp_path / "out")
    groups = np.fromfile(tmp_path / "out" / "triangle_groups.bin", np.uint32)
    assert len(info["groupNames"]) == len(nodes) and not sc.tris["_p6"].any()
    for mat_index, node_i in enumerate([0, 1, 4, 5, 6]):         # one material per primitive, in node order
        assert np.array_equal(groups == node_i, sc.tris["material_index"] == mat_index)
    plain = untagged(tmp_path / "s.glb", tmp_path / "plain")
    for k in plain:
        assert open(tmp_path / "out" / (k + ".bin"), "rb").read() == plain[k], k
