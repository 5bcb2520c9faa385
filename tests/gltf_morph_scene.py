"""A morphed file for the glTF morph tests: the two-bone bar of tests/gltf_skin_scene.py (floor, panel, skinned bar, two joints) whose
bar also has two morph targets, and a "collar" box with one target under a rotated (120 degrees about (1, 1, 1): a permutation matrix),
uniformly scaled (0.5) and translated node, which is not skinned. Every position, delta, weight and key is a binary fraction, so the
deltas in the uploaded space and the sampled weights at the keys are exact.

Bar, target 0 ("bulge"): the vertices at y >= 1 move outwards by half their (x, z), with a normal delta of (0, 0.25, 0): the lower
triangles' records are all zero and are dropped. Target 1 ("lean"): x grows by y / 8; no NORMAL. mesh.weights = [0.25, 0].
Collar, target 0: every vertex moves by a quarter of its local position, its normal delta is (local x / 2, 0, 0); mesh.weights = [1],
node.weights = [0.5], which wins.

Animation 0: the bar's joints as in gltf_skin_scene, the bar's weights LINEAR with keys at 0, 1, 2 s ([0, 0], [1, 0.5], [0, 1]) and
the collar's weight STEP with keys at 0 and 1 s ([0.5], [1]). Animation 1: one translation channel and no weights."""
import numpy as np

import gltf_skin_scene as bar
from ptmi import glb_io, scenes
from test_gltf_host import mesh_of

BAR_NODE, COLLAR_NODE = bar.BAR_NODE, 5
COLLAR_T, COLLAR_S = [0.0, 0.75, 0.25], 0.5
BAR_KEYS = [[0.0, 0.0], [1.0, 0.5], [0.0, 1.0]]
COLLAR_KEYS = [[0.5], [1.0]]
BAR_DEFAULT, COLLAR_MESH_DEFAULT, COLLAR_NODE_DEFAULT = [0.25, 0.0], [1.0], [0.5]
N_TARGETS = 3                                           # the bar's two (targetBase 0), then the collar's one (targetBase 2)


def bar_targets(mesh):
    pos = mesh["positions"]
    upper = (pos[:, 1] >= 1.0)[:, None]
    bulge = np.where(upper, pos * np.array([0.5, 0.0, 0.5], np.float32), 0.0).astype(np.float32)
    bulge_n = np.where(upper, np.array([0.0, 0.25, 0.0], np.float32), 0.0).astype(np.float32) * np.ones_like(pos)
    lean = np.zeros_like(pos)
    lean[:, 0] = pos[:, 1] / 8.0
    return [{"positions": bulge, "normals": bulge_n}, {"positions": lean, "normals": None}]


def collar_target(mesh):
    pos = mesh["positions"]
    dn = np.zeros_like(pos)
    dn[:, 0] = pos[:, 0] / 2.0
    return [{"positions": (pos / 4.0).astype(np.float32), "normals": dn}]


def collar_world():
    """the collar node's world matrix (4 x 4, float64): T . R . S with R the permutation of bar.Q120"""
    return bar.translation(COLLAR_T) @ bar.quat_matrix(bar.Q120) @ np.diag([COLLAR_S, COLLAR_S, COLLAR_S, 1.0])


def write_face(path):
    floor = scenes._quad((-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2), (0, 1, 0), 0)
    panel = scenes._quad((-0.5, 2.5, -0.5), (0.5, 2.5, -0.5), (0.5, 2.5, 0.5), (-0.5, 2.5, 0.5), (0, -1, 0), 0)
    materials = [
        {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.5}},
        {"emissiveFactor": [1, 0.9, 0.7], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}},
         "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 0.5}},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.2, 0.2, 1], "metallicFactor": 0, "roughnessFactor": 0.4}},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.3, 0.9, 1], "metallicFactor": 0, "roughnessFactor": 0.6}},
    ]
    rod = bar.bar_mesh(2)
    rod["targets"], rod["morph_weights"] = bar_targets(rod), BAR_DEFAULT
    box = mesh_of(scenes._box((0, 0, 0), (1, 1, 1), 0), 3)
    box["targets"], box["morph_weights"] = collar_target(box), COLLAR_MESH_DEFAULT
    nodes = [{"mesh": 0}, {"mesh": 1}, {"mesh": 2, "skin": 0, "translation": list(bar.MESH_AT), "name": "bar"},
             {"translation": list(bar.MESH_AT), "children": [bar.JOINT1], "name": "lower"}, {"translation": [0.0, 1.0, 0.0], "name": "upper"},
             {"mesh": 3, "translation": COLLAR_T, "rotation": bar.Q120, "scale": [COLLAR_S] * 3, "name": "collar",
              "weights": COLLAR_NODE_DEFAULT}]
    mesh_world = bar.translation(bar.MESH_AT)
    ibm = [np.linalg.inv(bar.translation(bar.MESH_AT)) @ mesh_world, np.linalg.inv(bar.translation(np.add(bar.MESH_AT, (0, 1, 0)))) @ mesh_world]
    skins = [{"joints": [bar.JOINT0, bar.JOINT1], "inverseBindMatrices": np.array([m.T.reshape(16) for m in ibm])}]
    animations = [
        {"samplers": [{"input": [0.0, 1.0, 2.0], "output": [[0, 0, 0, 1], bar.Q120, [0, 0, 0, 1]], "interpolation": "LINEAR"},
                      {"input": [0.0, 1.0], "output": list(bar.KEY_T), "interpolation": "STEP"},
                      {"input": [0.0, 2.0], "output": list(bar.KEY_S), "interpolation": "LINEAR"},
                      {"input": [0.0, 1.0, 2.0], "output": BAR_KEYS, "interpolation": "LINEAR", "scalar": True},
                      {"input": [0.0, 1.0], "output": COLLAR_KEYS, "interpolation": "STEP", "scalar": True}],
         "channels": [{"node": bar.JOINT1, "path": "rotation", "sampler": 0}, {"node": bar.JOINT0, "path": "translation", "sampler": 1},
                      {"node": bar.JOINT1, "path": "scale", "sampler": 2}, {"node": BAR_NODE, "path": "weights", "sampler": 3},
                      {"node": COLLAR_NODE, "path": "weights", "sampler": 4}]},
        {"samplers": [{"input": [0.0, 1.0], "output": list(bar.KEY_T), "interpolation": "LINEAR"}],
         "channels": [{"node": bar.JOINT0, "path": "translation", "sampler": 0}]},
    ]
    glb_io.write_glb(path, [mesh_of(floor, 0), mesh_of(panel, 1), rod, box], nodes, materials, skins=skins, animations=animations)
    return rod, box
