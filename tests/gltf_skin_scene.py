"""A two-bone bar for the glTF skin tests: a square bar of 8 segments along +y under a skinned mesh node, a floor, an emissive panel
and a box around the bar's middle that are not skinned (the box makes the BVH build's reorder cut the bar's triangles into runs),
two joints (the second a child of the first, one unit up), and two animations. Every position, weight, translation and key in the
file is exactly representable in float32 and so are the joints' world matrices and their inverses, so the double composition of the
joint matrices is exact at the keys the tests pose at.

Animation 0: the upper joint's rotation, LINEAR, keys at 0, 1, 2 s (identity; 120 degrees about (1, 1, 1), the quaternion
(0.5, 0.5, 0.5, 0.5), whose matrix is a permutation; identity), the lower joint's translation, STEP, keys at 0 and 1 s, and the upper
joint's scale, LINEAR, keys at 0 and 2 s. Animation 1: one CUBICSPLINE channel."""
import numpy as np

from ptmi import glb_io, scenes
from test_gltf_host import mesh_of

SEGMENTS, HALF, HEIGHT = 8, 0.125, 2.0
MESH_AT = (0.25, 0.0, 0.5)
Q120 = [0.5, 0.5, 0.5, 0.5]
KEY_T = [0.25, 0.0, 0.5], [0.5, 0.0, 0.5]
KEY_S = [1.0, 1.0, 1.0], [1.0, 2.0, 1.0]
BAR_NODE, JOINT0, JOINT1 = 2, 3, 4


def bar_mesh(material):
    """indexed: four vertices per ring, two triangles per side and segment; weights (unnormalised: they sum to 0.5) rise with y"""
    ring = np.array([[-HALF, -HALF], [HALF, -HALF], [HALF, HALF], [-HALF, HALF]])
    ys = np.linspace(0.0, HEIGHT, SEGMENTS + 1)
    pos = np.array([[x, y, z] for y in ys for x, z in ring], np.float32)
    nrm = np.array([[x, 0.0, z] for _ in ys for x, z in ring / np.linalg.norm(ring[0])], np.float32)
    idx = []
    for s in range(SEGMENTS):
        for k in range(4):
            a, b = 4 * s + k, 4 * s + (k + 1) % 4
            idx += [a, b, b + 4, a, b + 4, a + 4]
    w1 = pos[:, 1] / HEIGHT
    weights = np.stack([0.5 * (1.0 - w1), 0.5 * w1, np.zeros_like(w1), np.zeros_like(w1)], axis=1)
    joints = np.tile(np.array([0, 1, 0, 0], np.uint16), (len(pos), 1))
    return {"positions": pos, "normals": nrm, "uvs": None, "indices": np.array(idx), "material": material,
            "joints": joints, "weights": weights}


def translation(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def write_bar(path, skinned=True):
    floor = scenes._quad((-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2), (0, 1, 0), 0)
    panel = scenes._quad((-0.5, 2.5, -0.5), (0.5, 2.5, -0.5), (0.5, 2.5, 0.5), (-0.5, 2.5, 0.5), (0, -1, 0), 0)
    materials = [
        {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.5}},
        {"emissiveFactor": [1, 0.9, 0.7], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}},
         "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 0.5}},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.2, 0.2, 1], "metallicFactor": 0, "roughnessFactor": 0.4}},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.3, 0.9, 1], "metallicFactor": 0, "roughnessFactor": 0.6}},
    ]
    box = scenes._box((0, 0, 0), (1, 1, 1), 0)
    bar = bar_mesh(2)
    nodes = [{"mesh": 0}, {"mesh": 1}, {"mesh": 2, "skin": 0, "translation": list(MESH_AT), "name": "bar"},
             {"translation": list(MESH_AT), "children": [JOINT1], "name": "lower"}, {"translation": [0.0, 1.0, 0.0], "name": "upper"},
             {"mesh": 3, "translation": [0.0, 0.75, 0.25], "scale": [0.5, 0.5, 0.5], "name": "collar"}]
    # inverseBind_j = jointWorld_j^-1 . meshWorld at the bind pose, column-major in the file
    mesh_world = translation(MESH_AT)
    ibm = [np.linalg.inv(translation(MESH_AT)) @ mesh_world, np.linalg.inv(translation(np.add(MESH_AT, (0, 1, 0)))) @ mesh_world]
    skins = [{"joints": [JOINT0, JOINT1], "inverseBindMatrices": np.array([m.T.reshape(16) for m in ibm])}]
    animations = [
        {"samplers": [{"input": [0.0, 1.0, 2.0], "output": [[0, 0, 0, 1], Q120, [0, 0, 0, 1]], "interpolation": "LINEAR"},
                      {"input": [0.0, 1.0], "output": list(KEY_T), "interpolation": "STEP"},
                      {"input": [0.0, 2.0], "output": list(KEY_S), "interpolation": "LINEAR"}],
         "channels": [{"node": JOINT1, "path": "rotation", "sampler": 0}, {"node": JOINT0, "path": "translation", "sampler": 1},
                      {"node": JOINT1, "path": "scale", "sampler": 2}]},
        {"samplers": [{"input": [0.0, 1.0], "output": np.zeros((6, 3)), "interpolation": "CUBICSPLINE"}],
         "channels": [{"node": JOINT0, "path": "translation", "sampler": 0}]},
    ]
    if not skinned:
        for k in ("joints", "weights"):
            del bar[k]
        del nodes[BAR_NODE]["skin"]
        skins = animations = None
    glb_io.write_glb(path, [mesh_of(floor, 0), mesh_of(panel, 1), bar, mesh_of(box, 3)], nodes, materials, skins=skins, animations=animations)
    return bar


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 0],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w), 0],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y), 0], [0, 0, 0, 1.0]])


def joint_matrices(t_lower, q_upper, s_upper):
    """the device matrices (3 x 4 row-major, 12 numbers each) of the two joints for the lower joint's translation and the upper
    joint's rotation and scale, in float64: jointWorld . inverseBind . meshWorld^-1"""
    mesh_inv = np.linalg.inv(translation(MESH_AT))
    w0 = translation(t_lower)
    w1 = w0 @ translation((0, 1, 0)) @ quat_matrix(q_upper) @ np.diag([*s_upper, 1.0])
    ibm = [np.eye(4), translation((0, -1, 0))]
    return [(w @ b @ mesh_inv)[:3].reshape(12) for w, b in zip((w0, w1), ibm)]
