"""A small room with two cameras for the glTF camera tests: a floor, an emissive panel and a box, a perspective camera under a
rotated, translated node and an orthographic camera two levels down a chain of rotated, translated nodes. The world matrices are
composed here in float64; a glTF camera looks down its node's -Z with +Y up.

Nodes: 0 floor, 1 panel, 2 box; 3 the perspective camera's node (translated, turned about (1, 2, 0.5)); 4 "rig" (translated, turned
about y) with child 5 "arm" (translated, turned about x) with child 6, the orthographic camera's node (translated, turned about z).
Camera 0 of the file is the perspective one, camera 1 the orthographic one, and node order agrees with that."""

from ptmi import glb_io, scenes
from test_gltf_host import mesh_of, quat, trs

YFOV, ASPECT, ZNEAR = 0.7, 1.5, 0.05
XMAG, YMAG = 2.4, 1.6
PERSPECTIVE_NODE, ORTHO_NODE = 3, 6

P_T, P_R = (0.4, 1.3, 3.1), quat((1.0, 2.0, 0.5), 0.35)
RIG_T, RIG_R = (0.2, 0.1, 0.3), quat((0.0, 1.0, 0.0), 0.25)
ARM_T, ARM_R = (0.1, 1.2, 2.4), quat((1.0, 0.0, 0.0), -0.2)
CAM_T, CAM_R = (0.05, 0.1, 0.5), quat((0.0, 0.0, 1.0), 0.15)


def write_scene(path):
    """writes the file; returns {camera index: world matrix (4, 4) float64}"""
    floor = scenes._quad((-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2), (0, 1, 0), 0)
    panel = scenes._quad((-0.5, 2.5, -0.5), (0.5, 2.5, -0.5), (0.5, 2.5, 0.5), (-0.5, 2.5, 0.5), (0, -1, 0), 0)
    box = scenes._box((0, 0.5, 0), (1, 1, 1), 0)
    materials = [
        {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1], "metallicFactor": 0, "roughnessFactor": 0.5}},
        {"emissiveFactor": [1, 0.9, 0.7], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}},
         "pbrMetallicRoughness": {"metallicFactor": 0, "roughnessFactor": 0.5}},
        {"pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.2, 0.2, 1], "metallicFactor": 0, "roughnessFactor": 0.4}},
    ]
    cameras = [{"type": "perspective", "name": "hero", "perspective": {"yfov": YFOV, "aspectRatio": ASPECT, "znear": ZNEAR}},
               {"type": "orthographic", "name": "elevation", "orthographic": {"xmag": XMAG, "ymag": YMAG, "znear": ZNEAR, "zfar": 50.0}}]
    nodes = [{"mesh": 0}, {"mesh": 1}, {"mesh": 2},
             {"camera": 0, "translation": list(P_T), "rotation": P_R, "name": "hero node"},
             {"translation": list(RIG_T), "rotation": RIG_R, "children": [5], "name": "rig"},
             {"translation": list(ARM_T), "rotation": ARM_R, "children": [6], "name": "arm"},
             {"camera": 1, "translation": list(CAM_T), "rotation": CAM_R, "name": "elevation node"}]
    glb_io.write_glb(path, [mesh_of(floor, 0), mesh_of(panel, 1), mesh_of(box, 2)], nodes, materials, cameras=cameras)
    return {0: trs(P_T, P_R), 1: trs(RIG_T, RIG_R) @ trs(ARM_T, ARM_R) @ trs(CAM_T, CAM_R)}


def basis_of(world):
    """position, forward, right, up of a camera with this world matrix"""
    R = world[:3, :3]
    return world[:3, 3], R @ (0.0, 0.0, -1.0), R @ (1.0, 0.0, 0.0), R @ (0.0, 1.0, 0.0)
