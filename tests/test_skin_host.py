"""Skinning without a device (include/ptmi.h ptmi_set_skin, ptmi_pose_skin): the struct sizes, the calls' NULL-context answers, the
binding's joint_ops, and the model of tests/skin_ref.py: what it leaves alone, its positions against a float64 evaluation, and one-hot
weights against the model of the triangle groups byte for byte.

The bound of the float64 comparison, from the operation count. A position component is
    ((B[4k] p.x + B[4k+1] p.y) + B[4k+2] p.z) + B[4k+3],   B[e] = ((w0 J0[e] + w1 J1[e]) + w2 J2[e]) + w3 J3[e],
a sum of 16 elementary terms w_s * J_s[e] * p (p = 1 for the translation). Every float32 operation rounds its exact result by a factor
(1 + d), |d| <= u = 2^-24 (no operand here is near the denormals: see the magnitudes below). A term passes at most 8 roundings on its
way to the result: its product w * J (1), the three additions of the blend (3), the product with p (1) and the three additions of the
row (3). So the computed value is the exact sum with every term scaled by at most (1 + u)^8, and
    |computed - exact| <= gamma_8 * A,   gamma_8 = 8 u / (1 - 8 u),   A = sum over the 16 terms of |w_s| |J_s[e]| |p|
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1). `exact` is the same expression evaluated in float64 on the float32
inputs; its own error, 8 * 2^-53 A, is nine binary orders below the bound and is covered by evaluating the bound with 8.001 u."""
import ctypes
import os
import subprocess

import numpy as np

import skin_ref as ref
import transform_ref as tref
from ptmi import layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes(tmp_path):
    from ptmi import native
    assert ctypes.sizeof(native.SkinCorner) == 32 == layout.SKIN_CORNER.itemsize
    assert ctypes.sizeof(native.SkinStatus) == 32
    assert native.JOINT_TRANSFORM.itemsize == 96 == ctypes.sizeof(native.JointTransform)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptmi_skin_corner), sizeof(struct ptmi_skin_status),\n'
                   'sizeof(ptmi_joint_transform), offsetof(ptmi_skin_corner, weight), offsetof(struct ptmi_skin_status, poses),\n'
                   'offsetof(struct ptmi_skin_status, first_bad), offsetof(struct ptmi_skin_status, pose_ms));\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 32, 96, native.SkinCorner.weight.offset, native.SkinStatus.poses.offset, native.SkinStatus.first_bad.offset,
                   native.SkinStatus.pose_ms.offset]
    assert layout.SKIN_CORNER.fields["weight"][1] == got[3]


def test_calls_without_a_context_are_refused():
    """a NULL handle is PTMI_E_INVALID for every new entry point"""
    from ptmi import native
    L = native.load()
    t = np.zeros(1, np.uint32)
    c = ref.one_hot([0])
    j = native.joint_ops([(tref.affine(), None)])
    st = native.SkinStatus()
    assert L.ptmi_set_skin(None, native._p(t), native._p(c), 1, 1) == -1
    assert L.ptmi_pose_skin(None, native._p(j), 1) == -1
    assert L.ptmi_skin_status(None, ctypes.byref(st)) == -1
    assert L.ptmi_multi_set_skin(None, native._p(t), native._p(c), 1, 1) == -1
    assert L.ptmi_multi_pose_skin(None, native._p(j), 1) == -1
    assert L.ptmi_multi_skin_status(None, ctypes.byref(st)) == -1


def test_joint_ops_derives_the_normal_matrix():
    from ptmi import native
    m = tref.affine(tref.rot_y(0.4), scale=(3, 0.5, 1), shift=(1, 2, 3))
    rec = native.joint_ops([(m, None), (tref.affine(), np.arange(9)), (m, None)])
    assert rec.dtype == native.JOINT_TRANSFORM
    assert rec["group"].tolist() == [0, 1, 2] and rec["reserved0"].tolist() == [0, 0, 0] and rec["reserved1"].tolist() == [0, 0, 0]
    assert rec["m"][0].tobytes() == m.tobytes() and rec["nm"][2].tobytes() == tref.normal_matrix(m).tobytes()
    assert rec["nm"][1].tolist() == list(range(9))
    assert native.joint_ops(rec) is rec or native.joint_ops(rec).tobytes() == rec.tobytes()
    M, NM = ref.joint_arrays(rec)
    M2, NM2 = ref.joint_arrays([(m, None), (tref.affine(), np.arange(9)), (m, None)])
    assert M.tobytes() == M2.tobytes() and NM.tobytes() == NM2.tobytes()


def _skin_of(s, seed, n_joints, fraction):
    rng = np.random.default_rng(seed)
    n = len(s.tris)
    listed = np.sort(rng.choice(n, max(1, int(n * fraction)), replace=False)).astype(np.uint32)
    return listed, ref.random_corners(rng, len(listed), n_joints)


def test_model_leaves_everything_else_alone():
    from ptmi import scenes
    s = scenes.make("cornell")
    listed, corners = _skin_of(s, 21, 3, 0.4)
    joints = [(tref.affine(tref.rot_y(0.2 * k), shift=(0.1 * k, 0, 0)), None) for k in range(3)]
    out = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    other = np.ones(len(s.tris), bool)
    other[listed] = False
    assert other.any() and out[other].tobytes() == s.tris[other].tobytes()
    for f in s.tris.dtype.names:
        if f not in tref.REST_FIELDS:
            assert out[f].tobytes() == s.tris[f].tobytes(), f                # uvs, material_index, padding
    for f in tref.REST_FIELDS:
        assert not np.array_equal(out[f][listed], s.tris[f][listed]), f
    assert ref.first_bad(s.tris, tref.rest_of(s.tris), listed, corners, joints, True) == ref.NONE
    # a scale of 1e38 on ten times cornell's coordinates overflows every listed triangle: the first of the list is the smallest
    big = s.tris.copy()
    for f in ("v0", "v1", "v2"):
        big[f] *= np.float32(10.0)
    huge = [(tref.affine(scale=(1e38, 1e38, 1e38)), np.eye(3))] * 3
    assert ref.first_bad(big, tref.rest_of(big), listed, corners, huge, True) == int(listed[0])


def test_model_positions_against_float64():
    rng = np.random.default_rng(22)
    n, n_joints = 3000, 9
    p = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-2, 3, size=(n, 1))).astype(np.float32)
    u = 2.0 ** -24
    for trial in range(40):
        M = (rng.normal(size=(n_joints, 12)) * 10.0 ** rng.integers(-3, 4, size=(n_joints, 1))).astype(np.float32)
        corner = ref.random_corners(rng, n // 3, n_joints, influences=1 + trial % 4)
        if trial % 5 == 0:                                                   # weights as given: negative and unnormalised ones too
            corner["weight"] = rng.normal(size=(n, 4)).astype(np.float32)
        got = ref.point_rows(ref.blend(M, corner), p).astype(np.float64)
        w = corner["weight"].astype(np.float64)                              # (n, 4)
        Jm = M.astype(np.float64)[corner["joint"]]                           # (n, 4, 12)
        terms = w[:, :, None] * Jm                                           # w_s * J_s[e]
        B, Babs = terms.sum(axis=1).reshape(n, 3, 4), np.abs(terms).sum(axis=1).reshape(n, 3, 4)
        p1 = np.concatenate([p.astype(np.float64), np.ones((n, 1))], axis=1)
        exact = (B * p1[:, None, :]).sum(axis=2)
        A = (Babs * np.abs(p1)[:, None, :]).sum(axis=2)
        bound = 8.001 * u / (1.0 - 8.0 * u) * A
        assert np.all(np.abs(got - exact) <= bound), (trial, (np.abs(got - exact) / (u * A)).max())


def test_one_hot_weights_reproduce_the_group_transform():
    """weights (1, 0, 0, 0): B = (1 * J[j] + 0 * J[0]) + 0 * J[0] + 0 * J[0] is J[j] entry for entry unless an entry of J[j] is a
    negative zero (-0 + +0 = +0 would lose its sign), so the matrices here hold none, which is asserted"""
    from ptmi import scenes
    s = scenes.make("cornell")
    groups = np.random.default_rng(23).integers(0, 4, len(s.tris)).astype(np.uint32)
    ms = [tref.affine(tref.rot_y(0.4), shift=(0.05, 0.02, -0.03)), tref.affine(scale=(3, 0.5, 1)),
          tref.affine(scale=(-1, 1, 1), shift=(0.1, 0, 0)), tref.affine(tref.rot_y(-1.1), scale=(1, 2, 1))]
    ops = [(g,) + ref.joint(m) for g, m in enumerate(ms)]                     # (the mirror's cofactors hold negative zeros: joint() clears them)
    assert any(np.signbit(tref.normal_matrix(m)[tref.normal_matrix(m) == 0]).any() for m in ms)
    for _, m, nm in ops:
        assert not np.signbit(m[m == 0]).any() and not np.signbit(nm[nm == 0]).any()
    listed = np.arange(len(s.tris), dtype=np.uint32)
    joints = [(m, nm) for _, m, nm in ops]
    rest = tref.rest_of(s.tris)
    got = ref.skinned(s.tris, rest, listed, ref.one_hot(groups), joints)
    assert got.tobytes() == tref.transformed(s.tris, rest, groups, ops).tobytes()
    # and the per-row formulas are the per-matrix ones: the same bytes for a constant matrix
    m, nm = ops[0][1], ops[0][2]
    assert ref.point_rows(np.tile(m, (len(listed), 1)), s.tris["v1"]).tobytes() == tref.point(m, s.tris["v1"]).tobytes()
    assert ref.normal_rows(np.tile(nm, (len(listed), 1)), s.tris["n1"]).tobytes() == tref.normal(nm, s.tris["n1"]).tobytes()
