"""Triangle groups without a device (include/ptmi.h ptmi_normal_matrix, ptmi_group_transform): the host function against the model of
tests/transform_ref.py bit for bit, the model against a float64 evaluation, the struct sizes, and the calls' NULL-context answers.

Bounds. A position component is ((t1 + t2) + t3) + t4 with t1..t3 rounded products and t4 the translation. "The largest term" is
taken over the operands of the three additions: t1, t2, t3, t4 and the partial sums s1 = t1 + t2 and s2 = s1 + t3, with T their
largest magnitude. Each product is off by at most 0.5 ulp(T) (1.5 together), the roundings of s1 and s2 by at most 0.5 ulp(T) each
(they are operands themselves), and the result is at most 2 T in magnitude, so its rounding is at most 0.5 ulp(2 T) = 1 ulp(T): 3.5
ulp(T) in all, inside the 4 ulp the check allows. (Against the largest of the four addends t1..t4 alone no constant below 6.5 holds:
equal-signed addends of equal size make the partial sums up to four times as large.)
A unit normal: l2 sums three non-negative squares, so its three roundings plus the squares' leave a relative error of at most about
2 * 2^-24 on l2 and 2^-24 on the root; the root's own rounding and the quotients' add 2^-24 each. The length is off from 1 by less
than 3.5 * 2^-24 < 2 ulp of 1 (2 * 2^-23)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import transform_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrices():
    rng = np.random.default_rng(5)
    ms = [ref.affine(shift=rng.normal(size=3)) for _ in range(2)]
    ms += [(rng.normal(size=12) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(1000)]
    ms += [ref.affine(ref.rot_y(a), shift=(0.1, -2, 3)) for a in (0.0, 0.3, 1.5707963, 3.1, -2.2)]
    ms += [ref.affine(scale=s) for s in ((3, 0.5, 1), (1e-3, 1e3, 7), (1e19, 1e19, 1e-19))]
    ms += [ref.affine(scale=s) for s in ((-1, 1, 1), (1, -1, 1), (-1, -1, -1))]                     # mirrors
    ms += [ref.affine(scale=(1, 0, 1)), ref.affine(scale=(0, 0, 0)), np.ones(12, np.float32)]      # singular
    return ms


def test_normal_matrix_equals_the_model_bit_for_bit():
    from ptmi import native
    for m in _matrices():
        got, want = native.normal_matrix(m), ref.normal_matrix(m)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (m, got, want)


def test_normal_matrix_is_the_cofactor_matrix():
    """cof(A) = det(A) A^-T: rotations map to themselves, a mirror flips the sign, a non-uniform scale gives the inverse scales times det"""
    from ptmi import native
    r = ref.affine(ref.rot_y(0.7))
    assert np.allclose(native.normal_matrix(r).reshape(3, 3), r.reshape(3, 4)[:, :3], atol=1e-6)
    assert np.array_equal(native.normal_matrix(ref.affine(scale=(3, 0.5, 1))).reshape(3, 3), np.diag([0.5, 3, 1.5]).astype(np.float32))
    assert np.array_equal(native.normal_matrix(ref.affine(scale=(-1, 1, 1))).reshape(3, 3), np.diag([1, -1, -1]).astype(np.float32))
    for m in _matrices()[2:200]:
        a = m.reshape(3, 4)[:, :3].astype(np.float64)
        if abs(np.linalg.det(a)) > 1e-3 * np.abs(a).max() ** 3:
            want = np.linalg.det(a) * np.linalg.inv(a).T
            assert np.allclose(native.normal_matrix(m).reshape(3, 3), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_model_positions_against_float64():
    rng = np.random.default_rng(6)
    p = (rng.normal(size=(4000, 3)) * 10.0 ** rng.integers(-2, 3, size=(4000, 1))).astype(np.float32)
    for m in _matrices()[:300]:
        got = ref.point(m, p).astype(np.float64)
        m64, p64 = m.astype(np.float64).reshape(3, 4), p.astype(np.float64)
        exact = p64 @ m64[:, :3].T + m64[:, 3]
        t = p64[:, None, :] * m64[None, :, :3]                   # (n, 3 rows, 3 products)
        s1 = t[:, :, 0] + t[:, :, 1]
        s2 = s1 + t[:, :, 2]
        operands = np.stack([t[:, :, 0], t[:, :, 1], t[:, :, 2], np.broadcast_to(m64[None, :, 3], s1.shape), s1, s2], axis=2)
        ulp = np.spacing(np.abs(operands).max(axis=2).astype(np.float32)).astype(np.float64)
        worst = (np.abs(got - exact) / ulp).max()
        assert worst <= 4.0, (m, worst)


def test_model_normals_are_unit_within_two_ulp():
    rng = np.random.default_rng(7)
    n = rng.normal(size=(4000, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    ms = _matrices()
    for m in ms[:300] + ms[-14:-3]:
        out = ref.normal(ref.normal_matrix(m), n).astype(np.float64)
        nm = ref.normal_matrix(m).astype(np.float64).reshape(3, 3)
        q = n.astype(np.float32)
        with np.errstate(all="ignore"):
            q32 = np.stack([(np.float32(nm[k, 0]) * q[:, 0] + np.float32(nm[k, 1]) * q[:, 1]) + np.float32(nm[k, 2]) * q[:, 2] for k in range(3)], axis=1)
            l2 = (q32[:, 0] * q32[:, 0] + q32[:, 1] * q32[:, 1]) + q32[:, 2] * q32[:, 2]
        ok = (l2 > 1e-30) & np.isfinite(l2)                     # (below that the squares are denormal and carry fewer bits)
        length = np.sqrt((out[ok] ** 2).sum(axis=1))
        assert np.all(np.abs(length - 1.0) <= 2 * 2.0 ** -23), (m, np.abs(length - 1.0).max())
    # l2 = 0: the normal is q itself
    zero = ref.normal(np.zeros(9, np.float32), n[:4])
    assert np.array_equal(zero, np.zeros((4, 3), np.float32))


def test_mirror_flips_the_normal_with_the_winding():
    n = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    out = ref.normal(ref.normal_matrix(ref.affine(scale=(-1, 1, 1))), n)
    assert np.array_equal(out, np.array([[0, 0, -1], [1, 0, 0]], np.float32))


def test_struct_sizes(tmp_path):
    from ptmi import native
    assert ctypes.sizeof(native.GroupTransform) == 96 == native.GROUP_TRANSFORM.itemsize
    assert ctypes.sizeof(native.TransformStatus) == 32
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ptmi_group_transform), sizeof(struct ptmi_transform_status),\n'
                   'offsetof(ptmi_group_transform, m), offsetof(ptmi_group_transform, nm), offsetof(ptmi_group_transform, reserved1),\n'
                   'offsetof(struct ptmi_transform_status, transform_ms));\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [96, 32, native.GroupTransform.m.offset, native.GroupTransform.nm.offset, native.GroupTransform.reserved1.offset,
                   native.TransformStatus.transform_ms.offset]
    assert [native.GROUP_TRANSFORM.fields[f][1] for f in ("m", "nm", "reserved1")] == got[2:5]


def test_calls_without_a_context_are_refused():
    """the validation the binding allows without a device: a NULL handle is PTMI_E_INVALID for every new entry point"""
    from ptmi import native
    L = native.load()
    g = np.zeros(4, np.uint32)
    ops = native.group_ops([(0, ref.affine())])
    st = native.TransformStatus()
    assert L.ptmi_set_triangle_groups(None, native._p(g), 4) == -1
    assert L.ptmi_transform_groups(None, native._p(ops), 1) == -1
    assert L.ptmi_transform_status(None, ctypes.byref(st)) == -1
    assert L.ptmi_debug_read_triangles(None, 0, 0, None) == -1
    assert L.ptmi_multi_set_triangle_groups(None, native._p(g), 4) == -1
    assert L.ptmi_multi_transform_groups(None, native._p(ops), 1) == -1
    assert L.ptmi_multi_transform_status(None, ctypes.byref(st)) == -1


def test_group_ops_derives_the_normal_matrix():
    from ptmi import native
    m = ref.affine(ref.rot_y(0.4), scale=(3, 0.5, 1), shift=(1, 2, 3))
    rec = native.group_ops([(7, m), (2, m, np.arange(9))])
    assert rec["group"].tolist() == [7, 2] and rec["reserved0"].tolist() == [0, 0] and rec["reserved1"].tolist() == [0, 0]
    assert rec["m"][0].tobytes() == m.tobytes() and rec["nm"][0].tobytes() == ref.normal_matrix(m).tobytes()
    assert rec["nm"][1].tolist() == list(range(9))


def test_model_leaves_everything_else_alone():
    from ptmi import scenes
    s = scenes.make("cornell")
    groups = s.tris["material_index"].astype(np.uint32)
    g = int(groups[0])
    out = ref.transformed(s.tris, ref.rest_of(s.tris), groups, [ref.op(g, ref.affine(shift=(0.5, 0, 0)))])
    other = groups != g
    assert out[other].tobytes() == s.tris[other].tobytes()
    for f in s.tris.dtype.names:
        if f not in ref.REST_FIELDS:
            assert out[f].tobytes() == s.tris[f].tobytes(), f
    assert np.array_equal(out["v0"][~other], ref.point(ref.affine(shift=(0.5, 0, 0)), s.tris["v0"][~other]))
    # a scale of 1e38 overflows every member whose largest coordinate exceeds 3.4: here, ten times cornell's, all of them
    big = s.tris.copy()
    for f in ("v0", "v1", "v2"):
        big[f] *= np.float32(10.0)
    huge = [ref.op(g, ref.affine(scale=(1e38, 1e38, 1e38)), np.eye(3))]
    assert ref.first_bad(big, ref.rest_of(big), groups, huge, True) == int(np.flatnonzero(~other)[0])
    assert ref.first_bad(s.tris, ref.rest_of(s.tris), groups, [ref.op(g, ref.affine(shift=(0.5, 0, 0)))], True) == ref.NONE
