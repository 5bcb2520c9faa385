"""Morph targets without a device (include/ptmi.h ptmi_set_morph, ptmi_pose_morph): the struct sizes, the calls' NULL-context answers
and the model of tests/morph_ref.py: what an all-zero pose leaves, one record of weight one, and its positions against float64.

The bound of the float64 comparison, from the operation count. A component is p_k after k applied records,
    p_0 = rest,   p_i = fl(p_(i-1) + fl(w_i * d_i)).
Every float32 operation rounds its exact result by a factor (1 + e), |e| <= u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, (2.4); the operands here are far from the denormals). The rest component passes the k sums, term i its product and the
sums i..k: no term passes more than k + 1 roundings, so
    |computed - exact| <= ((1 + u)^(k+1) - 1) * A <= (k + 1) * 2 u * A = (k + 1) * 2^-23 * A,   A = |rest| + sum |w_i * d_i|
where the doubling covers the second-order terms of (1 + u)^(k+1) - 1 (for k + 1 <= 2^22) and the float64 evaluation's own error,
(k + 1) * 2^-53 * A."""
import ctypes
import os
import subprocess

import numpy as np

import morph_ref as ref
import transform_ref as tref
from ptmi import layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes(tmp_path):
    from ptmi import native
    assert ctypes.sizeof(native.MorphStatus) == 48 and layout.MORPH_DELTA.itemsize == 96
    names = ("present", "n_targets", "n_morphed", "n_records", "n_in_skin", "poses", "active_targets", "first_bad", "skin_stale",
             "reserved", "pose_ms")
    fields = ("dv0", "target", "dv1", "reserved0", "dv2", "reserved1", "dn0", "reserved2", "dn1", "reserved3", "dn2", "reserved4")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(ptmi_morph_delta), sizeof(struct ptmi_morph_status));\n'
                   + "".join(f'printf("%zu\\n", offsetof(struct ptmi_morph_status, {n}));\n' for n in names)
                   + "".join(f'printf("%zu\\n", offsetof(ptmi_morph_delta, {n}));\n' for n in fields) + "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:2] == [96, 48]
    assert got[2:2 + len(names)] == [getattr(native.MorphStatus, n).offset for n in names]
    assert got[2 + len(names):] == [layout.MORPH_DELTA.fields[n][1] for n in fields]
    assert [f for f, _ in native.MorphStatus._fields_] == list(names)


def test_calls_without_a_context_are_refused():
    """a NULL handle is PTMI_E_INVALID for every new entry point"""
    from ptmi import native
    L = native.load()
    t, rows = np.zeros(1, np.uint32), np.array([0, 1], np.uint32)
    d = np.zeros(1, layout.MORPH_DELTA)
    w = np.ones(1, np.float32)
    st = native.MorphStatus()
    p = native._p
    assert L.ptmi_set_morph(None, p(t), p(rows), p(d), 1, 1) == -1
    assert L.ptmi_pose_morph(None, p(w), 1) == -1
    assert L.ptmi_morph_status(None, ctypes.byref(st)) == -1
    assert L.ptmi_multi_set_morph(None, p(t), p(rows), p(d), 1, 1) == -1
    assert L.ptmi_multi_pose_morph(None, p(w), 1) == -1
    assert L.ptmi_multi_morph_status(None, ctypes.byref(st)) == -1


def _case(seed=51, fraction=0.4, n_targets=6, lengths=(0, 1, 2, 3)):
    from ptmi import scenes
    s = scenes.make("cornell")
    rng = np.random.default_rng(seed)
    n = len(s.tris)
    listed = np.sort(rng.choice(n, max(1, int(n * fraction)), replace=False)).astype(np.uint32)
    row_start, deltas = ref.table(rng, len(listed), n_targets, lengths)
    return s, listed, row_start, deltas, rng


def test_an_all_zero_pose_is_the_rest_bytes():
    """with weights of either sign of zero, and with negative zeros in the rest pose (which -0 + 0 * d would turn into +0)"""
    s, listed, row_start, deltas, _ = _case()
    tris = s.tris.copy()
    for f in ref.VERTS + ref.NORMALS:
        tris[f][listed[::2], 1] = -0.0
    tris["n0"][listed[1]] = (0.0, 3.0, 0.0)                              # not unit: an untouched triangle is not renormalised
    rest = tref.rest_of(tris)
    for w in (np.zeros(6, np.float32), np.full(6, -0.0, np.float32), np.array([0, -0.0, 0, -0.0, -0.0, 0], np.float32)):
        assert ref.morphed(tris, rest, listed, row_start, deltas, w).tobytes() == tris.tobytes()
    assert np.signbit(tris["v0"][listed[0], 1])
    with np.errstate(all="ignore"):
        assert not np.signbit(np.float32(-0.0) + np.float32(0.0) * np.float32(0.5))      # what the skip avoids


def test_one_record_of_weight_one_adds_its_delta_exactly():
    s, listed, row_start, deltas, _ = _case(lengths=(1,))
    rest = tref.rest_of(s.tris)
    for target in range(6):
        w = np.zeros(6, np.float32)
        w[target] = 1.0
        out = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
        hit = deltas["target"] == target                                 # (rows of one record: record e is entry e's)
        assert hit.any()
        for f, g in zip(ref.VERTS, ref.DV):
            assert out[f][listed[hit]].tobytes() == (s.tris[f][listed[hit]] + deltas[g][hit]).tobytes()
            assert out[f][listed[~hit]].tobytes() == s.tris[f][listed[~hit]].tobytes()
        for f, g in zip(ref.NORMALS, ref.DN):
            assert out[f][listed[hit]].tobytes() == ref.unit_tail(s.tris[f][listed[hit]] + deltas[g][hit]).tobytes()
            assert out[f][listed[~hit]].tobytes() == s.tris[f][listed[~hit]].tobytes()
        other = np.ones(len(s.tris), bool)
        other[listed] = False
        assert out[other].tobytes() == s.tris[other].tobytes()
        for f in s.tris.dtype.names:
            if f not in tref.REST_FIELDS:
                assert out[f].tobytes() == s.tris[f].tobytes(), f        # uvs, material_index, padding


def test_model_positions_against_float64():
    from ptmi import scenes
    s = scenes.random_soup(80)
    rng = np.random.default_rng(52)
    n, n_targets = len(s.tris), 12
    listed = np.arange(n, dtype=np.uint32)
    tris = s.tris.copy()
    for f in ref.VERTS:
        tris[f] = (tris[f] * 10.0 ** rng.integers(-2, 3, size=(n, 1))).astype(np.float32)
    rest = tref.rest_of(tris)
    for trial in range(12):
        row_start, deltas = ref.table(rng, n, n_targets, (0, 1, 3, 5, 8, 12), dv=10.0 ** rng.integers(-3, 3))
        w = ref.weights_for(rng, n_targets, (1, 4, 12)[trial % 3])
        if trial % 4 == 0:
            w = (w * 100.0).astype(np.float32)
        out = ref.morphed(tris, rest, listed, row_start, deltas, w)
        k = ref.applied_counts(row_start, deltas, w)
        assert k.max() > 3 or trial % 3 == 0
        rs = row_start.astype(np.int64)
        wd = w.astype(np.float64)[deltas["target"].astype(np.int64)]
        entry_of = np.repeat(np.arange(n), rs[1:] - rs[:-1])
        for f, g in zip(ref.VERTS, ref.DV):
            term = wd[:, None] * deltas[g].astype(np.float64)            # exact products of float32 values, zero where skipped
            exact, A = rest[f].astype(np.float64), np.abs(rest[f].astype(np.float64))
            np.add.at(exact, entry_of, term)
            np.add.at(A, entry_of, np.abs(term))
            bound = (k[:, None] + 1) * 2.0 ** -23 * A
            err = np.abs(out[f].astype(np.float64) - exact)
            assert np.all(err <= bound), (trial, f, (err / np.maximum(bound, 1e-300)).max())
            assert np.array_equal(out[f][k == 0], tris[f][k == 0])
