"""The inputs of tests/test_gpu_edit_edges.py reach what they are meant to reach, shown on the models alone (tests/transform_ref.py,
tests/skin_ref.py), without a device:

- the scene of the round cases is longer than a round of 256 CUs by a count that is no multiple of 8, and every launch of the
  transform cases makes a second round;
- every offender set of the refusal cases is, by the model, exactly the intended set of entries, each walked in the round, block and
  wave its name says, for the joint counts and the op counts the device is asked with;
- every k of the magnitude ladder reaches its class (q denormal, l2 = 0 with q != 0, l2 denormal, l2 just under the largest float,
  l2 = inf) on the normals the op or joint of that k actually transforms, on cornell and grid80; on soup80, whose normals are not
  unit and partly zero, every class occurs somewhere across the ladder;
- no model output of the magnitude and weight cases holds a NaN (a byte comparison would depend on its payload).

The device's CU count is not known here: the cases are built for 256, the MI355X's, and the device tests assert their own count."""
import numpy as np
import pytest

import skin_ref as ref
import test_gpu_edit_edges as cases
import transform_ref as tref

CUS = cases.MI355X_CUS
R = cases.round_of(CUS)


def test_the_round_scene_is_longer_than_a_round_by_a_partial_wave():
    s = cases.big_scene(CUS)
    n = len(s.tris)
    assert s.name == "grid_200" and n == 79212
    assert n > R and (n - R) % 8 != 0 and (n - R) % 32 != 0
    assert cases.where(n - 1, CUS)[0] == 1                             # the last entry is walked in round two
    for kind in ("one op", "600 ops"):
        groups, ops = cases.round_transform(s, kind, CUS)
        for first, end in tref.launch_ranges(groups, ops):
            assert first % 8 == 0 and end - first > R


def test_launch_ranges_are_the_chunks_of_the_call():
    groups = np.array([9, 9, 9, 3, 3, 9, 9, 9, 9, 9, 9, 1, 9, 2, 9, 9, 9, 9, 9, 9, 9, 9, 4, 9], np.uint32)
    ops = [tref.op(g, tref.affine()) for g in (3, 2, 7, 8, 4)]
    assert tref.launch_ranges(groups, ops, chunk=2) == [(0, 14), None, (16, 23)]
    assert tref.launch_ranges(groups, ops, chunk=5) == [(0, 23)]
    assert tref.launch_ranges(groups, [], chunk=2) == []


@pytest.mark.parametrize("n_joints", [512, 600])
def test_skin_offenders_are_the_intended_entries(n_joints):
    s = cases.big_scene(CUS)
    k, end = cases.refusal_window(s.tris, CUS)
    count = end - k
    assert k % 8 == 0 and count > R and (count - R) % 8 != 0
    rest = tref.rest_of(s.tris)
    good, bad = cases.bad_pose(n_joints, 66)
    assert all(np.isfinite(m).all() and np.isfinite(nm).all() for m, nm in bad)          # the host's argument check passes
    for which, entries in cases.offender_sets(R, count).items():
        cases.check_places(entries, which, CUS, count)
        listed, corners = cases.skin_refusal(s.tris, CUS, n_joints, entries)
        users = np.flatnonzero((corners["joint"].reshape(-1, 12) == n_joints - 1).any(axis=1))
        assert np.array_equal(users, np.sort(entries)), which                            # the bad joint is referenced by those entries only
        live = ref.skinned(s.tris, rest, listed, corners, good)
        assert len(ref.offenders(s.tris, rest, listed, corners, good, own=True)) == 0
        for own in (True, False):
            assert np.array_equal(ref.offenders(live, rest, listed, corners, bad, own), np.sort(entries)), which
        assert ref.first_bad(live, rest, listed, corners, bad, True) == k + min(entries)


def test_group_offenders_are_the_intended_entries():
    s = cases.big_scene(CUS)
    k, end = cases.refusal_window(s.tris, CUS)
    rest = tref.rest_of(s.tris)
    warm = [tref.op(1, cases.T1)]
    made = []
    for which, entries in cases.offender_sets(R, end - k).items():
        made.append((which, entries) + cases.group_refusal(s.tris, CUS, entries))
        assert tref.launch_ranges(*made[-1][2:]) == [(k, end)]
    for which, (first_entries, third_entries) in cases.chunk_sets(R).items():
        made.append((which, first_entries + third_entries) + cases.chunked_refusal(s.tris, CUS, first_entries, third_entries))
        ranges = tref.launch_ranges(*made[-1][2:])
        assert len(ranges) == 3 and ranges[0][0] == k and ranges[0][1] - k > R and ranges[2][1] - ranges[2][0] <= 8
    for which, entries, groups, ops in made:
        assert all(np.isfinite(m).all() and np.isfinite(nm).all() for _, m, nm in ops)
        bad_groups = [g for g, m, _ in ops if m.tobytes() == cases.BAD_M.tobytes()]
        assert np.array_equal(np.flatnonzero(np.isin(groups, bad_groups)), k + np.sort(entries)), which   # the bad groups have those members only
        live = tref.transformed(s.tris, rest, groups, warm)
        for own in (True, False):
            assert np.array_equal(tref.offenders(live, rest, groups, ops, own), k + np.sort(entries)), which
        good = [o for o in ops if o[0] not in bad_groups]
        assert len(tref.offenders(live, rest, groups, good, True)) == 0


def _reached(q, k):
    """every class CLASS_OF names for k occurs among the rows of q"""
    got = tref.normal_classes(q)
    want = cases.CLASS_OF[k]
    return all(got[c].any() for c in ((want,) if isinstance(want, str) else want)), {c: int(m.sum()) for c, m in got.items()}


@pytest.mark.parametrize("name", cases.MAGNITUDE_SCENES)
def test_every_k_reaches_its_class_under_transform_groups(name):
    s = cases.scene(name)
    groups, ops = cases.ladder_groups(s), cases.ladder_ops()
    seen = set()
    for (g, m, nm), k in zip(ops, cases.LADDER):
        assert nm.tobytes() == (np.float32(k) * np.eye(3, dtype=np.float32)).tobytes()
        n = np.concatenate([s.tris[f][groups == g] for f in cases.NORMALS])
        q = ref.q_rows(np.tile(nm, (len(n), 1)), n)
        ok, counts = _reached(q, k)
        seen |= {c for c, v in counts.items() if v}
        assert ok or name == "soup80", (name, k, counts)
    assert seen == set(tref.normal_classes(np.zeros((1, 3)))), (name, seen)
    out = tref.transformed(s.tris, tref.rest_of(s.tris), groups, ops)
    assert not any(np.isnan(out[f]).any() for f in tref.REST_FIELDS)
    assert all(np.isfinite(out[f]).all() for f in cases.VERTS)


@pytest.mark.parametrize("blended", [False, True])
@pytest.mark.parametrize("name", cases.MAGNITUDE_SCENES)
def test_every_k_reaches_its_class_under_pose_skin(name, blended):
    s = cases.scene(name)
    listed, corners = cases.ladder_skin(s, blended)
    joints = cases.ladder_records(60)
    M, NM = ref.joint_arrays(joints)
    c3 = corners.reshape(-1, 3)
    seen = set()
    for j, k in enumerate(cases.LADDER):
        q = []
        for c, f in enumerate(cases.NORMALS):
            sel = c3["joint"][:, c, 0] == j
            q.append(ref.q_rows(ref.blend(NM, c3[sel, c]), s.tris[f][listed][sel]))
        ok, counts = _reached(np.concatenate(q), k)
        seen |= {c for c, v in counts.items() if v}
        assert ok or blended or name == "soup80", (name, k, counts)
    # a blend of two k has the magnitude of the larger: no denormal q, and the classes of l2 all the same
    assert seen | ({"q_denormal"} if blended else set()) == set(tref.normal_classes(np.zeros((1, 3)))), (name, blended, seen)
    if blended:
        assert (np.count_nonzero(corners["weight"], axis=1) == 2).all() and (corners["joint"][:, 1] == corners["joint"][:, 0] + 1).all()
    out = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    assert not any(np.isnan(out[f]).any() for f in tref.REST_FIELDS)
    assert all(np.isfinite(out[f]).all() for f in cases.VERTS)


def test_the_weight_patterns_reach_what_they_name():
    s, listed, corners, joints = cases.weights_case()
    mirror = joints[cases.MIRROR_JOINT][1]
    assert np.signbit(mirror[mirror == 0]).any()                       # the record keeps the negative zeros of a mirror's cofactors
    assert not any(np.signbit(nm[nm == 0]).any() for i, (_, nm) in enumerate(joints) if i != cases.MIRROR_JOINT)
    c3 = corners.reshape(-1, 3)
    w, j = c3["weight"].reshape(-1, 4), c3["joint"].reshape(-1, 4)
    sums = w.astype(np.float64).sum(axis=1)
    assert (w < 0).any() and np.isclose(sums, 0.25).any() and np.isclose(sums, 3.0).any()
    assert (w == 0).all(axis=1).any() and ((w == 0).all(axis=1).reshape(-1, 3).all(axis=1)).any()    # a corner, and a whole triangle
    assert ((j == j[:, :1]).all(axis=1) & (w == 0.25).all(axis=1)).any()
    assert ((w == 0) & (j == cases.MIRROR_JOINT)).any()
    rest = tref.rest_of(s.tris)
    out = ref.skinned(s.tris, rest, listed, corners, joints)
    assert not any(np.isnan(out[f]).any() for f in tref.REST_FIELDS)
    # the collapsed corners are the model's signed zeros, some of them negative: 0 * entry keeps the entry's sign
    dead = np.flatnonzero((c3["weight"] == 0).all(axis=2).all(axis=1))
    v = np.concatenate([out[f][listed[dead]] for f in cases.VERTS + cases.NORMALS])
    assert (v == 0).all() and np.signbit(v).any() and not np.signbit(v).all()
    for own in (True, False):                                          # finite everywhere: the device accepts the pose
        assert ref.first_bad(s.tris, rest, listed, corners, joints, own) == ref.NONE


def test_the_overlap_and_the_rebase_ranges():
    s, groups, listed, corners, g = cases.overlap_case()
    members = np.flatnonzero(groups == g)
    share = np.isin(members, listed).mean()
    assert 0.3 < share < 0.7                                           # about half of the moved group is skinned too
    ranges = cases.rebase_ranges(listed, len(s.tris))
    lo, hi = ranges["a gap of the list"]
    assert not np.isin(np.arange(lo, hi), listed).any() and lo - 1 in listed and hi in listed
    assert ranges["the first listed"][0] == listed.min() and ranges["the last listed"][0] == listed.max()
    n = len(cases.scene("grid80").tris)
    al = cases.aligned_groups(n)
    assert np.flatnonzero(al == 1)[[0, -1]].tolist() == [cases.ALIGN_LO, cases.ALIGN_HI] and np.flatnonzero(al == 2).tolist() == [n - 1]
