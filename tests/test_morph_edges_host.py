"""The inputs of tests/test_gpu_morph_edges.py reach what they are meant to reach, shown on the models alone (tests/morph_ref.py,
tests/skin_ref.py, tests/transform_ref.py), without a device:

- every k of the magnitude ladder reaches its class under the morph's sum (q denormal, l2 = 0 with q != 0, l2 denormal, l2 just under
  the largest float, l2 = inf) on all three scenes, two records of neighbouring k reach every class but the first, and rest - rest
  is +0 in every component;
- every weight pattern has the effect it names: how many records are applied, the product that underflows, the -0 that comes out +0,
  the products that cancel, the row that is not touched; the padding words keep their bits;
- the offenders of the vertex cases and the accepted FLT_MAX are what the case says, the intermediate overflow is one (the exact sum
  is finite);
- the rows of 8 192 records are applied as their poses say;
- the triangle sets of the skin and group cases overlap as intended, and the live range of the motion case is strictly inside the
  list's;
- no model output that the device is compared with holds a NaN.

And the cases bite: three wrong variants of morph_ref.morphed - one that skips a record on w * d == 0 instead of w == 0, one that
renormalises untouched entries, one that adds a row's records in descending target order - differ from the model on these inputs."""
import numpy as np
import pytest

import morph_ref as ref
import test_gpu_morph_edges as cases
import transform_ref as tref
from ptmi import layout
from test_gpu_edit_edges import CLASS_OF, LADDER

CLASSES = set(tref.normal_classes(np.zeros((1, 3))))
TINY = np.finfo(np.float32).tiny


def wrong_morphed(tris, rest, listed, row_start, deltas, weights, wrong):
    """morph_ref.morphed with one thing wrong. product: a record is skipped where every one of its 18 products w * d is zero, not
    where w is; renormalise: the normals of untouched entries go through the tail too; descending: a row's records are added from
    its last to its first."""
    out = tris.copy()
    listed = np.asarray(listed, np.int64)
    row_start = np.asarray(row_start, np.int64)
    deltas = np.asarray(deltas, layout.MORPH_DELTA).reshape(-1)
    w_all = np.asarray(weights, np.float32)
    lengths = row_start[1:] - row_start[:-1]
    acc = {f: rest[f][listed].astype(np.float32).copy() for f in ref.VERTS + ref.NORMALS}
    touched = np.zeros(len(listed), bool)
    with np.errstate(all="ignore"):
        for j in range(int(lengths.max())):
            rows = np.flatnonzero(lengths > j)
            rec = row_start[rows + 1] - 1 - j if wrong == "descending" else row_start[rows] + j
            w = w_all[deltas["target"][rec].astype(np.int64)]
            if wrong == "product":
                use = np.zeros(len(rec), bool)
                for g in ref.DV + ref.DN:
                    use |= (w[:, None] * deltas[g][rec] != 0).any(axis=1)
            else:
                use = w != 0
            rows, rec, w = rows[use], rec[use], w[use]
            touched[rows] = True
            for f, g in zip(ref.VERTS + ref.NORMALS, ref.DV + ref.DN):
                acc[f][rows] = acc[f][rows] + w[:, None] * deltas[g][rec]
    if wrong == "renormalise":
        touched[:] = True
    for f in ref.VERTS:
        out[f][listed] = acc[f]
    for f in ref.NORMALS:
        n = acc[f]
        n[touched] = ref.unit_tail(n[touched])
        out[f][listed] = n
    return out


def test_the_wrong_variants_are_the_model_where_nothing_is_at_an_edge():
    """on an ordinary table with every weight non-zero and every row applied, two of the three variants are the model itself: what
    they get wrong is only what the edge cases reach"""
    s = cases.scene("cornell")
    listed = cases.listing_of(s, "third")
    rng = np.random.default_rng(151)
    row_start, deltas = ref.table(rng, len(listed), 4, (1, 2, 3))
    w = ref.weights_for(rng, 4, None)
    rest = tref.rest_of(s.tris)
    want = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    for wrong in ("product", "renormalise"):
        assert wrong_morphed(s.tris, rest, listed, row_start, deltas, w, wrong).tobytes() == want.tobytes(), wrong
    assert wrong_morphed(s.tris, rest, listed, row_start, deltas, w, None).tobytes() == want.tobytes()


def _normal_sums(s, listed, row_start, deltas, w):
    acc, touched = ref.summed(tref.rest_of(s.tris), listed, row_start, deltas, w)
    assert touched.all()
    return acc


@pytest.mark.parametrize("variant", ["one record", "two records"])
@pytest.mark.parametrize("name", cases.MAGNITUDE_SCENES)
def test_every_k_reaches_its_class_under_the_morphs_sum(name, variant):
    s, listed, row_start, deltas, w, idx = cases.magnitude_case(cases.scene(name), variant)
    assert np.count_nonzero(w) == 2 and (np.diff(row_start.astype(np.int64)) == (2 if variant == "two records" else 1)).all()
    assert all((s.tris[f][listed] == 0).all() for f in ref.NORMALS)
    acc = _normal_sums(s, listed, row_start, deltas, w)
    seen = set()
    for j, k in enumerate(LADDER[:len(LADDER) - (variant == "two records")]):
        q = np.concatenate([acc[f][idx == j] for f in ref.NORMALS])
        got = tref.normal_classes(q)
        seen |= {c for c, m in got.items() if m.any()}
        if variant == "one record":
            want = CLASS_OF[k]
            assert all(got[c].any() for c in ((want,) if isinstance(want, str) else want)), (name, k, {c: int(m.sum()) for c, m in got.items()})
    # two records of neighbouring k have the magnitude of the larger: no denormal q, and the classes of l2 all the same
    assert seen | ({"q_denormal"} if variant == "two records" else set()) == CLASSES, (name, variant, seen)
    out = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
    assert all(np.isfinite(out[f]).all() for f in tref.REST_FIELDS)
    assert all(np.abs(out[f]).max() < 100.0 for f in ref.VERTS)                          # the vertices stay ordinary
    zeros = np.concatenate([out[f][listed][idx == len(LADDER) - 1 - (variant == "two records")] for f in ref.NORMALS])
    assert (zeros == 0).all() and np.signbit(zeros).any() and not np.signbit(zeros).all()     # l2 = inf: signed zeros


@pytest.mark.parametrize("name", cases.MAGNITUDE_SCENES)
def test_rest_minus_rest_is_positive_zero(name):
    s, listed, row_start, deltas, w, _ = cases.magnitude_case(cases.scene(name), "cancelled")
    rest = tref.rest_of(s.tris)
    for f, g in zip(ref.NORMALS, ref.DN):
        r = rest[f][listed]
        assert (r != 0).any(axis=1).mean() > 0.9 and np.array_equal(r.astype(np.float64) * 8, np.round(r.astype(np.float64) * 8))
        assert deltas[g].tobytes() == (-r).tobytes()
    acc = _normal_sums(s, listed, row_start, deltas, w)
    out = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    for f in ref.NORMALS:
        assert (acc[f] == 0).all() and not np.signbit(acc[f]).any()
        assert out[f][listed].tobytes() == np.zeros((len(listed), 3), np.float32).tobytes()
    assert cases.no_nan(out)


def test_the_weight_patterns_reach_what_they_name():
    s, listed, row_start, deltas, w = cases.morph_weights_case()
    rest = tref.rest_of(s.tris)
    out = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    assert cases.no_nan(out) and all(np.isfinite(out[f]).all() for f in tref.REST_FIELDS)
    for own in (True, False):
        assert ref.first_bad(s.tris, rest, listed, row_start, deltas, w, own) == ref.NONE
    assert w[4] == np.float32(1e-45) > 0 and w[5] == np.float32(1e-41) and 0 < w[5] < TINY      # denormals, not zeros
    assert np.signbit(w[[10, 13]]).all() and (w[[10, 11, 13]] == 0).all() and not np.signbit(w[11])
    applied = ref.applied_counts(row_start, deltas, w)
    entries = {what: np.arange(len(listed))[i::cases.PERIOD] for i, what in enumerate(cases.PATTERNS)}
    for (what, e), k in zip(entries.items(), cases.APPLIED):
        assert len(e) > 8 and (applied[e] == k).all(), what
    rows = {what: [cases.row_of(row_start, deltas, x) for x in e] for what, e in entries.items()}
    fields = ref.DV + ref.DN

    def products(row):
        with np.errstate(all="ignore"):
            return np.concatenate([(w[row["target"].astype(np.int64)][:, None] * row[g]).reshape(-1) for g in fields])

    # the rest pose every pattern starts from
    assert np.signbit(rest["v1"][listed, 2]).all() and (rest["v1"][listed, 2] == 0).all()
    assert rest["n0"][listed].tobytes() == np.tile(np.array([-0.0, 2.0, 0.0], np.float32), (len(listed), 1)).tobytes()

    def turned_positive(e):
        z = out["v1"][listed[e], 2]
        x = out["n0"][listed[e], 0]
        return (z == 0).all() and not np.signbit(z).any() and (x == 0).all() and not np.signbit(x).any()

    # a denormal weight on an ordinary record: every product is zero, none negative, and still the entry is applied
    for what in ("1e-45 on an ordinary record", "one denormal weight beside it"):
        for row in rows[what]:
            p = products(row)
            assert (p == 0).all() and not np.signbit(p).any() and (np.concatenate([row[g].reshape(-1) for g in fields]) > 0).all(), what
        e = entries[what]
        assert turned_positive(e), what
        assert out["n0"][listed[e]].tobytes() == np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(e), 1)).tobytes(), what   # renormalised
        for f in ("v0", "v2"):                                           # x + 0 = x: the other vertices keep their value
            assert out[f][listed[e]].tobytes() == (rest[f][listed[e]] + np.float32(0.0)).tobytes(), what
    assert any((products(row) != 0).any() and (np.abs(products(row)) < TINY).all() for row in rows["1e-41 on an ordinary record"])
    for what in ("1e-45 on a record of 1e30", "1e-41 on a record of 1e30"):
        assert all((np.abs(products(row)) > TINY).sum() > 12 for row in rows[what]), what           # the product is ordinary
        assert out[listed[entries[what]]].tobytes() != s.tris[listed[entries[what]]].tobytes(), what
    for row in rows["w and -w on identical records"]:
        assert len(row) == 2 and all(row[g][0].tobytes() == row[g][1].tobytes() for g in fields)
        p = products(row).reshape(len(fields), 2, 3)
        assert (p[:, 0] == -p[:, 1]).all() and (p[:, 0] != 0).all()
    e = entries["w and -w on identical records"]
    n0 = out["n0"][listed[e]].astype(np.float64)
    assert np.allclose((n0 * n0).sum(axis=1), 1.0, atol=1e-6)            # the products cancel, and the normal is a unit vector all the same
    for f in ref.VERTS:
        assert np.allclose(out[f][listed[e]], rest[f][listed[e]], atol=1e-6)
    for what in ("1e30 on a record of 1e-30", "1e-30 on a record of 1e30"):
        for row in rows[what]:
            p = np.abs(products(row))
            assert (p < 1.0).all() and (p > 1e-6).sum() > 12, what
    for row in rows["only the last weight is not zero"]:
        assert (w[row["target"].astype(np.int64)] != 0).tolist() == [False, False, True]
    e = entries["every weight is -0"]
    for row in rows["every weight is -0"]:
        assert np.signbit(w[row["target"].astype(np.int64)]).all() and len(row) == 2
    assert out[listed[e]].tobytes() == s.tris[listed[e]].tobytes()       # untouched: the negative zeros and the normal of length 2 stay
    assert np.array_equal(entries["one denormal weight beside it"], e + 1)
    # the padding words keep their bits
    for i, f in enumerate(cases.PAD_FIELDS):
        bits = out[f][listed].view(np.uint32)
        assert np.array_equal(bits, cases.PAD_BITS[(np.arange(len(listed)) + i) % 4]) and out[f].tobytes() == s.tris[f].tobytes()
    assert {int(b) for f in cases.PAD_FIELDS for b in out[f][listed].view(np.uint32)} == {int(b) for b in cases.PAD_BITS}


def test_the_weight_case_tells_the_wrong_skips_apart():
    s, listed, row_start, deltas, w = cases.morph_weights_case()
    rest = tref.rest_of(s.tris)
    want = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    assert wrong_morphed(s.tris, rest, listed, row_start, deltas, w, None).tobytes() == want.tobytes()
    by_pattern = {}
    for wrong in ("product", "renormalise"):
        got = wrong_morphed(s.tris, rest, listed, row_start, deltas, w, wrong)
        assert got.tobytes() != want.tobytes(), wrong
        by_pattern[wrong] = [what for i, what in enumerate(cases.PATTERNS)
                             if got[listed[i::cases.PERIOD]].tobytes() != want[listed[i::cases.PERIOD]].tobytes()]
    assert by_pattern["product"] == ["1e-45 on an ordinary record", "one denormal weight beside it"]
    assert by_pattern["renormalise"] == ["every weight is -0"]


def test_the_vertex_cases_offend_where_they_say():
    s, set_on, listed, row_start, deltas, good, poses = cases.vertex_edge_case()
    rest = tref.rest_of(set_on)
    assert all(np.isfinite(deltas[g]).all() for g in ref.DV + ref.DN) and all(np.isfinite(w).all() for w, _ in poses.values())
    assert all(np.isfinite(set_on[f]).all() for f in ref.VERTS)          # update_triangles and the host's argument checks pass
    live = ref.morphed(set_on, rest, listed, row_start, deltas, good)
    assert len(ref.offenders(set_on, rest, listed, row_start, deltas, good, own=False)) == 0 and cases.no_nan(live)
    e1, e2, e3 = (cases.EDGE_ENTRIES[k] for k in ("FLT_MAX", "intermediate", "nan"))
    assert len({e // 32 for e in (e1, e2, e3)}) == 3                      # three blocks of the launch
    want = {"FLT_MAX exactly": [], "FLT_MAX + 2e31": [e1], "3e38 + 3e38 - 3e38 in row order": [e2], "inf - inf": [e3], "all three": [e1, e2, e3]}
    for name, (w, first) in poses.items():
        got = ref.offenders(live, rest, listed, row_start, deltas, w, own=False).tolist()
        assert got == want[name] and first == (got[0] if got else None), name
    out = ref.morphed(live, rest, listed, row_start, deltas, poses["FLT_MAX exactly"][0])
    assert out["v2"][listed[e1], 1] == tref.F32_MAX and cases.no_nan(out) and all(np.isfinite(out[f]).all() for f in ref.VERTS)
    with np.errstate(all="ignore"):
        assert np.isinf(tref.F32_MAX + np.float32(2e31)) and np.isfinite(tref.F32_MAX + np.float32(1e31))
    out = ref.morphed(live, rest, listed, row_start, deltas, poses["3e38 + 3e38 - 3e38 in row order"][0])
    row = cases.row_of(row_start, deltas, e2)
    exact = float(rest["v0"][listed[e2], 0]) + float(row["dv0"][0, 0]) + float(row["dv0"][1, 0])
    assert np.isposinf(out["v0"][listed[e2], 0]) and exact == float(np.float32(3e38))    # the exact sum is finite: the order decides
    out = ref.morphed(live, rest, listed, row_start, deltas, poses["inf - inf"][0])
    assert np.isnan(out["v1"][listed[e3], 2])
    # a sum in descending target order gives 3e38 - 3e38 + 3e38: that entry no longer offends
    for name, (w, _) in poses.items():
        t = wrong_morphed(live, rest, listed, row_start, deltas, w, "descending")[listed]
        bad = np.flatnonzero(~(np.isfinite(t["v0"]).all(axis=1) & np.isfinite(t["v1"]).all(axis=1) & np.isfinite(t["v2"]).all(axis=1))).tolist()
        assert bad == [e for e in want[name] if e != e2], name


def test_a_finite_pose_can_write_a_normal_that_is_not_finite():
    """what DESIGN.md §19 puts out of scope: the check pass looks at the vertices, as ptmi_update_triangles does, and no device case
    goes here (a NaN's bits differ between numpy and the device)"""
    s = cases.scene("cornell")
    listed, row_start = np.array([3], np.uint32), np.array([0, 1], np.uint32)
    deltas, w = cases.record(0, dn0=(3e38, 0, 0)), np.array([2.0], np.float32)
    rest = tref.rest_of(s.tris)
    assert np.isfinite(deltas["dn0"]).all() and np.isfinite(w).all()
    for own in (True, False):
        assert ref.first_bad(s.tris, rest, listed, row_start, deltas, w, own) == ref.NONE
    out = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    assert np.isnan(out["n0"][3, 0]) and out["v0"][3].tobytes() == s.tris["v0"][3].tobytes()      # inf / sqrt(inf)


def test_the_long_rows_are_applied_as_their_poses_say():
    for kind in ("wave", "neighbours"):
        s, listed, row_start, deltas = cases.row_shape_case(kind)
        lengths = np.diff(row_start.astype(np.int64))
        assert lengths[:8].tolist() == [0, 0, 0, 0, cases.LONG, 1 if kind == "neighbours" else 0, 0, 0]
        assert sorted(set(lengths[8:].tolist())) == [0, 1, 2, 3] and lengths.max() == ref.MAX_TARGETS == 8192
        long = cases.row_of(row_start, deltas, cases.LONG_ENTRY)
        assert np.array_equal(long["target"], np.arange(cases.LONG))
        rest = tref.rest_of(s.tris)
        for name, w in cases.row_shape_poses(kind).items():
            applied = ref.applied_counts(row_start, deltas, w)
            hit = np.flatnonzero(w[long["target"].astype(np.int64)] != 0)
            want = {"only target 8191": [cases.LONG - 1], "only target 0": [0], "all 8192": list(range(cases.LONG))}[name]
            assert hit.tolist() == want and applied[cases.LONG_ENTRY] == len(want), (kind, name)
            assert applied[[0, 1, 2, 3, 6, 7]].sum() == 0
            if kind == "neighbours":
                assert applied[cases.LONG_ENTRY + 1] == 1
            if name == "all 8192":
                assert (applied == lengths).all()
        w = cases.row_shape_poses(kind)["only target 8191"]
        out = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
        moved = np.flatnonzero([out[t].tobytes() != s.tris[t].tobytes() for t in listed[:8]])
        assert moved.tolist() == ([4, 5] if kind == "neighbours" else [4]) and cases.no_nan(out)
    s, listed, row_start, deltas = cases.row_shape_case("one")
    assert len(listed) == 1 and row_start.tolist() == [0, 8192] and len(np.unique(deltas["target"])) == 8192
    for name, w in cases.row_shape_poses("one").items():
        out = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
        assert cases.no_nan(out) and out[listed].tobytes() != s.tris[listed].tobytes()
        assert all(np.abs(out[f]).max() < 10.0 for f in ref.VERTS) and ref.first_bad(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w, True) == ref.NONE


def test_the_sets_overlap_as_intended():
    # 5: one offender among the entries that go to the skin's rest rows, a later one among those that go to live records
    s, m_list, row_start, deltas, s_list, corners, (e_in, e_out) = cases.skin_refusal_case()
    assert m_list[e_in] in s_list and m_list[e_out] not in s_list and e_in < e_out and e_in // 8 != e_out // 8
    assert cases.row_of(row_start, deltas, e_in)["target"][-1] == 5 and cases.row_of(row_start, deltas, e_out)["target"][-1] == 6
    assert (deltas["target"] == 5).sum() == 1 and (deltas["target"] == 6).sum() == 1
    rest = tref.rest_of(s.tris)
    assert len(ref.offenders(s.tris, rest, m_list, row_start, deltas, cases.refusal_weights(122), own=True)) == 0
    for i, (where, raised) in enumerate(cases.PLACEMENTS.items()):
        bad = cases.refusal_weights(123 + i, raised)
        assert (bad[:5] != cases.refusal_weights(122)[:5]).all()
        got = ref.offenders(s.tris, rest, m_list, row_start, deltas, bad, own=True).tolist()
        assert got == [e for e, t in ((e_in, 5), (e_out, 6)) if t in raised], where
    # 6, 7: a moved group with members in the morph alone, in the skin alone, in both and in neither
    s, groups, g, m_list, row_start, deltas, s_list, corners = cases.three_way_case()
    assert all(len(part) > 8 for part in cases.overlaps(groups, g, m_list, s_list))
    shared = np.intersect1d(m_list, s_list)
    inside = (shared >= 37) & (shared < 251)
    assert inside.sum() > 8 and (~inside).sum() > 8
    applied = ref.applied_counts(row_start, deltas, np.ones(4, np.float32))
    assert (applied[np.isin(m_list, shared)] > 0).sum() > 8              # shared triangles whose rows hold records
    ranges = cases.rebase_ranges(m_list, len(s.tris))
    lo, hi = ranges["a gap of the list"]
    assert not np.isin(np.arange(lo, hi), m_list).any() and lo - 1 in m_list and hi in m_list
    # 8: the lowest and the highest morphed triangle go to the skin's rest rows
    s, m_list, row_start, deltas, s_list, corners = cases.mixed_motion_case()
    lo, hi = cases.live_range(m_list, s_list)
    assert m_list.min() in s_list and m_list.max() in s_list and lo in m_list and hi in m_list
    assert m_list.min() < lo < hi < m_list.max()
    assert (np.diff(s_list.astype(np.int64)) > 0).all() and 8 < np.isin(m_list, s_list).sum() < len(m_list) // 2
    assert (~np.isin(s_list, m_list)).sum() > 8
    assert (ref.applied_counts(row_start, deltas, np.ones(3, np.float32))[np.isin(m_list, [lo, hi])] > 0).all()
