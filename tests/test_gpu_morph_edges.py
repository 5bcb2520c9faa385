"""ptmi_pose_morph (csrc/scene_morph.hip k_morph) where tests/test_gpu_morph.py, tests/test_gpu_morph_skin.py and
tests/test_gpu_morph_rounds.py do not reach: the second pass tests/test_gpu_edit_edges.py made for the groups and the skin.

The rule is theirs: context A uploads S and poses on the device; context B holds the same upload and gets the model's records through
update_triangles(0, ...) (tests/morph_ref.py, tests/skin_ref.py, tests/transform_ref.py: the header's arithmetic in float32 numpy, and
Composed below: the header's "Interactions" paragraphs said once). A's live records are the model's over all 128 bytes and
same_state(A, B) holds. No tolerance, no renders, no oracle.

1. Normals of every magnitude. The rest normals of the listed triangles are zero and every entry has one record dn = 2k u under
   weight 0.5 (u a seeded unit vector, k from LADDER by entry), so the sum is k u and falls to q denormal, l2 = 0 with q != 0, l2
   denormal, l2 just under the largest float and l2 = inf (signed zeros); then two records of neighbouring k under two weights; then
   rest normals that are exact in float32 with dn = -rest under weight 1: l2 = 0 with q = +0.
2. Weights as given, on a third of cornell: a denormal weight (1e-45, 1e-41) on an ordinary record (the product underflows, the entry
   still counts as applied and a -0 rest component comes out +0) and on a record of 1e30; w and -w on identical records; 1e30 on
   1e-30 and the reverse; a row whose only non-zero weight is its last; a row of -0 weights beside a row with one denormal weight;
   and rest padding words of arbitrary bits (a quiet NaN with a payload, all ones, 1, the sign bit alone), which keep them:
   upload_scene takes them as they are.
3. The edge of the vertex check, on reference leaves, where it is on the vertices alone: a sum of exactly FLT_MAX is accepted;
   FLT_MAX + 2e31, rest 3e38 + 3e38 - 3e38 in row order (inf where the exact sum is finite) and inf - inf (a NaN; the products
   2 * 3e38 and 2 * -3e38 overflow, which a sum of finite terms cannot give otherwise) are refused with the model's first_bad.
4. Row shapes: a row of 8 192 records beside seven empty ones in one wave, posed by its last target alone, by its first alone and
   by all; beside a row of one in the next octet; and a list of one entry owning every record.
5. Refusals while entries go to the skin's rest rows: the next pose_skin gives the bytes it gave before.
6. Morph and groups on one context, and all three features on one triangle.
7. Re-basing: the four ranges of morph_rebase, update_triangles over shared triangles with skin_stale 0 and 1, set_morph after a
   skin pose.
8. The dirty range of a pose whose extreme entries go to the skin's rest rows.

No model output that is compared holds a NaN (its bits would differ between numpy and the device): every case asserts it.

The functions down to "the device" build the cases and need no device; tests/test_morph_edges_host.py imports them and shows on the
model that every input reaches the case it names.

Every case fails without the feature: the binding has no set_morph."""
import numpy as np
import pytest

import morph_ref as ref
import scene_update_ref as uref
import skin_ref as sref
import transform_ref as tref
from ptmi import layout
from test_gpu_edit_edges import CLASS_OF, LADDER, MODES, T1, T2, equals_updated, overlap_case, rebase_ranges, snapshot, unchanged, upload
from test_gpu_morph import listing_of
from test_gpu_morph_skin import N_JOINTS, sets
from test_gpu_scene_update import ctx_a, ctx_b, scene  # noqa: F401 (fixtures)
from test_gpu_skin import pose
from test_gpu_skin import records as joint_records
from test_gpu_transform import fresh_scene
from test_gpu_transform import records as op_records

pytestmark = pytest.mark.gpu

E_INVALID = -1
NONE = 0xFFFFFFFF
VERTS, NORMALS = ref.VERTS, ref.NORMALS
FLT_MAX = tref.F32_MAX
OWN, REFERENCE = (2, 1, 0), (1, 1, 0)                # (leaves, tree_builder, keep_reference_tree)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def record(target, **fields):
    """one layout.MORPH_DELTA record on `target`: the fields named (dv0 .. dn2) as given, everything else zero"""
    r = np.zeros(1, layout.MORPH_DELTA)
    r["target"] = target
    for f, v in fields.items():
        r[f][0] = v
    return r


def random_record(rng, target, dv=0.03, dn=0.3, positive=False):
    """a seeded record of table()'s sizes; positive: no component is negative"""
    r = record(target)
    for fields, size in ((ref.DV, dv), (ref.DN, dn)):
        for f in fields:
            v = rng.uniform(-size, size, 3)
            r[f][0] = np.abs(v) if positive else v
    return r


def with_rows(row_start, deltas, rows):
    """the table (row_start, deltas) with the rows of the entries in `rows` (entry -> its records) replaced"""
    rs = np.asarray(row_start, np.int64)
    parts = [rows[e] if e in rows else deltas[rs[e]:rs[e + 1]] for e in range(len(rs) - 1)]
    out = np.concatenate(parts) if parts else deltas[:0]
    assert all((np.diff(p["target"].astype(np.int64)) > 0).all() for p in parts)         # every row ascends by target
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32), out


def row_of(row_start, deltas, e):
    return deltas[int(row_start[e]):int(row_start[e + 1])]


def no_nan(tris):
    return not any(np.isnan(tris[f]).any() for f in tref.REST_FIELDS)


class Composed:
    """The state of a context with a group table, a skin and a morph on it, as the "Interactions" paragraphs of include/ptmi.h give
    it: three rest poses (kept per triangle here; only the members' and the listed triangles' rows matter), each snapshotted from the
    live records when its feature is set and re-based by update_triangles inside its range; every pose is its feature's edit of its
    own rest pose, and the last writer's record stands. The morph's result for a triangle the skin lists too goes to the skin's rest
    row and leaves the live record alone."""

    def __init__(self, tris):
        self.live = tris.copy()
        self.groups = self.skin = self.morph = None

    def set_groups(self, groups):
        self.groups, self.g_rest = groups, tref.rest_of(self.live)

    def set_skin(self, listed, corners):
        self.skin, self.s_rest = (listed, corners), tref.rest_of(self.live)

    def set_morph(self, listed, row_start, deltas):
        self.morph, self.m_rest = (listed, row_start, deltas), tref.rest_of(self.live)

    def shared(self):
        return np.intersect1d(self.morph[0], self.skin[0]).astype(np.int64) if self.skin and self.morph else np.zeros(0, np.int64)

    def update(self, lo, edit):
        self.live = self.live.copy()
        self.live[lo:lo + len(edit)] = edit
        for on, rest in ((self.groups is not None, "g_rest"), (self.skin, "s_rest"), (self.morph, "m_rest")):
            if on:
                for f in tref.REST_FIELDS:
                    getattr(self, rest)[f][lo:lo + len(edit)] = edit[f]
        return self.live

    def pose_morph(self, w):
        out = ref.morphed(self.live, self.m_rest, *self.morph, w)
        both = self.shared()
        if len(both):
            for f in tref.REST_FIELDS:
                self.s_rest[f][both] = out[f][both]
            out[both] = self.live[both]
        self.live = out
        return out

    def pose_skin(self, joints):
        self.live = sref.skinned(self.live, self.s_rest, *self.skin, joints)
        return self.live

    def transform(self, ops):
        self.live = tref.transformed(self.live, self.g_rest, self.groups, ops)
        return self.live


# ---- 1: normals of every magnitude --------------------------------------------------------------------------------------------------------
MAGNITUDE_SCENES = ("cornell", "grid80", "soup80")
VARIANTS = ("one record", "two records", "cancelled")


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def magnitude_case(s, variant):
    """(the scene with the listed normals replaced, listed, row_start, deltas, weights, the index into LADDER of every entry's k):
    half the triangles, two targets. one record: rest normals 0, dn = 2k u on target entry % 2, weights (0.5, 0.5). two records:
    dn = 2k u on target 0 and 2k' u' on target 1, k' the next of the ladder, weights (0.75, -0.5). cancelled: rest normals of
    eighths (exact in float32), dn = -rest on target 0, weights (1, 0); the index is 0 throughout."""
    listed = listing_of(s, "half", seed=111)
    n = len(listed)
    rng = np.random.default_rng(112)
    tris = s.tris.copy()
    two = variant == "two records"
    idx = np.zeros(n, np.int64) if variant == "cancelled" else rng.integers(0, len(LADDER) - (1 if two else 0), n)
    k2 = np.float32(2.0) * np.array(LADDER, np.float32)
    d = np.zeros((n, 2 if two else 1), layout.MORPH_DELTA)
    d["target"][:, 0] = 0 if two or variant == "cancelled" else np.arange(n) % 2
    if two:
        d["target"][:, 1] = 1
    for f in ref.DV:
        d[f] = rng.uniform(-0.03, 0.03, d.shape + (3,))
    for f, g in zip(NORMALS, ref.DN):
        if variant == "cancelled":
            rest = (rng.integers(-8, 9, (n, 3)) / 8.0).astype(np.float32)
            tris[f][listed] = rest
            d[g][:, 0] = -rest
        else:
            tris[f][listed] = 0.0
            d[g][:, 0] = k2[idx][:, None] * unit_vectors(rng, n)
            if two:
                d[g][:, 1] = k2[idx + 1][:, None] * unit_vectors(rng, n)
    weights = {"one record": (0.5, 0.5), "two records": (0.75, -0.5), "cancelled": (1.0, 0.0)}[variant]
    row_start = (np.arange(n + 1) * d.shape[1]).astype(np.uint32)
    return fresh_scene(s, tris), listed, row_start, d.reshape(-1), np.array(weights, np.float32), idx


# ---- 2: weights as given ------------------------------------------------------------------------------------------------------------------
W_TARGETS = 14
SPECIAL_WEIGHTS = (1e-45, 1e-41, 0.7, -0.7, 1e30, 1e-30, -0.0, 0.0, 0.375, -0.0)         # of the targets 4 .. 13
PAD_BITS = np.array([0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x80000000], np.uint32)
PAD_FIELDS = ("_p0", "_p1", "_p2", "_p3", "_p4", "_p5")
PERIOD = 16
PATTERNS = ("1e-45 on an ordinary record", "1e-41 on an ordinary record", "1e-45 on a record of 1e30", "1e-41 on a record of 1e30",
            "w and -w on identical records", "1e30 on a record of 1e-30", "1e-30 on a record of 1e30", "only the last weight is not zero",
            "every weight is -0", "one denormal weight beside it")
APPLIED = (1, 1, 1, 1, 2, 1, 1, 1, 0, 1)             # records applied per pattern


def scaled(r, by):
    """the record with its 18 numbers multiplied by `by` in double and rounded once"""
    out = r.copy()
    for f in ref.DV + ref.DN:
        out[f] = (r[f].astype(np.float64) * by).astype(np.float32)
    return out


def morph_weights_case():
    """(scene, listed, row_start, deltas, weights): a third of cornell with a seeded table on the targets 0 .. 3, and pattern i of
    PATTERNS written over the row of the entries i, i + 16, ... on targets of their own (4 .. 13, SPECIAL_WEIGHTS). Every listed
    triangle's rest pose has v1.z = -0, n0 = (-0, 2, 0) (not unit) and the six padding words of PAD_BITS, rotated by entry."""
    s = scene("cornell")
    listed = listing_of(s, "third")
    n = len(listed)
    rng = np.random.default_rng(113)
    row_start, deltas = ref.table(rng, n, 4, (0, 1, 2, 3))
    w = np.concatenate([ref.weights_for(rng, 4, None), np.array(SPECIAL_WEIGHTS, np.float32)])
    tris = s.tris.copy()
    tris["v1"][listed, 2] = -0.0
    tris["n0"][listed] = (-0.0, 2.0, 0.0)
    for i, f in enumerate(PAD_FIELDS):
        tris[f][listed] = PAD_BITS[(np.arange(n) + i) % 4].view(np.float32)
    rows = {}
    for e in range(n):
        i = e % PERIOD
        if i >= len(PATTERNS):
            continue
        if i in (0, 1, 9):
            rows[e] = random_record(rng, 4 + (i == 1), positive=True)    # (no negative product: -0 + +0 is +0, -0 + -0 is not)
        elif i in (2, 3):
            rows[e] = scaled(random_record(rng, 4 + (i == 3), dv=1.0, dn=1.0), 1e30)
        elif i == 4:
            r = random_record(rng, 6)
            twin = r.copy()
            twin["target"] = 7
            rows[e] = np.concatenate([r, twin])
        elif i == 5:
            rows[e] = scaled(random_record(rng, 8), 1e-30)
        elif i == 6:
            rows[e] = scaled(random_record(rng, 9), 1e30)
        elif i == 7:
            rows[e] = np.concatenate([random_record(rng, t) for t in (10, 11, 12)])
        elif i == 8:
            rows[e] = np.concatenate([random_record(rng, t) for t in (10, 13)])
    row_start, deltas = with_rows(row_start, deltas, rows)
    return fresh_scene(s, tris), listed, row_start, deltas, w


# ---- 3: the edge of the vertex check ------------------------------------------------------------------------------------------------------
EDGE_ENTRIES = {"FLT_MAX": 7, "intermediate": 75, "nan": 203}       # list entries, in three blocks of the launch
EDGE_POSES = {"FLT_MAX exactly": ({4: 1.0}, None), "FLT_MAX + 2e31": ({4: 1.0, 5: 1.0}, "FLT_MAX"),
              "3e38 + 3e38 - 3e38 in row order": ({6: 1.0, 7: 1.0}, "intermediate"), "inf - inf": ({8: 2.0, 9: 2.0}, "nan"),
              "all three": ({4: 1.0, 5: 1.0, 6: 1.0, 7: 1.0, 8: 2.0, 9: 2.0}, "FLT_MAX")}


def vertex_edge_case():
    """(scene, the records the morph is set on, listed, row_start, deltas, the weights of an ordinary pose, {name: (weights, the entry
    that offends first or None)}): a third of cornell with a seeded table on the targets 0 .. 3; three entries have rows of their
    own, each on one component, and rest components that update_triangles writes before the morph is set.
    Entry 7: rest v2.y = 0, records FLT_MAX (target 4) and 2e31 (5). Entry 75: rest v0.x = 3e38, records +3e38 (6) and -3e38 (7).
    Entry 203: rest v1.z = 3e38, records +3e38 (8) and -3e38 (9), which weights of 2 take to +inf and -inf."""
    s = scene("cornell")
    listed = listing_of(s, "third")
    rng = np.random.default_rng(114)
    row_start, deltas = ref.table(rng, len(listed), 4, (0, 1, 2, 3))
    tris = s.tris.copy()
    e1, e2, e3 = (EDGE_ENTRIES[k] for k in ("FLT_MAX", "intermediate", "nan"))
    tris["v2"][listed[e1], 1] = 0.0
    tris["v0"][listed[e2], 0] = 3e38
    tris["v1"][listed[e3], 2] = 3e38
    rows = {e1: np.concatenate([record(4, dv2=(0, FLT_MAX, 0)), record(5, dv2=(0, 2e31, 0))]),
            e2: np.concatenate([record(6, dv0=(3e38, 0, 0)), record(7, dv0=(-3e38, 0, 0))]),
            e3: np.concatenate([record(8, dv1=(0, 0, 3e38)), record(9, dv1=(0, 0, -3e38))])}
    row_start, deltas = with_rows(row_start, deltas, rows)
    good = np.zeros(10, np.float32)
    good[:4] = ref.weights_for(rng, 4, None)
    poses = {}
    for name, (special, first) in EDGE_POSES.items():
        w = good.copy()
        for t, v in special.items():
            w[t] = v
        poses[name] = (w, None if first is None else EDGE_ENTRIES[first])
    return s, tris, listed, row_start, deltas, good, poses


# ---- 4: row shapes ------------------------------------------------------------------------------------------------------------------------
LONG = ref.MAX_TARGETS                                # 8 192: a row that names every target
LONG_ENTRY = 4


def long_row(rng):
    """8 192 records, one per target, small enough that their sum stays ordinary"""
    d = np.zeros(LONG, layout.MORPH_DELTA)
    d["target"] = np.arange(LONG)
    for f in ref.DV:
        d[f] = rng.uniform(-1e-3, 1e-3, (LONG, 3))
    for f in ref.DN:
        d[f] = rng.uniform(-1e-2, 1e-2, (LONG, 3))
    return d


def row_shape_case(kind):
    """(scene, listed, row_start, deltas). wave: a third of cornell; entry 4 has all 8 192 targets in its row, the other seven entries
    of its wave (0 - 3, 5 - 7) are empty and the rest have seeded rows of 0 .. 3 records. neighbours: the same with a row of one
    record, on target 8 191, in entry 5. one: tiny5, a list of one entry with 8 192 records."""
    rng = np.random.default_rng(115)
    if kind == "one":
        s = scene("tiny5")
        return s, np.array([2], np.uint32), np.array([0, LONG], np.uint32), long_row(rng)
    s = scene("cornell")
    listed = listing_of(s, "third")
    row_start, deltas = ref.table(rng, len(listed), LONG, (1, 2, 0, 3))
    rows = {e: deltas[:0] for e in range(8)}
    rows[LONG_ENTRY] = long_row(rng)
    if kind == "neighbours":
        rows[LONG_ENTRY + 1] = random_record(rng, LONG - 1)
    return (s, listed) + with_rows(row_start, deltas, rows)


def row_shape_poses(kind):
    """{name: weights}: only the last target, only the first, every target"""
    last, first = np.zeros(LONG, np.float32), np.zeros(LONG, np.float32)
    last[1::2], first[1::2] = -0.0, -0.0
    last[LONG - 1], first[0] = 0.625, -1.5
    everything = ref.weights_for(np.random.default_rng(116), LONG, None)
    if kind == "neighbours":
        return {"only target 8191": last}
    return {"only target 8191": last, "only target 0": first, "all 8192": everything}


# ---- 5: refusals with a skin in place -----------------------------------------------------------------------------------------------------
REFUSAL_TARGETS = 7                                   # test_gpu_morph_skin's 5, one for the entry in the skin (5), one for the other (6)
PLACEMENTS = {"an entry in the skin": (5,), "an entry outside it": (6,), "both": (5, 6)}


def skin_refusal_case():
    """test_gpu_morph_skin.sets with an overflowing record (test_gpu_morph.refusing's: 3e38 on one component, which weight 2 takes out
    of float32) behind the row of an entry in the skin, on target 5, and of a later entry outside it, on target 6.
    -> (scene, m_list, row_start, deltas, s_list, corners, (the entry in the skin, the entry outside))"""
    s = scene("cornell")
    m_list, row_start, deltas, s_list, corners, both = sets(s)
    in_skin = np.isin(m_list, both)
    e_in = int(np.flatnonzero(in_skin)[3])
    e_out = int(np.flatnonzero(~in_skin & (np.arange(len(m_list)) > e_in + 8))[0])
    rows = {e_in: np.concatenate([row_of(row_start, deltas, e_in), record(5, dv2=(0, 3e38, 0))]),
            e_out: np.concatenate([row_of(row_start, deltas, e_out), record(6, dv2=(0, 3e38, 0))])}
    row_start, deltas = with_rows(row_start, deltas, rows)
    return s, m_list, row_start, deltas, s_list, corners, (e_in, e_out)


def refusal_weights(seed, raised=()):
    w = ref.weights_for(np.random.default_rng(seed), REFUSAL_TARGETS, None)
    w[5:] = 0.0
    w[list(raised)] = 2.0
    return w


# ---- 6: morph, groups and skin on one context ---------------------------------------------------------------------------------------------
def three_way_case():
    """(scene, groups, the group moved, the morph's list, rows and records, the skin's list and corners): soup80, overlap_case's five
    groups and its skin over half the triangles, the morph over another seeded half"""
    s, groups, s_list, corners, g = overlap_case()
    m_list = listing_of(s, "half")
    row_start, deltas = ref.table(np.random.default_rng(117), len(m_list), 4, (2, 0, 1, 3))
    return s, groups, g, m_list, row_start, deltas, s_list, corners


def overlaps(groups, g, m_list, s_list):
    """the triangles of group g by which of the two lists name them: (morph only, skin only, both, neither)"""
    members = np.flatnonzero(groups == g)
    m, k = np.isin(members, m_list), np.isin(members, s_list)
    return members[m & ~k], members[~m & k], members[m & k], members[~m & ~k]


# ---- 8: motion with a mixed list ----------------------------------------------------------------------------------------------------------
def mixed_motion_case():
    """(scene, m_list, row_start, deltas, s_list, corners): a third of cornell morphed; the skin lists the two lowest and the two
    highest morphed triangles, every fifth of the others and a seeded tenth of the triangles the morph does not list"""
    s = scene("cornell")
    m_list = listing_of(s, "third")
    rng = np.random.default_rng(118)
    row_start, deltas = ref.table(rng, len(m_list), 3, (1, 2, 1))
    others = np.setdiff1d(np.arange(len(s.tris)), m_list)
    s_list = np.union1d(np.concatenate([m_list[:2], m_list[-2:], m_list[5:-5:5]]), rng.choice(others, len(others) // 10, replace=False))
    s_list = s_list.astype(np.uint32)
    return s, m_list, row_start, deltas, s_list, sref.random_corners(rng, len(s_list), N_JOINTS, 3)


def live_range(m_list, s_list):
    """[lowest, highest] of the morphed triangles the skin does not list: the live records a pose_morph writes"""
    out = np.setdiff1d(m_list, s_list)
    return int(out.min()), int(out.max())


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
def morph_counts(ctx):
    st = ctx.morph_status()
    return st.poses, st.first_bad, st.skin_stale


def refused(ctx, w, want, what):
    """pose_morph(w) is refused with first_bad = want and leaves the context and the morph's counters as they were"""
    from ptmi import native
    snap, ms = snapshot(ctx), ctx.morph_status()
    with pytest.raises(native.PtmiError) as e:
        ctx.pose_morph(w)
    assert e.value.code == E_INVALID, what
    now = ctx.morph_status()
    assert now.first_bad == want, f"{what}: first_bad {now.first_bad}, the model's {want}"
    assert (now.poses, now.pose_ms, now.active_targets, now.skin_stale) == (ms.poses, ms.pose_ms, ms.active_targets, ms.skin_stale), what
    unchanged(ctx, snap, what)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", MAGNITUDE_SCENES)
def test_morphed_normals_of_every_magnitude(ctx_a, ctx_b, name, variant):
    s, listed, row_start, deltas, w, idx = magnitude_case(scene(name), variant)
    moved = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
    assert all(np.isfinite(moved[f]).all() for f in tref.REST_FIELDS)
    assert (ref.applied_counts(row_start, deltas, w) > 0).all()
    for mode in MODES:
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_morph(listed, row_start, deltas, 2)
        ctx_a.pose_morph(w)
        got = ctx_a.read_triangles()
        for j in np.unique(idx):                                       # (per k, so that a failure names its class)
            sel = listed[idx == j]
            named = "rest - rest" if variant == "cancelled" else f"k = {LADDER[j]:g} ({CLASS_OF[LADDER[j]]})"
            for f in NORMALS:
                assert got[f][sel].tobytes() == moved[f][sel].tobytes(), f"{name} {mode} {variant}: {f} under {named}"
        equals_updated(ctx_a, ctx_b, moved, f"{name} {mode} {variant}")


@pytest.mark.parametrize("mode", [OWN, REFERENCE])
def test_weights_are_used_as_given(ctx_a, ctx_b, mode):
    s, listed, row_start, deltas, w = morph_weights_case()
    rest = tref.rest_of(s.tris)
    moved = ref.morphed(s.tris, rest, listed, row_start, deltas, w)
    assert no_nan(moved) and ref.first_bad(s.tris, rest, listed, row_start, deltas, w, own=mode[0] == 2) == NONE
    upload(ctx_a, s, mode)
    upload(ctx_b, s, mode)
    assert ctx_a.read_triangles().tobytes() == s.tris.tobytes()        # the upload keeps the padding words' bits
    ctx_a.set_morph(listed, row_start, deltas, W_TARGETS)
    ctx_a.pose_morph(w)
    st = ctx_a.morph_status()
    assert (st.poses, st.first_bad, st.active_targets) == (1, NONE, int(np.count_nonzero(w)))
    got = ctx_a.read_triangles()
    for i, what in enumerate(PATTERNS):                                # (per pattern, so that a failure names it)
        sel = listed[i::PERIOD]
        assert got[sel].tobytes() == moved[sel].tobytes(), f"{mode}: {what}"
    for f in PAD_FIELDS:
        assert got[f].tobytes() == s.tris[f].tobytes(), f"{mode}: padding word {f}"
    equals_updated(ctx_a, ctx_b, moved, f"weights as given {mode}")
    ctx_a.pose_morph(np.where(np.arange(W_TARGETS) % 2 == 0, 0.0, -0.0).astype(np.float32))
    equals_updated(ctx_a, ctx_b, s.tris, f"an all-zero pose {mode}")   # negative zeros, the normal that is not unit, the padding


def test_the_vertex_check_at_the_edge_of_float32(ctx_a, ctx_b):
    s, set_on, listed, row_start, deltas, good, poses = vertex_edge_case()
    rest = tref.rest_of(set_on)
    upload(ctx_a, s, REFERENCE)
    upload(ctx_b, s, REFERENCE)
    ctx_a.update_triangles(0, set_on)
    ctx_a.set_morph(listed, row_start, deltas, 10)
    ctx_a.pose_morph(good)
    live = ref.morphed(set_on, rest, listed, row_start, deltas, good)
    assert ctx_a.read_triangles().tobytes() == live.tobytes()
    for name, (w, entry) in poses.items():
        if entry is not None:
            assert ref.offenders(live, rest, listed, row_start, deltas, w, own=False)[0] == entry
            refused(ctx_a, w, int(listed[entry]), name)
    w, _ = poses["FLT_MAX exactly"]
    assert ref.first_bad(live, rest, listed, row_start, deltas, w, own=False) == NONE
    want = ref.morphed(live, rest, listed, row_start, deltas, w)
    assert want["v2"][listed[EDGE_ENTRIES["FLT_MAX"]], 1] == FLT_MAX and no_nan(want)
    ctx_a.pose_morph(w)
    assert morph_counts(ctx_a) == (2, NONE, 0)
    equals_updated(ctx_a, ctx_b, want, "a vertex at FLT_MAX")


@pytest.mark.parametrize("kind", ["wave", "neighbours", "one"])
def test_rows_of_8192_records_beside_empty_and_short_ones(ctx_a, ctx_b, kind):
    s, listed, row_start, deltas = row_shape_case(kind)
    rest = tref.rest_of(s.tris)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_morph(listed, row_start, deltas, LONG)
    assert ctx_a.morph_status().n_records == len(deltas)
    live = s.tris
    for i, (name, w) in enumerate(row_shape_poses(kind).items()):
        live = ref.morphed(live, rest, listed, row_start, deltas, w)
        assert no_nan(live)
        ctx_a.pose_morph(w)
        st = ctx_a.morph_status()
        assert (st.poses, st.first_bad, st.active_targets) == (i + 1, NONE, int(np.count_nonzero(w))), f"{kind}: {name}"
        equals_updated(ctx_a, ctx_b, live, f"{kind}: {name}")


def test_a_pose_refused_while_entries_go_to_the_skin(ctx_a, ctx_b):
    s, m_list, row_start, deltas, s_list, corners, (e_in, e_out) = skin_refusal_case()
    both = np.intersect1d(m_list, s_list)
    model = Composed(s.tris)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_skin(s_list, corners, N_JOINTS)
    ctx_a.set_morph(m_list, row_start, deltas, REFUSAL_TARGETS)
    model.set_skin(s_list, corners)
    model.set_morph(m_list, row_start, deltas)
    assert ctx_a.morph_status().n_in_skin == len(both)
    j1 = pose(N_JOINTS, 121)
    ctx_a.pose_morph(refusal_weights(122))
    ctx_a.pose_skin(joint_records(j1))
    model.pose_morph(refusal_weights(122))
    before = model.pose_skin(j1)
    assert ctx_a.read_triangles().tobytes() == before.tobytes() and no_nan(before)
    for i, (where, raised) in enumerate(PLACEMENTS.items()):
        bad = refusal_weights(123 + i, raised)                          # other weights throughout: every entry's result would differ
        entries = ref.offenders(model.live, model.m_rest, m_list, row_start, deltas, bad, own=True)
        assert entries.tolist() == [e for e, t in ((e_in, 5), (e_out, 6)) if t in raised], where
        assert morph_counts(ctx_a)[::2] == (1, 0), where                  # (first_bad keeps the last refusal's until a pose succeeds)
        refused(ctx_a, bad, int(m_list[entries[0]]), where)
        ctx_a.pose_skin(joint_records(j1))                              # from rest rows that the refused call has not written
        assert ctx_a.read_triangles().tobytes() == before.tobytes(), f"{where}: the skin's rest rows"
    w2, j2 = refusal_weights(126), pose(N_JOINTS, 127)
    ctx_a.pose_morph(w2)
    assert morph_counts(ctx_a) == (2, NONE, 1)
    model.pose_morph(w2)
    assert ctx_a.read_triangles().tobytes() == model.live.tobytes()
    ctx_a.pose_skin(joint_records(j2))
    equals_updated(ctx_a, ctx_b, model.pose_skin(j2), "after the refusals")


@pytest.mark.parametrize("order", ["morph first", "groups first"])
def test_morph_and_groups_keep_separate_rest_poses(ctx_a, ctx_b, order):
    """neither call re-bases the other's rest pose, and a triangle that is listed and a member takes the last writer's record"""
    s, groups, g, m_list, row_start, deltas, _, _ = three_way_case()
    rng = np.random.default_rng(128)
    w1, w2 = ref.weights_for(rng, 4, None), ref.weights_for(rng, 4, 3)
    model, alone = Composed(s.tris), Composed(s.tris)                  # alone: every step made on S, without the steps before it
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    if order == "morph first":
        ctx_a.set_morph(m_list, row_start, deltas, 4)
        ctx_a.set_triangle_groups(groups)
        steps = [("pose", w1), ("move", T1), ("pose", w2)]
    else:
        ctx_a.set_triangle_groups(groups)
        ctx_a.set_morph(m_list, row_start, deltas, 4)
        steps = [("move", T1), ("pose", w1), ("move", T2)]
    for m in (model, alone):
        m.set_groups(groups)
        m.set_morph(m_list, row_start, deltas)
    overlap = np.intersect1d(np.flatnonzero(groups == g), m_list)
    assert len(overlap) > 8
    for i, (kind, arg) in enumerate(steps):
        before = model.live
        alone.live = s.tris
        if kind == "pose":
            live, single = model.pose_morph(arg), alone.pose_morph(arg)
            ctx_a.pose_morph(arg)
        else:
            live, single = model.transform([tref.op(g, arg)]), alone.transform([tref.op(g, arg)])
            ctx_a.transform_groups(op_records([tref.op(g, arg)]))
        assert live[overlap].tobytes() != before[overlap].tobytes()    # the overlap takes this writer's record ...
        assert live[overlap].tobytes() == single[overlap].tobytes()    # ... which is its edit of S, not of the other's record
        equals_updated(ctx_a, ctx_b, live, f"{order}, step {i}: {kind}")
    assert ctx_a.scene_update_status().updates == 3


def test_morph_skin_and_groups_on_one_triangle(ctx_a, ctx_b):
    s, groups, g, m_list, row_start, deltas, s_list, corners = three_way_case()
    triple = overlaps(groups, g, m_list, s_list)[2]
    assert len(triple) > 8
    rng = np.random.default_rng(129)
    w1, w2 = ref.weights_for(rng, 4, None), ref.weights_for(rng, 4, None)
    j1, j2 = pose(4, 130), pose(4, 131)
    model = Composed(s.tris)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_triangle_groups(groups)
    ctx_a.set_skin(s_list, corners, 4)
    ctx_a.set_morph(m_list, row_start, deltas, 4)
    model.set_groups(groups)
    model.set_skin(s_list, corners)
    model.set_morph(m_list, row_start, deltas)
    calls = [("pose_morph", w1, 1), ("pose_skin", j1, 0), ("transform_groups", T1, 0), ("pose_morph", w2, 1), ("pose_skin", j2, 0)]
    for i, (call, arg, stale) in enumerate(calls):
        before = model.live
        if call == "pose_morph":
            live = model.pose_morph(arg)
            ctx_a.pose_morph(arg)
            assert live[triple].tobytes() == before[triple].tobytes()  # they wait for the skin, whoever wrote them last
        elif call == "pose_skin":
            live = model.pose_skin(arg)
            ctx_a.pose_skin(joint_records(arg))
            assert live[triple].tobytes() != before[triple].tobytes()
        else:
            live = model.transform([tref.op(g, arg)])
            ctx_a.transform_groups(op_records([tref.op(g, arg)]))
            assert live[triple].tobytes() == tref.transformed(s.tris, tref.rest_of(s.tris), groups, [tref.op(g, arg)])[triple].tobytes()
        assert no_nan(live) and ctx_a.morph_status().skin_stale == stale, f"call {i}: {call}"
        equals_updated(ctx_a, ctx_b, live, f"call {i}: {call}")
    assert ctx_a.scene_update_status().updates == 5


@pytest.mark.parametrize("which", ["a gap of the list", "the first listed", "the last listed", "everything"])
def test_morph_rebase_ranges(ctx_a, ctx_b, which):
    s = scene("soup80")
    listed = listing_of(s, "half")
    row_start, deltas = ref.table(np.random.default_rng(132), len(listed), 4, (1, 0, 3))
    lo, hi = rebase_ranges(listed, len(s.tris))[which]
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    assert edit.tobytes() != s.tris[lo:hi].tobytes()
    rng = np.random.default_rng(133)
    w1, w2 = ref.weights_for(rng, 4, None), ref.weights_for(rng, 4, None)
    model = Composed(s.tris)
    model.set_morph(listed, row_start, deltas)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_morph(listed, row_start, deltas, 4)
    ctx_a.pose_morph(w1)
    ctx_a.update_triangles(lo, edit)
    model.pose_morph(w1)
    assert ctx_a.read_triangles().tobytes() == model.update(lo, edit).tobytes()
    ctx_a.pose_morph(w2)                                               # listed triangles outside the range keep the old rest pose
    equals_updated(ctx_a, ctx_b, model.pose_morph(w2), which)


@pytest.mark.parametrize("stale", [0, 1])
def test_update_triangles_rebases_the_morph_and_the_skin(ctx_a, ctx_b, stale):
    """the records written are the rest pose of both for the triangles inside the range; a shared triangle outside it keeps its skin
    rest row, which with skin_stale = 1 is the morphed one that no pose_skin has carried to the live records yet"""
    s, _, _, m_list, row_start, deltas, s_list, corners = three_way_case()
    lo, hi = 37, 251
    shared = np.intersect1d(m_list, s_list)
    inside = (shared >= lo) & (shared < hi)
    assert inside.sum() > 8 and (~inside).sum() > 8                    # the range cuts through the shared triangles
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    rng = np.random.default_rng(134)
    w = [ref.weights_for(rng, 4, None) for _ in range(3)]
    j = [pose(4, 135 + i) for i in range(3)]
    model = Composed(s.tris)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_skin(s_list, corners, 4)
    ctx_a.set_morph(m_list, row_start, deltas, 4)
    model.set_skin(s_list, corners)
    model.set_morph(m_list, row_start, deltas)
    ctx_a.pose_morph(w[0])
    ctx_a.pose_skin(joint_records(j[0]))
    model.pose_morph(w[0])
    model.pose_skin(j[0])
    if stale:
        ctx_a.pose_morph(w[1])
        model.pose_morph(w[1])
    assert ctx_a.morph_status().skin_stale == stale
    ctx_a.update_triangles(lo, edit)
    assert ctx_a.read_triangles().tobytes() == model.update(lo, edit).tobytes()
    ctx_a.pose_skin(joint_records(j[1]))                               # the skin's rest rows as the update left them
    live = model.pose_skin(j[1])
    out = shared[~inside]
    carried = sref.skinned(live, tref.rest_of(ref.morphed(s.tris, tref.rest_of(s.tris), m_list, row_start, deltas, w[stale])), s_list, corners, j[1])
    assert live[out].tobytes() == carried[out].tobytes()               # outside the range: the rest row of the last morph pose
    rebased = s.tris.copy()
    rebased[lo:hi] = edit
    assert live[shared[inside]].tobytes() == sref.skinned(live, tref.rest_of(rebased), s_list, corners, j[1])[shared[inside]].tobytes()
    equals_updated(ctx_a, ctx_b, live, f"skin_stale {stale}: a skin pose after the edit")
    ctx_a.pose_morph(w[2])
    ctx_a.pose_skin(joint_records(j[2]))
    model.pose_morph(w[2])
    equals_updated(ctx_a, ctx_b, model.pose_skin(j[2]), f"skin_stale {stale}: both poses after the edit")


def test_a_morph_set_after_a_skin_pose_rests_on_the_skinned_records(ctx_a, ctx_b):
    s, _, _, m_list, row_start, deltas, s_list, corners = three_way_case()
    shared = np.intersect1d(m_list, s_list)
    w = ref.weights_for(np.random.default_rng(138), 4, None)
    j1, j2 = pose(4, 139), pose(4, 140)
    model = Composed(s.tris)
    upload(ctx_a, s, OWN)
    upload(ctx_b, s, OWN)
    ctx_a.set_skin(s_list, corners, 4)
    ctx_a.pose_skin(joint_records(j1))
    ctx_a.set_morph(m_list, row_start, deltas, 4)
    model.set_skin(s_list, corners)
    skinned = model.pose_skin(j1)
    model.set_morph(m_list, row_start, deltas)
    assert model.m_rest["v0"][shared].tobytes() == skinned["v0"][shared].tobytes() != s.tris["v0"][shared].tobytes()
    ctx_a.pose_morph(w)
    assert ctx_a.read_triangles().tobytes() == model.pose_morph(w).tobytes()
    ctx_a.pose_skin(joint_records(j2))
    live = model.pose_skin(j2)
    from_the_upload = sref.skinned(live, tref.rest_of(ref.morphed(s.tris, tref.rest_of(s.tris), m_list, row_start, deltas, w)), s_list, corners, j2)
    assert live[shared].tobytes() != from_the_upload[shared].tobytes()  # the shared triangles are skinned twice: INTEGRATION.md §1.16
    equals_updated(ctx_a, ctx_b, live, "a morph set on skinned records")


def test_motion_follows_a_pose_of_a_mixed_list(ctx_a, ctx_b):
    s, m_list, row_start, deltas, s_list, corners = mixed_motion_case()
    lo, hi = live_range(m_list, s_list)
    assert int(m_list.min()) < lo and hi < int(m_list.max())
    s_lo, s_hi = int(s_list.min()), int(s_list.max())
    w = np.array([0.8, -0.5, 0.6], np.float32)
    joints = pose(N_JOINTS, 141)
    model = Composed(s.tris)
    model.set_skin(s_list, corners)
    model.set_morph(m_list, row_start, deltas)
    morphed = model.pose_morph(w)
    skinned = model.pose_skin(joints)
    assert morphed[lo:hi + 1].tobytes() != s.tris[lo:hi + 1].tobytes() and skinned.tobytes() != morphed.tobytes()
    cam = layout.make_camera(96, 64, aperture=0.0)
    got = []
    try:
        for c in (ctx_a, ctx_b):
            upload(c, s, OWN)
            c.resize(96, 64)
            c.set_aovs("normal", "id")
            c.set_moments(True)
            c.set_motion(True)
            c.dispatch(cam, 4)
            if c is ctx_a:
                c.set_skin(s_list, corners, N_JOINTS)
                c.set_morph(m_list, row_start, deltas, 3)
                c.pose_morph(w)
            else:
                c.update_triangles(lo, morphed[lo:hi + 1])
            ms = c.motion_status()
            assert (ms.dirty_first, ms.dirty_count) == (lo, hi - lo + 1)
            if c is ctx_a:
                c.pose_skin(joint_records(joints))
            else:
                c.update_triangles(s_lo, skinned[s_lo:s_hi + 1])
            ms = c.motion_status()
            assert (ms.dirty_first, ms.dirty_count) == (min(lo, s_lo), max(hi, s_hi) - min(lo, s_lo) + 1)
            assert c.read_triangles().tobytes() == skinned.tobytes()
            c.reproject(cam, cam)
            got.append((c.read_motion(), c.read_output(), c.read_moments(), c.read_aov("normal"), c.read_aov("id"), c.motion_status().moved))
    finally:
        for c in (ctx_a, ctx_b):
            c.set_motion(False)
            c.set_aovs()
            c.set_moments(False)
    for x, y, what in zip(got[0][:5], got[1][:5], ("motion", "output", "moments", "normal", "id")):
        assert x.tobytes() == y.tobytes(), what
    assert got[0][5] == got[1][5]
