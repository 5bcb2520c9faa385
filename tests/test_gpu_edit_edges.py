"""ptmi_transform_groups and ptmi_pose_skin (csrc/scene_transform.hip k_transform, csrc/scene_skin.hip k_skin, csrc/pt_transform.h) where
the small scenes of tests/test_gpu_transform.py and tests/test_gpu_skin.py do not reach.

The rule is theirs: context A uploads S and edits it on the device; context B uploads S and calls update_triangles(0, the model's
records) (tests/transform_ref.py, tests/skin_ref.py: the header's arithmetic in float32 numpy). same_state(A, B) must hold and A's live
records must be the model's bytes. No tolerance, no renders, no oracle: these cases are about the edit kernels.

A. More than one round of the grid-stride loop. Both kernels launch at most cus * 8 blocks of 32 triangles (or list entries), so one
   round is R = cus * 256 of them. The scene is the smallest grid_1m(n) with more than 1.2 R triangles whose count beyond R is no
   multiple of 8 (so round two ends in a partial block and a partial wave): n = 200, 79 212 triangles on 256 CUs. Every case asserts
   count > R itself, so a larger device cannot turn it into a one-round case unnoticed.
B. Refusals decided across rounds, blocks, chunks and instantiations: the offenders sit at chosen positions of the walk (entry R + 5:
   round two, block 0; R - 3: the last block of round one; the last entry: a partial wave of round two; ...), with up to 512 joints
   (LDS) and with 600 (k_skin<false, false> reads them from global memory), and for the groups with 1 025 ops, which are three
   launches that share the first_bad word. The model says which entries offend before the device is asked (the same assertion runs
   without a device in tests/test_edit_edges_host.py). Then the counts at the 512 boundary, on grid80: 512 and 513 joints, 512, 513
   and 1 025 ops.
C. Normal magnitudes: nm = k * I for k in LADDER, which takes q to the denormals, l2 to zero with q != 0, l2 to the denormals, l2 to
   just under the largest float and l2 to infinity (tests/test_edit_edges_host.py shows that each k reaches its class on these scenes
   and that the model's output holds no NaN, whose payload a byte comparison would depend on).
D. Weights as given: negative weights, sums of 0.25 and 3, a corner of four zero weights, one joint in all four slots, a zero-weight
   slot on a mirror joint whose record keeps its negative zeros.
E. A skin and groups on one context: separate rest poses, the last writer's record on the overlap, update_triangles re-bases both;
   and the ranges of skin_rebase: one without a listed triangle, exactly the first, exactly the last, everything.
F. The alignment of k_transform's range: it starts at lo & ~7 and ends at hi + 1, with lo % 8 = 3 and (hi + 1) % 8 = 5 here, and a
   group that is the last triangle alone.

The functions down to "the device" build the cases and need no device; tests/test_edit_edges_host.py imports them."""
import functools
import subprocess
import sys

import numpy as np
import pytest

import scene_update_ref as uref
import skin_ref as ref
import transform_ref as tref
from test_gpu_scene_update import ctx_a, ctx_b, scene  # noqa: F401 (fixtures)
from test_gpu_skin import pose, skin_for
from test_gpu_skin import records as joint_records
from test_gpu_transform import grouping, same_state
from test_gpu_transform import records as op_records

pytestmark = pytest.mark.gpu

E_INVALID = -1
NONE = 0xFFFFFFFF
VERTS = ("v0", "v1", "v2")
NORMALS = ("n0", "n1", "n2")
OCTETS = 32                                          # triangles (list entries) per block and round in both kernels
MODES = ((2, 2, 0), (1, 2, 0))                       # (leaves, tree_builder, keep_reference_tree): own and reference leaves, the device builder
MI355X_CUS = 256                                     # what the host test sizes the cases by

# ---- A: a scene of more than one round --------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def device_cus():
    """torch's multi_processor_count of device 0, the number csrc/ptmi_api.hip keeps in n_cu. Asked once per session, in a child
    process: torch brings a HIP runtime of its own, which finds no device in a process where the library's has opened it already."""
    ask = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    return int(subprocess.check_output([sys.executable, "-c", ask], text=True).split()[-1])


def round_of(cus):
    """triangles (list entries) one round of either kernel covers: cus * 8 blocks of 32"""
    return cus * 8 * OCTETS


def big_scene(cus):
    """the smallest grid_1m(n) with more than 1.2 rounds of triangles whose count beyond one round is no multiple of 8 (nor of 32)"""
    R = round_of(cus)
    n = 2
    while 2 * (n - 1) ** 2 + 10 <= 1.2 * R:
        n += 1
    while (2 * (n - 1) ** 2 + 10 - R) % 8 == 0 or (2 * (n - 1) ** 2 + 10 - R) % 32 == 0:
        n += 1
    s = scene(f"grid{n}")
    count = len(s.tris)
    assert count == 2 * (n - 1) ** 2 + 10
    assert count > R and (count - R) % 32 != 0 and (count - R) % 8 != 0, (count, R)
    return s


def where(entry, cus):
    """(round, block, wave of the block, octet of the wave) that walks entry `entry` of a launch"""
    R = round_of(cus)
    return entry // R, entry % R // OCTETS, entry % OCTETS // 8, entry % 8


def rotations(n, seed):
    """n small seeded rotations with a small shift, as 3 x 4 matrices"""
    rng = np.random.default_rng(seed)
    return [tref.affine(tref.rot_y(rng.uniform(-0.3, 0.3)), shift=rng.uniform(-0.02, 0.02, 3)) for _ in range(n)]


def groups_of(n_tris, n_groups, seed):
    return np.random.default_rng(seed).integers(0, n_groups, n_tris).astype(np.uint32)


def ops_on_all(n_groups, seed):
    """one op per group, in a seeded order"""
    order = np.random.default_rng(seed).permutation(n_groups)
    return [tref.op(int(g), m) for g, m in zip(order, rotations(n_groups, seed + 1))]


def round_transform(s, kind, cus):
    """(groups, ops) of a section A case: one op on a group of `random5`, whose range is the whole array, or all 600 ops of a
    600-group table, two launches. Every launch makes a second round that ends off a block."""
    n, R = len(s.tris), round_of(cus)

    def two_rounds(ranges):
        return all(end - first > R and (end - first - R) % OCTETS != 0 for first, end in ranges)

    if kind == "one op":
        groups = grouping(s, "random5")
        ops = [tref.op(int(groups[n // 2]), T1)]
    else:
        ops = ops_on_all(600, 65)
        for seed in range(66, 98):                                     # (the first seeded table whose two launches both end off a block)
            groups = groups_of(n, 600, seed)
            if two_rounds(tref.launch_ranges(groups, ops)):
                break
    ranges = tref.launch_ranges(groups, ops)
    assert len(ranges) == (len(ops) + 511) // 512 and two_rounds(ranges), ranges
    return groups, ops


# ---- B: refusals at chosen places of the walk -------------------------------------------------------------------------------------------
# The first row (3e38, 0, 0, 3e38) gives x' = 3e38 x + 3e38, which leaves float32 where x > 0.14; every entry is finite, so the host's
# argument check passes. Offenders are chosen among triangles whose three x exceed 0.5.
BAD_M = np.array([3e38, 0, 0, 3e38, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
BAD = (BAD_M, np.eye(3, dtype=np.float32).reshape(9))


def offender_sets(R, count):
    """entries of a launch over `count` entries, by where they are walked (check_places). A block walks 32 entries, so R + 5 and
    R + 40 fall to neighbouring blocks of round two, and R + 5 and R + 12 to two waves of one block."""
    return {"round two, block 0": [R + 5],
            "the last block of round one against block 0 of round two": [R - 3, R + 5],
            "the last entry, in a partial wave of round two": [count - 1],
            "blocks 0 and 1 of round two": [R + 5, R + 40],
            "two waves of one block in round two": [R + 5, R + 12]}


def refusal_window(tris, cus):
    """[k, end): the triangles a refusal case walks, k a multiple of 8, chosen so that the entries R - 3, R + 5, R + 12, R + 40 and
    the last one (entry e is triangle k + e) have all three x above 0.5, the walk is longer than a round and round two ends in a
    partial wave and a partial block"""
    R = round_of(cus)
    x = np.stack([tris[f][:, 0] for f in VERTS], axis=1)
    ok = (x > 0.5).all(axis=1)
    n = len(tris)
    for end in range(n, R + 64, -1):
        if not ok[end - 1]:
            continue
        for k in range(0, end - R - 64, 8):
            if ok[k + R - 3] and ok[k + R + 5] and ok[k + R + 12] and ok[k + R + 40] and (end - k - R) % 8 and (end - k - R) % 32:
                return k, end
    raise AssertionError("no window of this scene puts the offenders where x > 0.5")


def check_places(entries, which, cus, count):
    """the entries of an offender set are walked where the set's name says"""
    R = round_of(cus)
    at = {e: where(e, cus) for e in entries}
    assert count > R
    if R + 5 in at:
        assert at[R + 5] == (1, 0, 0, 5)
    if R - 3 in at:
        assert at[R - 3] == (0, cus * 8 - 1, 3, 5)
    if R + 40 in at:
        assert at[R + 40] == (1, 1, 1, 0)
    if R + 12 in at:
        assert at[R + 12] == (1, 0, 1, 4)
    if count - 1 in at:
        assert at[count - 1][0] == 1 and count % 8 != 0 and count % OCTETS != 0, which    # idle octets after it in its wave, idle waves in its block


def skin_refusal(tris, cus, n_joints, entries):
    """(listed, corners): the list is the window; the entries `entries` are one-hot on the last joint, which nothing else names.
    Every other joint is referenced where there are more than 512 (the instantiation that reads them from global memory)."""
    k, end = refusal_window(tris, cus)
    listed = np.arange(k, end, dtype=np.uint32)
    corners = ref.random_corners(np.random.default_rng(51), len(listed), n_joints - 1, 2, cover=n_joints > 512).reshape(-1, 3)
    corners[np.asarray(entries)] = ref.one_hot(np.full(len(entries), n_joints - 1)).reshape(-1, 3)
    assert len(np.unique(corners["joint"])) == n_joints or n_joints <= 512
    return listed, corners.reshape(-1)


def bad_pose(n_joints, seed):
    """(a good pose, the same with the last joint's matrix replaced by BAD)"""
    good = pose(n_joints, seed)
    return good, good[:-1] + [ref.joint(*BAD)]


def group_refusal(tris, cus, entries):
    """(groups, ops) of one launch: group 0 is everything outside the window and is never named, groups 1 to 4 share the window at
    random, group 5 has the entries alone and gets BAD"""
    k, end = refusal_window(tris, cus)
    groups = np.zeros(len(tris), np.uint32)
    groups[k:end] = np.random.default_rng(52).integers(1, 5, end - k)
    groups[k + np.asarray(entries)] = 5
    good = rotations(4, 53)
    ops = [tref.op(2, good[0]), tref.op(4, good[1]), tref.op(5, *BAD), tref.op(1, good[2]), tref.op(3, good[3])]
    return groups, ops


def chunk_sets(R):
    """1 025 ops are launches of 512, 512 and 1: (the entries of the bad group named in the first chunk, those of the one named last)"""
    return {"the third chunk alone": ([], [R + 5]),
            "the first chunk holds the smaller triangle": ([R - 3], [R + 5]),
            "the third chunk holds the smaller triangle": ([R + 5], [R - 3])}


def chunked_refusal(tris, cus, first_entries, third_entries):
    """(groups, 1 025 ops): groups 1 to 1 024 share the window at random and get rotations; group 1 025 has `third_entries` alone and
    is the last op (the third launch); group 1 026 has `first_entries` alone and, where there are any, is op 100 in place of a good one"""
    k, end = refusal_window(tris, cus)
    groups = np.zeros(len(tris), np.uint32)
    groups[k:end] = np.random.default_rng(54).integers(1, 1025, end - k)
    groups[k + np.asarray(third_entries, np.int64)] = 1025
    groups[k + np.asarray(first_entries, np.int64)] = 1026
    ops = [tref.op(int(g) + 1, m) for g, m in zip(np.random.default_rng(55).permutation(1024), rotations(1024, 56))]
    if len(first_entries):
        ops[100] = tref.op(1026, *BAD)
    ops.append(tref.op(1025, *BAD))
    assert len(ops) == 1025
    return groups, ops


# ---- C: normal magnitudes -------------------------------------------------------------------------------------------------------------------
LADDER = (1e-41, 1e-25, 3e-23, 1e-20, 1.8e19, 1e25)
# the class of tref.normal_classes each k is there to reach
CLASS_OF = {1e-41: "q_denormal", 1e-25: "l2_zero", 3e-23: ("l2_zero", "l2_denormal"), 1e-20: "l2_denormal", 1.8e19: "l2_large", 1e25: "l2_inf"}
MAGNITUDE_SCENES = ("cornell", "grid80", "soup80")


def ladder_records(seed):
    """one (m, nm) per k: m a small rotation, so the vertices stay ordinary, and nm = k * I given explicitly"""
    return [ref.joint(m, np.float32(k) * np.eye(3, dtype=np.float32)) for m, k in zip(rotations(len(LADDER), seed), LADDER)]


def ladder_groups(s):
    """a group per k, and a seventh that no op names"""
    return groups_of(len(s.tris), len(LADDER) + 1, 57)


def ladder_ops(seed=58):
    return [(g, m, nm) for g, (m, nm) in enumerate(ladder_records(seed))]


def ladder_skin(s, blended):
    """(listed, corners): every triangle, one-hot on the joint of its k; blended: two influences, the joints of neighbouring k"""
    n = len(s.tris)
    rng = np.random.default_rng(59)
    listed = np.arange(n, dtype=np.uint32)
    j = rng.integers(0, len(LADDER) - (1 if blended else 0), 3 * n).astype(np.uint32)
    corners = ref.one_hot(j[::3]).reshape(-1)
    if blended:
        w = rng.uniform(0.1, 0.9, 3 * n).astype(np.float32)
        corners["joint"][:, 0], corners["joint"][:, 1] = j, j + 1
        corners["weight"][:, 0], corners["weight"][:, 1] = w, np.float32(1.0) - w
    return listed, corners


# ---- D: weights as given --------------------------------------------------------------------------------------------------------------------
MIRROR_JOINT = 2
PATTERNS = [((0, 1, 0, 0), (1.5, -0.5, 0.0, 0.0)),                 # a negative weight, cancellation
            ((0, 1, 3, 0), (0.1, 0.1, 0.05, 0.0)),                 # a sum of 0.25
            ((0, 1, 2, 3), (1.0, 1.0, 0.5, 0.5)),                  # a sum of 3, the mirror among them
            ((1, 0, 3, 2), (0.0, 0.0, 0.0, 0.0)),                  # four zero weights: the vertex collapses to the model's signed zeros
            ((3, 3, 3, 3), (0.25, 0.25, 0.25, 0.25)),              # one joint in all four slots
            ((0, 1, 2, 2), (0.6, 0.4, 0.0, 0.0))]                  # zero-weight slots on the mirror: 0 * -0, 0 * -1


def weights_case():
    """(scene, listed, corners, joints): cornell, a third listed, four joints of which MIRROR_JOINT is a mirror (scale (-1, 1, 1), turned a
    little about y: the cofactors of the plain mirror hold no negative zero, these do) whose record is passed as it is, and the PATTERNS written over a seeded base: pattern i on all three corners of the entries
    i, i + 12, ..., and on corner 1 alone of the entries i + 6, i + 18, ..."""
    s = scene("cornell")
    listed, corners = skin_for(s, "third", 4, 3)
    joints = pose(4, 61)
    joints[MIRROR_JOINT] = ref.joint_raw(tref.affine(tref.rot_y(-0.2), scale=(-1, 1, 1), shift=(0.1, 0, 0)))
    c = corners.reshape(-1, 3).copy()
    for i, (j, w) in enumerate(PATTERNS):
        c["joint"][i::12], c["weight"][i::12] = j, w
        c["joint"][i + 6::12, 1], c["weight"][i + 6::12, 1] = j, w
    return s, listed, c.reshape(-1), joints


# ---- E: a skin and groups on one context ----------------------------------------------------------------------------------------------------
T1 = tref.affine(tref.rot_y(0.4), shift=(0.05, 0.02, -0.03))
T2 = tref.affine(scale=(-1, 1, 1), shift=(0.1, 0, 0))


def overlap_case():
    """(scene, groups, listed, corners, the group moved): soup80, five random groups, half the triangles listed; the moved group is
    about half listed"""
    s = scene("soup80")
    groups = grouping(s, "random5")
    listed, corners = skin_for(s, "half", 4, 3)
    g = 2
    both = np.isin(np.flatnonzero(groups == g), listed)
    assert both.any() and not both.all()
    return s, groups, listed, corners, g


def rebase_ranges(listed, n):
    """[lo, hi) of the update_triangles calls: a gap of the list, exactly its first triangle, exactly its last, everything"""
    gap = int(np.flatnonzero(np.diff(listed.astype(np.int64)) > 2)[0])
    ranges = {"a gap of the list": (int(listed[gap]) + 1, int(listed[gap + 1])), "the first listed": (int(listed[0]), int(listed[0]) + 1),
              "the last listed": (int(listed[-1]), int(listed[-1]) + 1), "everything": (0, n)}
    lo, hi = ranges["a gap of the list"]
    assert hi - lo >= 2 and not ((listed >= lo) & (listed < hi)).any()
    return ranges


# ---- F: the alignment of k_transform's range ------------------------------------------------------------------------------------------------
ALIGN_LO, ALIGN_HI = 8 * 37 + 3, 8 * 911 + 4                         # members [lo, hi]: lo % 8 = 3, (hi + 1) % 8 = 5


def aligned_groups(n):
    groups = np.zeros(n, np.uint32)
    groups[ALIGN_LO:ALIGN_HI + 1] = 1
    groups[n - 1] = 2
    assert ALIGN_LO > 8 and ALIGN_LO % 8 == 3 and (ALIGN_HI + 1) % 8 == 5 and ALIGN_HI + 8 < n - 1
    return groups


# ---- the device -----------------------------------------------------------------------------------------------------------------------------
def upload(ctx, s, mode):
    from ptmi import native
    leaves, builder, keep = mode
    ctx.set_options(leaves=leaves, tree_builder=builder, keep_reference_tree=keep, traversal=native.TRAVERSAL_AUTO, cull=1)
    ctx.upload_scene(s)


def equals_updated(ctx_a, ctx_b, want, what):
    """A's live records are the model's bytes, and A is in the state of B (which holds the same upload) updated with them"""
    assert ctx_a.read_triangles().tobytes() == want.tobytes(), f"{what}: live records against the model"
    ctx_b.update_triangles(0, want)
    same_state(ctx_a, ctx_b, what)


def skin_counts(ctx):
    st = ctx.skin_status()
    return st.present, st.n_joints, st.n_skinned, st.poses, st.first_bad


def group_counts(ctx):
    st = ctx.transform_status()
    return st.present, st.n_groups, st.transforms, st.last_moved, st.first_bad


def snapshot(ctx):
    return ctx.read_triangles(), ctx.read_image(), bytes(ctx.scene_update_status())


def unchanged(ctx, snap, what):
    tris, image, upd = snap
    assert ctx.read_triangles().tobytes() == tris.tobytes(), f"{what}: live records"
    again = ctx.read_image()
    assert bytes(again[0]) == bytes(image[0]), f"{what}: image header"
    assert all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(image[1:], again[1:])), f"{what}: image"
    assert bytes(ctx.scene_update_status()) == upd, f"{what}: scene_update_status"


@pytest.mark.parametrize("n_joints,influences", [(7, 4), (600, 2)])
def test_a_pose_of_more_than_one_round(ctx_a, ctx_b, n_joints, influences):
    cus = device_cus()
    s = big_scene(cus)
    n = len(s.tris)
    assert n > cus * 256
    listed = np.arange(n, dtype=np.uint32)
    corners = ref.random_corners(np.random.default_rng(62), n, n_joints, influences, cover=n_joints > 512)
    assert len(np.unique(corners["joint"])) == n_joints
    joints = pose(n_joints, 63)
    moved = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    assert (moved[-1:].tobytes() != s.tris[-1:].tobytes()) and moved[round_of(cus):].tobytes() != s.tris[round_of(cus):].tobytes()
    for mode in MODES:
        what = f"{s.name} {n_joints} joints {mode}"
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_skin(listed, corners, n_joints)
        ctx_a.pose_skin(joint_records(joints))
        assert skin_counts(ctx_a) == (1, n_joints, n, 1, NONE), what
        equals_updated(ctx_a, ctx_b, moved, what)


@pytest.mark.parametrize("kind", ["one op", "600 ops"])
def test_a_transform_of_more_than_one_round(ctx_a, ctx_b, kind):
    cus = device_cus()
    s = big_scene(cus)
    n, R = len(s.tris), round_of(cus)
    assert n > cus * 256
    groups, ops = round_transform(s, kind, cus)
    members = int(np.isin(groups, [g for g, _, _ in ops]).sum())
    moved = tref.transformed(s.tris, tref.rest_of(s.tris), groups, ops)
    assert moved[R:].tobytes() != s.tris[R:].tobytes()
    for mode in MODES:
        what = f"{s.name} {kind} {mode}"
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_triangle_groups(groups)
        ctx_a.transform_groups(op_records(ops))
        assert group_counts(ctx_a) == (1, int(groups.max()) + 1, 1, members, NONE), what
        equals_updated(ctx_a, ctx_b, moved, what)


@pytest.mark.parametrize("n_joints", [512, 600])
def test_a_pose_refused_in_another_round_block_or_wave(ctx_a, ctx_b, n_joints):
    """512 joints: the last launch that keeps them in LDS (48 KB). 600: k_skin<false, false> refuses."""
    from ptmi import native
    cus = device_cus()
    s = big_scene(cus)
    R = round_of(cus)
    k, end = refusal_window(s.tris, cus)
    count = end - k
    assert count > cus * 256
    rest = tref.rest_of(s.tris)
    good, bad = bad_pose(n_joints, 66)
    upload(ctx_a, s, MODES[0])
    upload(ctx_b, s, MODES[0])
    for which, entries in offender_sets(R, count).items():
        check_places(entries, which, cus, count)
        listed, corners = skin_refusal(s.tris, cus, n_joints, entries)
        ctx_a.update_triangles(0, s.tris)                              # the rest pose of every set is S
        ctx_a.set_skin(listed, corners, n_joints)
        ctx_a.pose_skin(joint_records(good))
        live = ref.skinned(s.tris, rest, listed, corners, good)
        assert np.array_equal(ref.offenders(live, rest, listed, corners, bad, own=True), np.sort(entries)), which
        want = ref.first_bad(live, rest, listed, corners, bad, own=True)
        assert want == k + min(entries)
        snap, sk = snapshot(ctx_a), ctx_a.skin_status()
        assert snap[0].tobytes() == live.tobytes(), which
        with pytest.raises(native.PtmiError) as e:
            ctx_a.pose_skin(joint_records(bad))
        assert e.value.code == E_INVALID, which
        now = ctx_a.skin_status()
        assert now.first_bad == want, f"{which}: first_bad {now.first_bad}, the model's {want}"
        assert (now.poses, now.pose_ms) == (sk.poses, sk.pose_ms) == (1, sk.pose_ms), which
        unchanged(ctx_a, snap, which)
    p2 = pose(n_joints, 67)                                            # the next valid call gives the usual bits
    ctx_a.pose_skin(joint_records(p2))
    assert skin_counts(ctx_a) == (1, n_joints, count, 2, NONE)
    equals_updated(ctx_a, ctx_b, ref.skinned(live, rest, listed, corners, p2), f"{n_joints} joints after the refusals")


def refused_transforms(ctx_a, s, cases):
    """every (name, groups, ops, the entries expected, k) of `cases` is refused with the model's first_bad and changes nothing; returns
    the live records, groups and rest pose the last of them left"""
    from ptmi import native
    rest = tref.rest_of(s.tris)
    warm = [tref.op(1, T1)]
    for which, groups, ops, entries, k in cases:
        ctx_a.update_triangles(0, s.tris)                              # the rest pose of every set is S
        ctx_a.set_triangle_groups(groups)
        ctx_a.transform_groups(op_records(warm))
        live = tref.transformed(s.tris, rest, groups, warm)
        assert np.array_equal(tref.offenders(live, rest, groups, ops, own=True), k + np.sort(entries)), which
        want = tref.first_bad(live, rest, groups, ops, own=True)
        snap, tf = snapshot(ctx_a), ctx_a.transform_status()
        assert snap[0].tobytes() == live.tobytes(), which
        with pytest.raises(native.PtmiError) as e:
            ctx_a.transform_groups(op_records(ops))
        assert e.value.code == E_INVALID, which
        now = ctx_a.transform_status()
        assert now.first_bad == want, f"{which}: first_bad {now.first_bad}, the model's {want}"
        assert (now.transforms, now.last_moved, now.transform_ms) == (tf.transforms, tf.last_moved, tf.transform_ms), which
        assert tf.transforms == 1
        unchanged(ctx_a, snap, which)
    return live, groups, rest


def test_a_transform_refused_in_another_round_block_or_wave(ctx_a, ctx_b):
    cus = device_cus()
    s = big_scene(cus)
    R = round_of(cus)
    k, end = refusal_window(s.tris, cus)
    assert end - k > cus * 256
    cases = []
    for which, entries in offender_sets(R, end - k).items():
        check_places(entries, which, cus, end - k)
        groups, ops = group_refusal(s.tris, cus, entries)
        assert tref.launch_ranges(groups, ops) == [(k, end)]           # entry e of the launch is triangle k + e
        cases.append((which, groups, ops, entries, k))
    upload(ctx_a, s, MODES[0])
    upload(ctx_b, s, MODES[0])
    live, groups, rest = refused_transforms(ctx_a, s, cases)
    ops = [tref.op(3, T2), tref.op(5, T1)]                             # the next valid call gives the usual bits: the bad group too
    ctx_a.transform_groups(op_records(ops))
    assert group_counts(ctx_a) == (1, 6, 2, int(np.isin(groups, (3, 5)).sum()), NONE)
    equals_updated(ctx_a, ctx_b, tref.transformed(live, rest, groups, ops), "after the refusals")


def test_a_transform_refused_across_chunks_of_ops(ctx_a, ctx_b):
    """1 025 ops: launches of 512, 512 and 1 op that share the first_bad word; the smallest triangle wins whichever launch finds it"""
    cus = device_cus()
    s = big_scene(cus)
    R = round_of(cus)
    k, end = refusal_window(s.tris, cus)
    assert end - k > cus * 256
    cases = []
    for which, (first_entries, third_entries) in chunk_sets(R).items():
        groups, ops = chunked_refusal(s.tris, cus, first_entries, third_entries)
        ranges = tref.launch_ranges(groups, ops)
        assert len(ranges) == 3 and ranges[0][0] == k and ranges[0][1] - k > R and ranges[1][1] - ranges[1][0] > R, which
        assert ranges[2] == ((k + third_entries[0]) & ~7, k + third_entries[0] + 1), which
        for e in first_entries:                                        # in the first launch the entries are walked where their names say
            check_places([e], which, cus, ranges[0][1] - k)
        cases.append((which, groups, ops, first_entries + third_entries, k))
    upload(ctx_a, s, MODES[0])
    upload(ctx_b, s, MODES[0])
    live, groups, rest = refused_transforms(ctx_a, s, cases)
    ops = [o for o in ops if o[0] < 1025]                              # the next valid call: the 1 023 good ops of the last case
    assert len(ops) == 1023
    ctx_a.transform_groups(op_records(ops))
    assert group_counts(ctx_a) == (1, 1027, 2, int(np.isin(groups, [g for g, _, _ in ops]).sum()), NONE)
    equals_updated(ctx_a, ctx_b, tref.transformed(live, rest, groups, ops), "after the refusals")


@pytest.mark.parametrize("n_joints", [512, 513])
def test_joint_counts_at_the_lds_boundary(ctx_a, ctx_b, n_joints):
    s = scene("grid80")
    listed = skin_for(s, "half", n_joints)[0]
    corners = ref.random_corners(np.random.default_rng(68), len(listed), n_joints, 2, cover=True)
    assert len(np.unique(corners["joint"])) == n_joints                # every joint is referenced
    joints = pose(n_joints, 69)
    moved = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    for mode in MODES:
        what = f"grid80 {n_joints} joints {mode}"
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_skin(listed, corners, n_joints)
        ctx_a.pose_skin(joint_records(joints))
        assert skin_counts(ctx_a) == (1, n_joints, len(listed), 1, NONE), what
        equals_updated(ctx_a, ctx_b, moved, what)


@pytest.mark.parametrize("n_ops", [512, 513, 1025])
def test_op_counts_at_the_chunk_boundary(ctx_a, ctx_b, n_ops):
    s = scene("grid80")
    groups, ops = groups_of(len(s.tris), n_ops, 70), ops_on_all(n_ops, 71)
    assert int(groups.max()) + 1 == n_ops and len(tref.launch_ranges(groups, ops)) == (n_ops + 511) // 512
    members = int(np.isin(groups, [g for g, _, _ in ops]).sum())
    moved = tref.transformed(s.tris, tref.rest_of(s.tris), groups, ops)
    for mode in MODES:
        what = f"grid80 {n_ops} ops {mode}"
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_triangle_groups(groups)
        ctx_a.transform_groups(op_records(ops))
        assert group_counts(ctx_a) == (1, n_ops, 1, members, NONE), what
        equals_updated(ctx_a, ctx_b, moved, what)


@pytest.mark.parametrize("name", MAGNITUDE_SCENES)
def test_transformed_normals_of_every_magnitude(ctx_a, ctx_b, name):
    s = scene(name)
    groups, ops = ladder_groups(s), ladder_ops()
    moved = tref.transformed(s.tris, tref.rest_of(s.tris), groups, ops)
    assert not any(np.isnan(moved[f]).any() for f in NORMALS)
    for mode in MODES:
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_triangle_groups(groups)
        ctx_a.transform_groups(op_records(ops))                        # one op per k in a single call
        for g, k in enumerate(LADDER):                                 # (per k, so that a failure names its class)
            sel = groups == g
            got = ctx_a.read_triangles()[sel]
            for f in NORMALS:
                assert got[f].tobytes() == moved[f][sel].tobytes(), f"{name} {mode}: {f} under nm = {k:g} * I ({CLASS_OF[k]})"
        equals_updated(ctx_a, ctx_b, moved, f"{name} {mode}")


@pytest.mark.parametrize("blended", [False, True])
@pytest.mark.parametrize("name", MAGNITUDE_SCENES)
def test_skinned_normals_of_every_magnitude(ctx_a, ctx_b, name, blended):
    s = scene(name)
    listed, corners = ladder_skin(s, blended)
    joints = ladder_records(60)
    moved = ref.skinned(s.tris, tref.rest_of(s.tris), listed, corners, joints)
    assert not any(np.isnan(moved[f]).any() for f in NORMALS)
    first = corners["joint"].reshape(-1, 3, 4)[:, :, 0]
    for mode in MODES:
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_skin(listed, corners, len(LADDER))
        ctx_a.pose_skin(joint_records(joints))
        got = ctx_a.read_triangles()
        for j, k in enumerate(LADDER):                                 # (per k, so that a failure names its class)
            for c, f in enumerate(NORMALS):
                sel = first[:, c] == j
                assert got[f][sel].tobytes() == moved[f][sel].tobytes(), \
                    f"{name} {mode}: {f} under nm = {k:g} * I ({CLASS_OF[k]}){' blended with the next k' if blended else ''}"
        equals_updated(ctx_a, ctx_b, moved, f"{name} {mode} blended {blended}")


@pytest.mark.parametrize("mode", [(2, 1, 0), (1, 1, 0)])
def test_weights_are_used_as_given(ctx_a, ctx_b, mode):
    from ptmi import native
    s, listed, corners, joints = weights_case()
    rest = tref.rest_of(s.tris)
    moved = ref.skinned(s.tris, rest, listed, corners, joints)
    assert not any(np.isnan(moved[f]).any() for f in tref.REST_FIELDS)
    want = ref.first_bad(s.tris, rest, listed, corners, joints, own=mode[0] == 2)
    upload(ctx_a, s, mode)
    upload(ctx_b, s, mode)
    ctx_a.set_skin(listed, corners, 4)
    rec = joint_records(joints)
    assert rec["nm"][MIRROR_JOINT].tobytes() == joints[MIRROR_JOINT][1].tobytes() and np.signbit(rec["nm"][MIRROR_JOINT]).sum() > 2
    if want == NONE:
        ctx_a.pose_skin(rec)
        assert skin_counts(ctx_a) == (1, 4, len(listed), 1, NONE)
        equals_updated(ctx_a, ctx_b, moved, f"weights as given {mode}")
    else:                                                              # the model refuses (the collapsed corner's edges): so must the device
        with pytest.raises(native.PtmiError) as e:
            ctx_a.pose_skin(rec)
        assert e.value.code == E_INVALID and ctx_a.skin_status().first_bad == want
        assert ctx_a.read_triangles().tobytes() == s.tris.tobytes()


@pytest.mark.parametrize("order", ["skin first", "groups first"])
def test_skin_and_groups_keep_separate_rest_poses(ctx_a, ctx_b, order):
    """neither call re-bases the other's rest pose, and a triangle that is listed and a member takes the last writer's record"""
    s, groups, listed, corners, g = overlap_case()
    rest = tref.rest_of(s.tris)                                        # of both: each was set on S
    p1, p2 = pose(4, 72), pose(4, 73)

    def posed(tris, p):
        return ref.skinned(tris, rest, listed, corners, p)

    def moved(tris, m):
        return tref.transformed(tris, rest, groups, [tref.op(g, m)])

    if order == "skin first":
        steps = [("pose", p1, posed), ("move", T1, moved), ("pose", p2, posed)]
    else:
        steps = [("move", T1, moved), ("pose", p1, posed), ("move", T2, moved)]
    overlap = np.intersect1d(np.flatnonzero(groups == g), listed)
    upload(ctx_a, s, (2, 1, 0))
    upload(ctx_b, s, (2, 1, 0))
    ctx_a.set_triangle_groups(groups)
    ctx_a.set_skin(listed, corners, 4)
    live = s.tris
    for i, (kind, arg, model) in enumerate(steps):
        before, live = live, model(live, arg)
        assert live[overlap].tobytes() != before[overlap].tobytes()    # the overlap takes this writer's record ...
        assert live[overlap].tobytes() == model(s.tris, arg)[overlap].tobytes()   # ... which is its edit of S, not of the other's record
        if kind == "pose":
            ctx_a.pose_skin(joint_records(arg))
        else:
            ctx_a.transform_groups(op_records([tref.op(g, arg)]))
        equals_updated(ctx_a, ctx_b, live, f"{order}, step {i}: {kind}")
    assert ctx_a.scene_update_status().updates == 3


def test_update_triangles_rebases_the_skin_and_the_groups(ctx_a, ctx_b):
    s, groups, listed, corners, g = overlap_case()
    lo, hi = 37, 251
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    rebased = s.tris.copy()
    rebased[lo:hi] = edit
    rest = tref.rest_of(rebased)                                       # the edited records inside the range, S outside: for both
    inside = np.arange(lo, hi)
    assert np.isin(inside, listed).any() and (groups[inside] == g).any() and (groups[:lo] == g).any()
    upload(ctx_a, s, (2, 1, 0))
    upload(ctx_b, s, (2, 1, 0))
    ctx_a.set_triangle_groups(groups)
    ctx_a.set_skin(listed, corners, 4)
    ctx_a.update_triangles(lo, edit)
    assert ctx_a.read_triangles().tobytes() == rebased.tobytes()
    p = pose(4, 74)
    ctx_a.pose_skin(joint_records(p))
    live = ref.skinned(rebased, rest, listed, corners, p)
    assert live.tobytes() != ref.skinned(rebased, tref.rest_of(s.tris), listed, corners, p).tobytes()
    equals_updated(ctx_a, ctx_b, live, "a pose after the edit")
    ctx_a.transform_groups(op_records([tref.op(g, T1)]))
    want = tref.transformed(live, rest, groups, [tref.op(g, T1)])
    assert want.tobytes() != tref.transformed(live, tref.rest_of(s.tris), groups, [tref.op(g, T1)]).tobytes()
    equals_updated(ctx_a, ctx_b, want, "a transform after the edit and the pose")


@pytest.mark.parametrize("which", ["a gap of the list", "the first listed", "the last listed", "everything"])
def test_skin_rebase_ranges(ctx_a, ctx_b, which):
    s = scene("soup80")
    listed, corners = skin_for(s, "half", 4, 3)
    lo, hi = rebase_ranges(listed, len(s.tris))[which]
    edit = uref.deformed(s.tris, "wobble")[lo:hi]
    assert edit.tobytes() != s.tris[lo:hi].tobytes()
    upload(ctx_a, s, (2, 1, 0))
    upload(ctx_b, s, (2, 1, 0))
    ctx_a.set_skin(listed, corners, 4)
    ctx_a.pose_skin(joint_records(pose(4, 75)))
    ctx_a.update_triangles(lo, edit)
    live = ctx_a.read_triangles()
    assert live[lo:hi].tobytes() == edit.tobytes()
    rebased = s.tris.copy()
    rebased[lo:hi] = edit                                              # listed triangles outside the range keep the old rest pose
    p2 = pose(4, 76)
    ctx_a.pose_skin(joint_records(p2))
    equals_updated(ctx_a, ctx_b, ref.skinned(live, tref.rest_of(rebased), listed, corners, p2), which)


def test_transform_ranges_off_the_octet(ctx_a, ctx_b):
    s = scene("grid80")
    n = len(s.tris)
    groups = aligned_groups(n)
    rest = tref.rest_of(s.tris)
    calls = [[tref.op(1, T1)], [tref.op(2, T2)], [tref.op(2, T1), tref.op(1, tref.affine(scale=(3, 0.5, 1)))]]
    assert tref.launch_ranges(groups, calls[0]) == [(ALIGN_LO - 3, ALIGN_HI + 1)] and tref.launch_ranges(groups, calls[1]) == [((n - 1) & ~7, n)]
    straddled = np.r_[ALIGN_LO & ~7:ALIGN_LO, ALIGN_HI + 1:(ALIGN_HI + 8) & ~7]
    assert len(straddled) == 3 + 3
    for mode in MODES:
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_triangle_groups(groups)
        live = s.tris
        for i, ops in enumerate(calls):
            what = f"grid80 {mode} call {i}"
            live = tref.transformed(live, rest, groups, ops)
            ctx_a.transform_groups(op_records(ops))
            moved = sum(int((groups == g).sum()) for g, _, _ in ops)
            assert group_counts(ctx_a) == (1, 3, i + 1, moved, NONE), what
            assert ctx_a.read_triangles()[straddled].tobytes() == s.tris[straddled].tobytes(), f"{what}: the rest of the straddled octets"
            equals_updated(ctx_a, ctx_b, live, what)
