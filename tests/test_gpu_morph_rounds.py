"""ptmi_pose_morph (csrc/scene_morph.hip k_morph) past one round of the grid, where the small scenes of tests/test_gpu_morph.py do not
reach: the launch has 8 blocks per compute unit of 32 list entries each, and entries beyond that are walked by the blocks' second
round. The scene is tests/test_gpu_edit_edges.py's big_scene: more than 1.2 rounds of triangles, with a count beyond one round that is
no multiple of 8 or of 32, so that the last round ends in a partial wave and a partial octet.

A: a pose of the whole list equals update_triangles(0, the model's records), on own and on reference leaves.
B: a pose refused by one entry, placed at R + 5 (the second round), at R - 3 (the last block of the first), at the last entry (the
   partial octet), and by all three at once: first_bad is the model's and nothing has changed.

Every case fails without the feature: the binding has no set_morph."""
import numpy as np
import pytest

import morph_ref as ref
import transform_ref as tref
from ptmi import layout
from test_gpu_edit_edges import MODES, big_scene, device_cus, equals_updated, round_of, snapshot, unchanged, upload
from test_gpu_scene_update import ctx_a, ctx_b  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

E_INVALID = -1
NONE = 0xFFFFFFFF
N_TARGETS = 6


def test_a_pose_of_more_than_one_round(ctx_a, ctx_b):
    cus = device_cus()
    s = big_scene(cus)
    count, R = len(s.tris), round_of(cus)
    assert count > R
    listed = np.arange(count, dtype=np.uint32)
    rng = np.random.default_rng(101)
    row_start, deltas = ref.table(rng, count, N_TARGETS, (1, 3, 0, 2))
    w = ref.weights_for(rng, N_TARGETS, 4)
    moved = ref.morphed(s.tris, tref.rest_of(s.tris), listed, row_start, deltas, w)
    assert moved[-1:].tobytes() != s.tris[-1:].tobytes() or moved[-2:].tobytes() != s.tris[-2:].tobytes()
    assert moved[R:].tobytes() != s.tris[R:].tobytes()
    for mode in MODES:
        what = f"{s.name} {mode}"
        upload(ctx_a, s, mode)
        upload(ctx_b, s, mode)
        ctx_a.set_morph(listed, row_start, deltas, N_TARGETS)
        ctx_a.pose_morph(w)
        st = ctx_a.morph_status()
        assert (st.n_morphed, st.n_records, st.poses, st.first_bad) == (count, len(deltas), 1, NONE), what
        equals_updated(ctx_a, ctx_b, moved, what)


def test_a_pose_refused_in_another_round_block_or_octet(ctx_a, ctx_b):
    """three records more, each on a target of its own (N_TARGETS + k) and in the row of its own entry, with a delta of 3e38 that
    weight 2 takes out of float32: a pose that raises target N_TARGETS + k is refused by that entry alone"""
    from ptmi import native
    cus = device_cus()
    s = big_scene(cus)
    count, R = len(s.tris), round_of(cus)
    assert count > R + 5
    places = [R + 5, R - 3, count - 1]
    listed = np.arange(count, dtype=np.uint32)
    rng = np.random.default_rng(102)
    row_start, deltas = ref.table(rng, count, N_TARGETS, (1, 3, 0, 2))
    rows = [deltas[row_start[e]:row_start[e + 1]] for e in range(count)]
    for k, e in enumerate(places):
        extra = np.zeros(1, layout.MORPH_DELTA)
        extra["target"], extra["dv1"][0, 2] = N_TARGETS + k, 3e38
        rows[e] = np.concatenate([rows[e], extra])
    deltas = np.concatenate(rows)
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    nt = N_TARGETS + 3
    rest = tref.rest_of(s.tris)
    good = ref.weights_for(rng, nt, None)
    good[N_TARGETS:] = 0.0
    upload(ctx_a, s, MODES[0])
    upload(ctx_b, s, MODES[0])
    ctx_a.set_morph(listed, row_start, deltas, nt)
    ctx_a.pose_morph(good)
    live = ref.morphed(s.tris, rest, listed, row_start, deltas, good)
    snap, ms = snapshot(ctx_a), ctx_a.morph_status()
    assert snap[0].tobytes() == live.tobytes()
    for which in ([0], [1], [2], [0, 1, 2]):
        bad = good.copy()
        bad[[N_TARGETS + k for k in which]] = 2.0
        assert ref.offenders(live, rest, listed, row_start, deltas, bad, own=True).tolist() == sorted(places[k] for k in which)
        want = min(places[k] for k in which)
        with pytest.raises(native.PtmiError) as e:
            ctx_a.pose_morph(bad)
        assert e.value.code == E_INVALID, which
        now = ctx_a.morph_status()
        assert now.first_bad == want, f"{which}: first_bad {now.first_bad}, the model's {want}"
        assert (now.poses, now.pose_ms) == (ms.poses, ms.pose_ms), which
        unchanged(ctx_a, snap, str(which))
    w2 = ref.weights_for(rng, nt, 5)                                      # the next valid call gives the usual bits
    w2[N_TARGETS:] = 0.0
    ctx_a.pose_morph(w2)
    assert ctx_a.morph_status().first_bad == NONE and ctx_a.morph_status().poses == 2
    equals_updated(ctx_a, ctx_b, ref.morphed(live, rest, listed, row_start, deltas, w2), "after the refusals")
