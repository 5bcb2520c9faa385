"""The model of ptmi_pose_morph (include/ptmi.h): the arithmetic restated in float32 numpy, operation by operation. Per corner of a
listed triangle the records of its row are taken in order; a record whose weight is zero (either sign) is SKIPPED, every other one adds
w * d to the running vertex and normal, the product rounded first and the sum second (numpy fuses nothing). A triangle of which no
record was applied keeps its rest bits, normals included; the normals of every other one go through the tail of
ptmi_transform_groups' normal formula (q / sqrt(l2) where l2 > 0, else q).

The rows differ in length, so the model walks them by position: step j handles record j of every row that has one, for all rows at
once, which keeps each row's own order."""
import numpy as np

import transform_ref as tref
from ptmi import layout

NONE = tref.NONE
VERTS, NORMALS = ("v0", "v1", "v2"), ("n0", "n1", "n2")
DV, DN = ("dv0", "dv1", "dv2"), ("dn0", "dn1", "dn2")
MAX_TARGETS = 8192


def unit_tail(q):
    """q / sqrt(l2) where l2 = (q.x q.x + q.y q.y) + q.z q.z > 0, else q: the tail of transform_ref.normal, rows of float32"""
    q = np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        l2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        unit = l2 > 0
        length = np.sqrt(l2[unit])
        out = q.copy()
        for k in range(3):
            out[unit, k] = q[unit, k] / length
    return out


def applied_counts(row_start, deltas, weights):
    """per list entry, how many records of its row have a non-zero weight"""
    row_start = np.asarray(row_start, np.int64)
    w = np.asarray(weights, np.float32)
    live = (w[np.asarray(deltas["target"], np.int64)] != 0).astype(np.int64) if len(deltas) else np.zeros(0, np.int64)
    total = np.concatenate([[0], np.cumsum(live)])
    return total[row_start[1:]] - total[row_start[:-1]]


def summed(rest, listed, row_start, deltas, weights):
    """(the six running vectors of every list entry after its row, before the normal tail: a dict of (len(listed), 3) float32 arrays;
    which entries had a record applied)"""
    listed = np.asarray(listed, np.int64)
    row_start = np.asarray(row_start, np.int64)
    deltas = np.asarray(deltas, layout.MORPH_DELTA).reshape(-1)
    w_all = np.asarray(weights, np.float32)
    lengths = row_start[1:] - row_start[:-1]
    acc = {f: rest[f][listed].astype(np.float32).copy() for f in VERTS + NORMALS}
    touched = np.zeros(len(listed), bool)
    with np.errstate(all="ignore"):
        for j in range(int(lengths.max()) if len(lengths) else 0):
            rows = np.flatnonzero(lengths > j)
            rec = row_start[rows] + j
            w = w_all[deltas["target"][rec].astype(np.int64)]
            use = w != 0                                             # -0.0 != 0 is False: either sign is skipped
            rows, rec, w = rows[use], rec[use], w[use]
            touched[rows] = True
            for f, g in zip(VERTS + NORMALS, DV + DN):
                acc[f][rows] = acc[f][rows] + w[:, None] * deltas[g][rec]
    return acc, touched


def morphed(tris, rest, listed, row_start, deltas, weights):
    """the records after pose_morph(weights) where every listed triangle goes to its live record: the listed triangles become their
    rest pose plus the weighted records of their rows, everything else keeps its bytes. rest: transform_ref.rest_of of the records
    the morph was set on (indexed by triangle); listed: ascending triangle indices; row_start: len(listed) + 1 bounds; deltas:
    layout.MORPH_DELTA records."""
    out = tris.copy()
    listed = np.asarray(listed, np.int64)
    acc, touched = summed(rest, listed, row_start, deltas, weights)
    for f in VERTS:
        out[f][listed] = acc[f]
    for f in NORMALS:
        n = acc[f]
        n[touched] = unit_tail(n[touched])                           # an untouched triangle is not renormalised
        out[f][listed] = n
    return out


def offenders(tris, rest, listed, row_start, deltas, weights, own):
    """every list ENTRY (position in `listed`) the check pass refuses (ptmi_update_triangles' vertex checks on the morphed vertices),
    ascending; listed[offenders] are the triangles"""
    listed = np.asarray(listed, np.int64)
    t = morphed(tris, rest, listed, row_start, deltas, weights)[listed]
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(t["v0"]).all(axis=1) & np.isfinite(t["v1"]).all(axis=1) & np.isfinite(t["v2"]).all(axis=1))
        if own:
            a = t["v0"]
            for f in ("v1", "v2"):
                bad |= ~np.isfinite(a + (t[f] - a)).all(axis=1)
    return np.flatnonzero(bad)


def first_bad(tris, rest, listed, row_start, deltas, weights, own):
    """the smallest listed triangle among offenders() (the list ascends: the first entry's), or NONE"""
    bad = offenders(tris, rest, listed, row_start, deltas, weights, own)
    return int(np.asarray(listed, np.int64)[bad[0]]) if len(bad) else NONE


def table(rng, n_listed, n_targets, lengths, cover=False, dv=0.03, dn=0.3):
    """a seeded sparse table (row_start, deltas): row e has lengths[e % len(lengths)] records (0: an empty row) on distinct targets,
    ascending. cover: row e takes the targets (e * L + k) % n_targets, k < L, so that every target is referenced once the rows hold
    n_targets records between them. Position deltas are uniform in +-dv, normal deltas in +-dn."""
    lengths = np.asarray([lengths[e % len(lengths)] for e in range(n_listed)], np.int64)
    assert lengths.max(initial=0) <= n_targets
    row_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    d = np.zeros(int(row_start[-1]), layout.MORPH_DELTA)
    order = None if cover else np.argsort(rng.random((n_listed, n_targets)), axis=1)     # a seeded permutation of the targets per row
    for n in np.unique(lengths[lengths > 0]):
        rows = np.flatnonzero(lengths == n)
        first = row_start[rows].astype(np.int64)
        if cover:
            t = (first[:, None] + np.arange(n)) % n_targets
        else:
            t = order[rows, :n]
        d["target"][first[:, None] + np.arange(n)] = np.sort(t, axis=1)
    for g in DV:
        d[g] = rng.uniform(-dv, dv, (len(d), 3))
    for g in DN:
        d[g] = rng.uniform(-dn, dn, (len(d), 3))
    return row_start, d


def weights_for(rng, n_targets, active):
    """n_targets weights of which `active` (None: all) are non-zero, in (0.1, 1) with either sign; the zeros alternate between +0 and
    -0"""
    w = np.zeros(n_targets, np.float32)
    w[1::2] = -0.0
    pick = np.arange(n_targets) if active is None else rng.choice(n_targets, active, replace=False)
    w[pick] = rng.uniform(0.1, 1.0, len(pick)) * rng.choice([-1.0, 1.0], len(pick))
    return w
