"""The model of ptmi_pose_skin (include/ptmi.h): the arithmetic restated in float32 numpy, operation by operation. The blend of the
joint records is one product or sum per line of the header's formula, over all corners at once; the blended matrices then go through
the vertex and normal formulas of ptmi_transform_groups, row by row what transform_ref.point / transform_ref.normal compute for one
matrix (point_rows / normal_rows below are those two with a matrix per row; tests/test_skin_host.py holds them to the originals
byte for byte). numpy fuses nothing."""
import numpy as np

import transform_ref as tref
from ptmi import layout

NONE = tref.NONE
VERTS, NORMALS = ("v0", "v1", "v2"), ("n0", "n1", "n2")


def joint_arrays(joints):
    """(M (n_joints, 12), NM (n_joints, 9)) float32 from (m, nm) pairs (nm None: the cofactor matrix) or from 96-byte records"""
    if isinstance(joints, np.ndarray) and joints.dtype.names:
        return np.ascontiguousarray(joints["m"], np.float32), np.ascontiguousarray(joints["nm"], np.float32)
    M = np.array([np.asarray(m, np.float32).reshape(12) for m, _ in joints], np.float32).reshape(-1, 12)
    NM = np.array([tref.normal_matrix(m) if nm is None else np.asarray(nm, np.float32).reshape(9) for m, nm in joints],
                  np.float32).reshape(-1, 9)
    return M, NM


def joint(m, nm=None):
    """an (m, nm) pair, nm derived where None, with every negative zero replaced by +0 (x + 0 does that and changes nothing else):
    the cofactors of a mirror hold some, and a one-hot blend would not keep their sign"""
    m = np.asarray(m, np.float32).reshape(12)
    nm = tref.normal_matrix(m) if nm is None else np.asarray(nm, np.float32).reshape(9)
    return m + np.float32(0.0), nm + np.float32(0.0)


def blend(J, corner):
    """((w0 J[j0] + w1 J[j1]) + w2 J[j2]) + w3 J[j3] per entry, for the corner records `corner` (n,): every slot evaluated"""
    j, w = corner["joint"], corner["weight"].astype(np.float32)
    with np.errstate(all="ignore"):
        t = [w[:, k, None] * J[j[:, k]] for k in range(4)]
        return ((t[0] + t[1]) + t[2]) + t[3]


def point_rows(M, p):
    """transform_ref.point with a matrix per row: M (n, 12), p (n, 3)"""
    p = np.asarray(p, np.float32)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = ((M[:, 4 * k] * p[:, 0] + M[:, 4 * k + 1] * p[:, 1]) + M[:, 4 * k + 2] * p[:, 2]) + M[:, 4 * k + 3]
    return out


def q_rows(NM, n):
    """q = NM n alone, a matrix per row, as normal_rows computes it before it normalises (for transform_ref.normal_classes)"""
    n = np.asarray(n, np.float32)
    q = np.empty_like(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            q[:, k] = (NM[:, 3 * k] * n[:, 0] + NM[:, 3 * k + 1] * n[:, 1]) + NM[:, 3 * k + 2] * n[:, 2]
    return q


def normal_rows(NM, n):
    """transform_ref.normal with a matrix per row: NM (n, 9), n (n, 3)"""
    n = np.asarray(n, np.float32)
    q = np.empty_like(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            q[:, k] = (NM[:, 3 * k] * n[:, 0] + NM[:, 3 * k + 1] * n[:, 1]) + NM[:, 3 * k + 2] * n[:, 2]
        l2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        unit = l2 > 0
        length = np.sqrt(l2[unit])
        out = q.copy()
        for k in range(3):
            out[unit, k] = q[unit, k] / length
    return out


def skinned(tris, rest, listed, corners, joints):
    """the live records after pose_skin(joints): the listed triangles become the blend applied to their rest pose, everything else
    keeps its bytes. rest: transform_ref.rest_of of the records the skin was set on (indexed by triangle); listed: ascending triangle
    indices; corners: layout.SKIN_CORNER records, three per listed triangle; joints: see joint_arrays."""
    out = tris.copy()
    listed = np.asarray(listed, np.int64)
    corners = np.asarray(corners, layout.SKIN_CORNER).reshape(len(listed), 3)
    M, NM = joint_arrays(joints)
    for k in range(3):
        out[VERTS[k]][listed] = point_rows(blend(M, corners[:, k]), rest[VERTS[k]][listed])
        out[NORMALS[k]][listed] = normal_rows(blend(NM, corners[:, k]), rest[NORMALS[k]][listed])
    return out


def offenders(tris, rest, listed, corners, joints, own):
    """every list ENTRY (position in `listed`) the check pass refuses (ptmi_update_triangles' vertex checks on the skinned vertices),
    ascending; listed[offenders] are the triangles"""
    listed = np.asarray(listed, np.int64)
    t = skinned(tris, rest, listed, corners, joints)[listed]
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(t["v0"]).all(axis=1) & np.isfinite(t["v1"]).all(axis=1) & np.isfinite(t["v2"]).all(axis=1))
        if own:
            a = t["v0"]
            for f in ("v1", "v2"):
                bad |= ~np.isfinite(a + (t[f] - a)).all(axis=1)
    return np.flatnonzero(bad)


def first_bad(tris, rest, listed, corners, joints, own):
    """the smallest listed triangle among offenders() (the list ascends: the first entry's), or NONE"""
    bad = offenders(tris, rest, listed, corners, joints, own)
    return int(np.asarray(listed, np.int64)[bad[0]]) if len(bad) else NONE


def joint_raw(m, nm=None):
    """joint() without the + 0: an (m, nm) pair as given or derived, negative zeros kept (a mirror's cofactors hold some)"""
    m = np.asarray(m, np.float32).reshape(12)
    return m.copy(), tref.normal_matrix(m) if nm is None else np.asarray(nm, np.float32).reshape(9).copy()


def one_hot(joint_of_triangle):
    """corner records that give every corner of listed triangle i the joint joint_of_triangle[i] alone: weights (1, 0, 0, 0)"""
    j = np.asarray(joint_of_triangle, np.uint32)
    c = np.zeros((len(j), 3), layout.SKIN_CORNER)
    c["joint"][:, :, 0] = j[:, None]
    c["weight"][:, :, 0] = 1.0
    return c.reshape(-1)


def random_corners(rng, n_listed, n_joints, influences=4, cover=False):
    """seeded corner records: `influences` non-zero weights per corner (the other slots weight 0 on joint 0), summing to 1 in double
    before the rounding to float32. cover: corner i's first slot names joint i % n_joints, so that every joint is referenced when there
    are at least n_joints corners."""
    c = np.zeros(3 * n_listed, layout.SKIN_CORNER)
    j = rng.integers(0, n_joints, (3 * n_listed, 4))
    if cover:
        j[:, 0] = np.arange(3 * n_listed) % n_joints
    w = rng.uniform(0.1, 1.0, (3 * n_listed, 4))
    w[:, influences:] = 0.0
    j[:, influences:] = 0
    w /= w.sum(axis=1, keepdims=True)
    c["joint"], c["weight"] = j, w
    return c
