"""The model of ptmi_transform_groups (include/ptmi.h): the arithmetic restated in float32 numpy, operation by operation, and the
cofactor matrix of ptmi_normal_matrix in float64. Every product and sum below is one IEEE operation on float32 (float64 for the
cofactors) arrays, in the order the header writes them; numpy fuses nothing."""
import numpy as np

REST_FIELDS = ("v0", "v1", "v2", "n0", "n1", "n2")
NONE = 0xFFFFFFFF
F32_MAX = np.float32(3.4028234663852886e38)


def normal_matrix(m):
    """the cofactors of the upper 3 x 3 of the 3 x 4 row-major m, each a*b - c*d in float64 in that order, rounded to float32"""
    a = np.asarray(m, np.float32).reshape(3, 4)[:, :3].astype(np.float64)
    c = np.empty(9, np.float64)
    c[0] = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
    c[1] = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
    c[2] = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    c[3] = a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]
    c[4] = a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]
    c[5] = a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]
    c[6] = a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]
    c[7] = a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]
    c[8] = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    with np.errstate(over="ignore"):
        return c.astype(np.float32)


def rest_of(tris):
    """the rest pose a table set now would snapshot: the six vector fields of every record"""
    return {f: tris[f].copy() for f in REST_FIELDS}


def point(m, p):
    """p'_k = ((m[4k] p.x + m[4k+1] p.y) + m[4k+2] p.z) + m[4k+3] for the points p (n, 3)"""
    m = np.asarray(m, np.float32).reshape(12)
    p = np.asarray(p, np.float32)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = ((m[4 * k] * p[:, 0] + m[4 * k + 1] * p[:, 1]) + m[4 * k + 2] * p[:, 2]) + m[4 * k + 3]
    return out


def normal(nm, n):
    """q = nm n, then q / sqrt(q.q) where q.q > 0, else q, for the normals n (n, 3)"""
    nm = np.asarray(nm, np.float32).reshape(9)
    n = np.asarray(n, np.float32)
    q = np.empty_like(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            q[:, k] = (nm[3 * k] * n[:, 0] + nm[3 * k + 1] * n[:, 1]) + nm[3 * k + 2] * n[:, 2]
        l2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        unit = l2 > 0
        length = np.sqrt(l2[unit])
        out = q.copy()
        for k in range(3):
            out[unit, k] = q[unit, k] / length
    return out


def normal_classes(q):
    """which magnitude class of the normal formula each row of q = nm n (n, 3) falls to: a dict of boolean masks over the rows.
    q_denormal: a component of q is a denormal; l2_zero: l2 underflows to 0 while q != 0 (q is stored unnormalised); l2_denormal:
    l2 > 0 is a denormal; l2_large: l2 is finite and within a factor 256 of the largest float; l2_inf: l2 overflows with q finite
    (the result is a signed zero)"""
    q = np.asarray(q, np.float32)
    tiny, big = np.finfo(np.float32).tiny, F32_MAX / np.float32(256.0)
    with np.errstate(all="ignore"):
        l2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    return {"q_denormal": ((q != 0) & (np.abs(q) < tiny)).any(axis=1), "l2_zero": (l2 == 0) & (q != 0).any(axis=1),
            "l2_denormal": (l2 > 0) & (l2 < tiny), "l2_large": np.isfinite(l2) & (l2 > big),
            "l2_inf": np.isinf(l2) & np.isfinite(q).all(axis=1)}


def transformed(tris, rest, groups, ops):
    """the live records after transform_groups(ops): members of a named group become T(rest), everything else keeps its bytes.
    ops: (group, m, nm) tuples, m 12 and nm 9 floats."""
    out = tris.copy()
    groups = np.asarray(groups, np.uint32)
    for g, m, nm in ops:
        sel = np.flatnonzero(groups == g)
        if not len(sel):
            continue
        for f in ("v0", "v1", "v2"):
            out[f][sel] = point(m, rest[f][sel])
        for f in ("n0", "n1", "n2"):
            out[f][sel] = normal(nm, rest[f][sel])
    return out


def offenders(tris, rest, groups, ops, own):
    """every member triangle the check pass refuses (ptmi_update_triangles' vertex checks on the transformed vertices), ascending"""
    t = transformed(tris, rest, groups, ops)
    named = np.isin(np.asarray(groups, np.uint32), [g for g, _, _ in ops])
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(t["v0"]).all(axis=1) & np.isfinite(t["v1"]).all(axis=1) & np.isfinite(t["v2"]).all(axis=1))
        if own:
            a = t["v0"]
            for f in ("v1", "v2"):
                bad |= ~np.isfinite(a + (t[f] - a)).all(axis=1)
    bad &= named
    return np.flatnonzero(bad)


def first_bad(tris, rest, groups, ops, own):
    """the smallest of offenders(), or NONE"""
    bad = offenders(tris, rest, groups, ops, own)
    return int(bad[0]) if len(bad) else NONE


def launch_ranges(groups, ops, chunk=512):
    """the triangle range [first, end) each launch of a pass walks, as csrc/scene_transform.hip run_pass sets it: one launch per
    chunk of `chunk` ops in call order, from the lowest member of the chunk's groups rounded down to a multiple of 8 to one past the
    highest; None for a chunk whose groups have no member. A test uses it to say which block and round a triangle falls to."""
    groups = np.asarray(groups, np.uint32)
    out = []
    for f in range(0, len(ops), chunk):
        member = np.flatnonzero(np.isin(groups, [g for g, _, _ in ops[f:f + chunk]]))
        out.append((int(member[0]) & ~7, int(member[-1]) + 1) if len(member) else None)
    return out


def affine(rot=None, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """a 3 x 4 row-major affine as 12 float32: rot (3 x 3, default identity) times diag(scale), then the shift"""
    a = (np.eye(3) if rot is None else np.asarray(rot, np.float64)) @ np.diag(np.asarray(scale, np.float64))
    return np.concatenate([a, np.asarray(shift, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


def rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def op(group, m, nm=None):
    m = np.asarray(m, np.float32).reshape(12)
    return (int(group), m, normal_matrix(m) if nm is None else np.asarray(nm, np.float32).reshape(9))
