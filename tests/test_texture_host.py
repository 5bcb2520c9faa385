"""The texture lookup at its edges on the CPU: the plain float64 reference of tests/texture_ref.py against the oracle's
one-bounce render of scenes.texture_edges, and the scene's own promises (distinct texels, the specials where it says)."""
import numpy as np
import pytest

import texture_ref
from ptmi import layout, scenes

SHAPES = [(67, 29), (3, 517), (65537, 3)]
W, H = 64, 48


def probe_hits(oracle, sc, cam):
    ys, xs = np.mgrid[0:H, 0:W]
    o, d, _ = oracle.raygen(cam, xs.ravel(), ys.ravel(), np.zeros(W * H, np.uint32))
    t, tri, u, v, _ = oracle.intersect(sc, o, d)
    return t, tri, u, v


@pytest.mark.parametrize("fmt", ["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_predicts_the_oracle_probe_wall(oracle, shape, fmt):
    sc = scenes.texture_edges(shape, fmt)
    cam = layout.make_camera(W, H)
    img, _ = oracle.render(sc, cam, 1, max_bounces=1, do_mis=0)
    t, tri, u, v = probe_hits(oracle, sc, cam)
    n_probe, n_exact = texture_ref.check(sc, img[..., :3].reshape(-1, 3), t, tri, u, v)
    assert n_probe > 0.4 * W * H


@pytest.mark.parametrize("fmt", ["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_texture_edges_atlas(shape, fmt):
    Wa, Ha = shape
    sc = scenes.texture_edges(shape, fmt)
    a = sc.atlas
    assert a.shape == (Ha, Wa, 4) and a.dtype == (np.float16 if fmt == "f16" else np.float32) and a.flags.c_contiguous
    assert len(np.unique(a.view(np.uint8).reshape(Ha * Wa, -1), axis=0)) == Ha * Wa, "texels are not all distinct"
    r = scenes.texture_edge_rects(Wa, Ha)
    x, y, w, h = r["specials"]
    block = a[y:y + h, x:x + w, 0].astype(np.float64).ravel()
    with np.errstate(over="ignore"):
        bits16 = a[y:y + h, x:x + w, 0].astype(np.float16).view(np.uint16).ravel()
    for pattern in (0x0000, 0x8000, 0x0001, 0x03FF, 0x7BFF, 0x7C00, 0xFC00, 0xFBFF):
        assert pattern in bits16, hex(pattern)
    assert np.isnan(block).any() and (block < 0).any()
    if fmt == "f32":
        for val in (np.float32(1 + 2.0 ** -20), np.float32(1e-40), np.float32(3e38)):
            assert (a[y:y + h, x:x + w, 0] == val).any()
        with np.errstate(over="ignore"):
            assert not np.array_equal(a.astype(np.float16).astype(np.float32), a)
    nx, ny = r["normal"][:2]
    flat = np.array([0.5, 0.5, 1.0], np.float32)
    nb = a[ny:ny + 2, nx:nx + 2, :3].astype(np.float32).reshape(-1, 3)
    assert (nb == flat).all(axis=1).sum() == 1
    for k in range(3):                                    # one-f16-ulp neighbours of the flat value
        assert any(((q != flat).sum() == 1) and abs(float(q[k]) - float(flat[k])) <= 2.0 ** -11 and q[k] != flat[k] for q in nb)
    m = sc.mats
    for field in ("albedo_map", "normal_map", "pbr_map", "emissive_map"):
        assert (m[field]["w"] | m[field]["h"]).any(), field
    rects = {tuple(int(q) for q in e) for e in m["emissive_map"]}
    assert {(Wa, 0, 2, 2), (0xFFFFFFFF, 0, 4, 4), (Wa - 1, Ha - 1, 1, 1), (0, 0, 0x80000000, 1)} <= rects
    assert any(e[2] == 0 and e[3] > 0 for e in rects) and any(e[2] > 0 and e[3] == 0 for e in rects)
    uv = np.concatenate([sc.tris["uv0"], sc.tris["uv1"], sc.tris["uv2"]])
    assert np.isnan(uv).any() and np.isinf(uv).any() and (uv >= 1e7).any() and (uv == np.float32(1 - 2.0 ** -24)).any()
    assert (np.signbit(uv) & (uv == 0)).any()
    same_uv = (sc.tris["uv0"] == sc.tris["uv1"]).all(1) & (sc.tris["uv1"] == sc.tris["uv2"]).all(1)
    assert same_uv.any()
    assert (sc.lights["light_type"] == layout.LIGHT_POINT).any() and (sc.lights["light_type"] == layout.LIGHT_EMISSIVE).any()
