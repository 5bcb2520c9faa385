"""First-hit planes (include/ptmi.h ptmi_set_aovs) without a GPU: the header and the library agree on the new entry points,
every one of them refuses a NULL context, and the plain reference of tests/aov_ref.py holds on the Cornell box."""
import ctypes
import os
import re

import numpy as np
import pytest

import aov_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOV_FUNCS = ["ptmi_set_aovs", "ptmi_get_aovs", "ptmi_read_aov", "ptmi_aov_device_ptr"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)


def test_header_declares_the_aov_entry_points():
    h = _header()
    for f in AOV_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, h), f
    vals = dict(re.findall(r"\b(PTMI_AOV_[A-Z]+)\s*=\s*(\d+)u?", h))
    assert vals == {"PTMI_AOV_ALBEDO": "1", "PTMI_AOV_NORMAL": "2", "PTMI_AOV_ID": "4"}
    assert re.search(r"#define PTMI_ABI_VERSION 4\b", h)


def test_library_exports_them_and_the_binding_lists_them():
    from ptmi import native
    L = native.load()
    for f in AOV_FUNCS:
        assert hasattr(L, f), f
        assert f in native.EXPORTS
    assert (native.AOV_ALBEDO, native.AOV_NORMAL, native.AOV_ID) == (1, 2, 4)


def test_null_context_is_refused():
    from ptmi import native
    L = native.load()
    m = ctypes.c_uint32(123)
    buf = np.zeros(64, np.uint8)
    assert L.ptmi_set_aovs(None, 0) == -1
    assert L.ptmi_set_aovs(None, 7) == -1
    assert L.ptmi_get_aovs(None, ctypes.byref(m)) == -1 and m.value == 123
    assert L.ptmi_read_aov(None, 1, native._p(buf), buf.nbytes) == -1
    assert L.ptmi_read_aov(None, 4, None, 0) == -1
    for which in (0, 1, 2, 4, 3, 8):
        assert L.ptmi_aov_device_ptr(None, which) is None


def test_binding_rejects_unknown_plane_names():
    from ptmi import native
    with pytest.raises(ValueError):
        native._aov("depth")
    assert set(native.AOVS) == {"albedo", "normal", "id"}


def test_reference_on_cornell(oracle, scene_factory):
    from ptmi import layout
    sc = scene_factory("cornell")
    W, H = 40, 30
    cam = layout.make_camera(W, H)
    s = aov_ref.samples(oracle, sc, cam, 0)
    hit = s["hit"]
    assert 0 < hit.sum() <= W * H
    # misses: zeros and 0xFFFFFFFF
    assert (s["tri"][~hit] == aov_ref.MISS).all() and (s["mat"][~hit] == aov_ref.MISS).all()
    assert (s["t"][~hit] == 0).all() and (s["albedo"][~hit] == 0).all()
    assert (s["t"][hit] > 0).all()
    # no textures in the Cornell box: albedo is the base colour, bit for bit
    base = sc.mats["base_color"][s["mat"][hit]].astype(np.float32)
    assert np.array_equal(s["albedo"][hit].view(np.uint32), base.view(np.uint32))
    assert s["albedo_exact"].all() and s["normal_exact"].all() and not s["normal_mapped"].any()
    # flat triangles (the walls, the light, the boxes): the shading normal is the quad's normal, of unit length
    T = sc.tris[s["tri"][hit]]
    flat = (T["n0"] == T["n1"]).all(axis=1) & (T["n0"] == T["n2"]).all(axis=1)
    assert flat.sum() > 0.5 * hit.sum()
    n = s["normal"][hit][flat]
    assert np.abs(n - T["n0"][flat]).max() < 1e-7
    assert np.abs(np.linalg.norm(s["normal"][hit], axis=1) - 1).max() < 1e-12
    # one frame folds to itself: coverage exactly 0 or 1, depth and normal as sampled
    a, nrm, ids, exact = aov_ref.fold([s], [0])
    assert set(np.unique(a[:, 3]).tolist()) <= {0.0, 1.0}
    assert np.array_equal(a[:, 3] == 1, hit)
    assert np.array_equal(nrm[:, 3].view(np.uint32), s["t"].view(np.uint32))
    assert np.array_equal(ids[:, 0], s["tri"]) and exact.all()
    # two frames: the mean, and the ids of the last one
    s1 = aov_ref.samples(oracle, sc, cam, 1)
    a2, _, ids2, _ = aov_ref.fold([s, s1], [0, 1])
    want = (s["hit"].astype(np.float64) + s1["hit"]) / 2
    assert np.abs(a2[:, 3] - want).max() < 1e-7
    assert np.array_equal(ids2[:, 0], s1["tri"])
