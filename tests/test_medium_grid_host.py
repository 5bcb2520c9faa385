"""The medium's density grid without a GPU (include/ptmi.h ptmi_upload_medium_density): the numpy model of
tests/medium_grid_ref.py checked against what it must satisfy by itself, the two precisions of the model against each other on the
probes' inputs (the proof that the GPU test's set-aside cap can be met by the reference alone), the layout of the new structs by a C
compiler, the new symbols, and the argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import medium_grid_ref as R
import medium_ref
from ptmi import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ptmi_upload_medium_density", "ptmi_medium_grid_status", "ptmi_multi_upload_medium_density", "ptmi_debug_medium_density",
       "ptmi_debug_medium_track", "ptmi_debug_medium_grid_check"]


def test_rng_of_the_model_on_hand_values():
    """the PCG step of csrc/pt_math.h worked by hand for state 0, and the float's range"""
    s1 = 2891336453
    r = (((s1 >> ((s1 >> 28) + 4)) ^ s1) * 277803737) & 0xFFFFFFFF
    w = (r >> 22) ^ r
    st, f = R.rng_next(np.uint32([0]))
    assert int(st[0]) == s1 and f.dtype == np.float32 and float(f[0]) == float(np.float32(w) * np.float32(2.0 ** -32))
    st = np.arange(1 << 16, dtype=np.uint32) * np.uint32(65521)
    for _ in range(4):
        st, f = R.rng_next(st)
        assert f.min() >= 0.0 and f.max() <= 1.0 and abs(float(f.mean()) - 0.5) < 0.01


def test_lookup_on_hand_cases():
    m = medium_ref.Medium(1.0, 1.0, 0.0, (0, 0, 0), (3, 5, 2))
    g = np.arange(30, dtype=np.float32).reshape(2, 5, 3) / 32                  # entry (k * 5 + j) * 3 + i holds its own index / 32
    p = np.float64([(0.5, 0.5, 0.5), (2.5, 0.5, 0.5), (0.5, 4.5, 0.5), (0.5, 0.5, 1.5), (2.99, 4.99, 1.99), (-1, -1, -1), (9, 9, 9),
                    (np.nan, 4.5, 1.5)])
    want = np.float64([0, 2, 12, 15, 29, 0, 29, 27]) / 32
    for dt in (np.float64, np.float32):
        assert np.array_equal(R.lookup(m, g, 0, p.astype(dt), dt), want.astype(dt))
        lin = R.lookup(m, g, 1, p.astype(dt), dt)
        assert np.array_equal(lin[:4], want[:4].astype(dt))                    # a cell centre is its own value
        assert lin[5] == 0 and lin[6] == dt(29 / 32) and np.isnan(lin[7])      # outside: the clamped taps
    mid = R.lookup(m, g, 1, np.float64([(1.0, 0.5, 0.5), (0.5, 1.0, 0.5), (0.5, 0.5, 1.0), (1.0, 1.0, 1.0)]), np.float64)
    assert np.allclose(mid, np.float64([0.5, 1.5, 7.5, 9.5]) / 32, rtol=0, atol=1e-15)     # half way along x, y, z, and all three
    # a constant grid is that constant under both filters, wherever the point is
    c = np.full((2, 5, 3), 0.25, np.float32)
    q = R.lookup_points()[:64].astype(np.float64)
    q = q[~np.isnan(q).any(axis=1)]
    assert np.all(R.lookup(m, c, 0, q) == 0.25) and np.allclose(R.lookup(m, c, 1, q), 0.25, rtol=0, atol=1e-15)


def test_trackers_of_the_model_against_their_closed_forms():
    """a constant grid rho over a slab: delta tracking scatters with probability 1 - exp(-sigma_t rho l), and ratio tracking's mean is
    exp(-sigma_t rho l); 4 standard errors of the samples' own spread"""
    n, rho, length = 40000, 0.5, 1.5
    m = medium_ref.Medium(2.0, 1.0, 0.0, (-1, -1, 0), (1, 1, length))
    g = np.full((2, 5, 3), rho, np.float32)
    o, d = np.zeros((n, 3), np.float32), np.tile(np.float32([0, 0, 1]), (n, 1))
    o[:, 2] = -1.0
    state = np.random.default_rng(3).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    p = 1.0 - np.exp(-m.sigma_t * rho * length)
    dl = R.delta_track(m, g, 0, o, d, np.full(n, np.inf, np.float32), state)
    assert abs(dl["scattered"].mean() - p) <= 4.0 * np.sqrt(p * (1 - p) / n)
    draws = 2 * dl["steps"] + np.where(dl["scattered"], 0, 1)                  # two per tentative collision, one for the flight that leaves
    want = state.copy()
    for _ in range(int(draws.max())):
        want = np.where(draws > 0, R.rng_next(want)[0], want)
        draws = np.maximum(draws, 1) - 1
    assert np.array_equal(dl["rng"], want)
    assert np.all((dl["t"][dl["scattered"]] > 1.0) & (dl["t"][dl["scattered"]] < 1.0 + length))
    rt = R.ratio_track(m, g, 1, o, d, np.full(n, -1.0, np.float32), state)
    T = rt["value"]
    assert abs(T.mean() - (1 - p)) <= 4.0 * T.std(ddof=1) / np.sqrt(n) and np.all(rt["t"] == 1.0 + length)
    # rho = 1 is the homogeneous medium: the first tentative collision is real; rho = 0 never scatters and T stays 1
    one, zero = np.ones((1, 1, 1), np.float32), np.zeros((1, 1, 1), np.float32)
    d1 = R.delta_track(m, one, 0, o, d, np.full(n, np.inf, np.float32), state)
    assert np.all(d1["steps"] == d1["scattered"])
    s, r = R.rng_next(state)
    assert np.array_equal(d1["scattered"], 1.0 + medium_ref.free_flight(m, r) < 1.0 + length)
    d0 = R.delta_track(m, zero, 0, o, d, np.full(n, np.inf, np.float32), state)
    assert not d0["scattered"].any() and d0["steps"].max() > 3
    assert np.all(R.ratio_track(m, zero, 0, o, d, np.full(n, -1.0, np.float32), state)["value"] == 1.0)
    assert np.all((R.ratio_track(m, one, 0, o, d, np.full(n, -1.0, np.float32), state)["value"] == 0.0) == d1["scattered"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("dims", R.GRID_DIMS)
def test_the_two_precisions_take_the_same_decisions(dims, filt, mode):
    """No device call. Fewer than 2 % of the probe rays are set aside for the committed seeds, the rays exercise the loops, stay far from
    the cap, and the float32 model's values are within rounding of the float64 model's on the rays that are not set aside."""
    m64, m32, aside = R.models(dims, filt, mode)
    keep = ~aside
    dev_t, dev_v = R.deviation(m32["t"][keep], m64["t"][keep]), R.deviation(m32["value"][keep], m64["value"][keep])
    print("grid %s filter %d mode %d: %.3f %% set aside, up to %d tentative collisions (mean %.2f), deviation of t %.3g, of the value %.3g"
          % (dims, filt, mode, 100 * aside.mean(), m64["steps"].max(), m64["steps"].mean(), dev_t, dev_v))
    assert aside.mean() < R.ASIDE_CAP
    assert np.array_equal(m32["rng"][keep], m64["rng"][keep])
    assert m64["steps"].max() >= 5 and m64["steps"].max() < R.TRACK_CAP // 100 and (m64["steps"] == 0).any()
    if mode == 0:
        assert 0.1 < m64["scattered"].mean() < 0.9
    else:
        assert ((m64["value"] > 0) & (m64["value"] < 1)).mean() > 0.1
    assert dev_t <= 1e-5 and dev_v <= 1e-5


@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("dims", R.GRID_DIMS)
def test_lookup_of_the_two_precisions(dims, filt):
    m, g, p = R.probe_medium(), R.probe_grid(dims), R.lookup_points()
    a, b = R.lookup(m, g, filt, p.astype(np.float64), np.float64), R.lookup(m, g, filt, p, np.float32)
    if filt == 0:
        # the points are float32 and the cell faces of these boxes are not: both precisions find the same cell but on the few points
        # within a rounding of a face
        same = a == b
        print("grid %s nearest: %d of %d points in another cell" % (dims, (~same).sum(), len(p)))
        assert (~same).mean() < R.ASIDE_CAP
    else:
        dev = R.deviation(b, a)
        print("grid %s trilinear: deviation %.3g" % (dims, dev))
        assert dev <= 1e-5


def test_grid_structs_by_a_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(ptmi_medium_grid), offsetof(ptmi_medium_grid, reserved),\n'
                   '       sizeof(struct ptmi_medium_grid_status), offsetof(struct ptmi_medium_grid_status, rho_min),\n'
                   '       offsetof(struct ptmi_medium_grid_status, rho_mean), sizeof(ptmi_medium), PTMI_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 4, 32, 16, 24, 64, 4]
    assert ctypes.sizeof(native.MediumGrid) == 32 and ctypes.sizeof(native.MediumGridStatus) == 32
    assert native.MediumGridStatus.rho_mean.offset == 24 and native.ABI_VERSION == 4


def test_library_exports_the_new_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert f in native.EXPORTS and getattr(L, f)


def test_calls_without_a_handle_are_invalid():
    """the checks that come before any device is touched"""
    L = native.load()
    one = np.ones(1, np.float32)
    st = native.MediumGridStatus()
    assert L.ptmi_upload_medium_density(None, native._p(one), 1, 1, 1, None) == -1
    assert L.ptmi_multi_upload_medium_density(None, native._p(one), 1, 1, 1, None) == -1
    assert L.ptmi_medium_grid_status(None, ctypes.byref(st)) == -1
    assert L.ptmi_debug_medium_density(None, 1, native._p(np.zeros(3, np.float32)), native._p(one)) == -1
    assert L.ptmi_debug_medium_track(None, 0, None, None, None, None, 0, None, None, None, None, None) == -1


def test_argument_checks_without_a_device():
    """every PTMI_E_* case of ptmi_upload_medium_density's checks, through the host-only entry point that runs them"""
    g = R.probe_grid((3, 5, 2))
    box = ((-1.0, 0.0, -2.0), (2.0, 1.0, 2.0))
    diag = float(np.linalg.norm(np.float64(box[1]) - np.float64(box[0])))
    med = dict(sigma_t=1.5, albedo=(0.9, 0.8, 0.7), g=0.4, box=box)
    st = native.medium_grid_check(g, filter=1, medium=med).as_dict()
    assert dict(st, rho_mean=0) == dict(dims=(3, 5, 2), filter=1, rho_min=0.0, rho_max=1.0, rho_mean=0)
    assert abs(st["rho_mean"] - float(g.astype(np.float64).mean())) < 1e-12
    assert native.medium_grid_check(np.full((1, 1, 1), 0.25, np.float32)).as_dict() == dict(dims=(1, 1, 1), filter=0, rho_min=0.25,
                                                                                            rho_max=0.25, rho_mean=0.25)
    native.medium_grid_check(np.zeros((1, 1, 1024), np.float32))                     # the largest dimension
    native.medium_grid_check(np.float32([0.0, 1.0]).reshape(2, 1, 1))                # both ends of the range

    def code(*a, **kw):
        with pytest.raises(native.PtmiError) as e:
            native.medium_grid_check(*a, **kw)
        assert str(e.value).split(": ", 1)[1]                                        # a reason is given
        return e.value.code
    for v in (1.0000001, -1e-6, -0.0 - 1e-38, np.nan, np.inf, -np.inf):
        bad = g.copy()
        bad[1, 3, 2] = v
        assert code(bad) == -1 and code(bad, medium=med) == -1, v
    for kw in (dict(filter=2), dict(filter=0xFFFFFFFF), dict(reserved=(0, 0, 0, 0, 0, 0, 1)), dict(reserved=(1, 0, 0, 0, 0, 0, 0)),
               dict(dims=(1025, 1, 1)), dict(dims=(1, 1025, 1)), dict(dims=(1, 1, 1025)), dict(dims=(3, 0, 2))):
        assert code(g, **kw) == -1, kw
    assert code(g, medium=dict(med, sigma_t=-1.0)) == -1                             # a medium ptmi_set_medium would refuse
    # the optical-depth limit: sigma_t * |box diagonal| <= 256, on either side of it; a bad value is reported before it
    assert code(g, medium=dict(med, sigma_t=256.5 / diag)) == -5
    native.medium_grid_check(g, medium=dict(med, sigma_t=255.5 / diag))
    bad = g.copy()
    bad[0, 0, 0] = 2.0
    assert code(bad, medium=dict(med, sigma_t=256.5 / diag)) == -1
