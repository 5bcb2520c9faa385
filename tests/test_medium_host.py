"""The participating medium without a GPU (include/ptmi.h ptmi_set_medium): the float64 model of tests/medium_ref.py checked against
what it must satisfy by itself (the phase density integrates to 1 and has mean cosine g, the sampled direction is unit and makes the
sampled angle with the ray), the layout of ptmi_medium by a C compiler, and the new symbols."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import medium_ref
import medium_ref as G
from ptmi import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ptmi_set_medium", "ptmi_get_medium", "ptmi_multi_set_medium", "ptmi_debug_medium_step", "ptmi_debug_medium_tr"]
N = 100_000


@pytest.mark.parametrize("g", [0.0, 0.6, -0.8, 0.99])
def test_phase_density_integrates_to_one(g):
    """over the sphere: 2 pi times the integral over cos theta, composite Simpson on a grid fine enough for the peak of g = 0.99
    (width ~ (1 - g)^2 = 1e-4 in cos theta; 2^22 intervals: the rule's error is far below the bound)"""
    n = 1 << 22
    mu = np.linspace(-1.0, 1.0, n + 1)
    p = medium_ref.phase(g, mu)
    w = np.ones(n + 1)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    total = 2.0 * np.pi * (w * p).sum() * (2.0 / n) / 3.0
    assert abs(total - 1.0) <= 1e-9


@pytest.mark.parametrize("g", [0.0, 0.6, -0.8, 0.99])
def test_mean_cosine_of_the_samples_is_g(g):
    """E[cos theta] = g for Henyey-Greenstein; the tolerance is 4 standard errors of the mean, from the samples' own variance"""
    xi = np.random.default_rng(17).random(N, np.float32)
    ct = medium_ref.sample_cos(g, xi)
    se = ct.std(ddof=1) / np.sqrt(N)
    g32 = float(np.float32(g))
    print("g %g: mean cos %.6f, standard error %.2g" % (g, ct.mean(), se))
    assert abs(ct.mean() - g32) <= 4.0 * se
    # and the samples follow the phase density: the share with cos theta below c is the density's integral from -1 to c,
    # 2 pi int p = (1 - g^2) / (2 g) (1 / sqrt(1 + g^2 - 2 g c) - 1 / (1 + g)), within 4 binomial standard deviations
    for c in (-0.5, 0.0, 0.5, g32):
        F = (c + 1.0) / 2.0 if abs(g32) < 1e-3 else (1.0 - g32 ** 2) / (2.0 * g32) * (1.0 / np.sqrt(1.0 + g32 ** 2 - 2.0 * g32 * c) - 1.0 / (1.0 + g32))
        share = float((ct < c).mean())
        assert abs(share - F) <= 4.0 * np.sqrt(max(F * (1.0 - F), 1.0 / N) / N), (c, share, F)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("g", [0.0, 0.6, -0.8, 0.99])
def test_sampled_direction_is_unit_and_makes_the_sampled_angle(g):
    rng = np.random.default_rng(23)
    d = unit(rng.normal(size=(4096, 3)))
    d[:8] = unit([(0, 0, -1), (0, 0, 1), (1, 0, 0), (0, 1, 0), (0, -1, 0), (-1, 0, 0), (1e-4, 0, -1), (0.6, 0, -0.8)])   # the frame's branch
    xi = rng.random((len(d), 2), np.float32)
    xi[:4] = [(0, 0), (0.5, 0.25), (np.float32(1 - 2.0 ** -24), 0.5), (0.25, np.float32(1 - 2.0 ** -24))]
    direc, ct = medium_ref.sample_direction(g, d, xi[:, 0], xi[:, 1])
    d64 = d.astype(np.float64)
    # d is a float32 unit vector: |d| = 1 within 1e-7, so the frame is orthonormal within that and the cosine moves as much
    assert np.all(np.abs(np.linalg.norm(direc, axis=1) - 1.0) <= 1e-12)
    assert np.all(np.abs((direc * d64).sum(axis=1) - ct) <= 5e-7)
    assert np.isfinite(direc).all()
    # the density of the sampled direction is the phase value at the sampled cosine: what next-event estimation evaluates. A cosine
    # that moves by e moves p by at most 3 |g| e / (1 - |g|)^2 of itself (d ln p / d cos = 3 g / k, k >= (1 - |g|)^2); e is the 5e-7 above
    rtol = 3.0 * abs(g) * 5e-7 / (1.0 - abs(g)) ** 2 + 1e-12
    assert np.allclose(medium_ref.phase(g, (direc * d64).sum(axis=1)), medium_ref.phase(g, ct), rtol=rtol, atol=0.0)


def test_medium_struct_is_64_bytes_by_a_c_compiler(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ptmi_medium), offsetof(ptmi_medium, sigma_t), offsetof(ptmi_medium, albedo),\n'
                   'offsetof(ptmi_medium, g), offsetof(ptmi_medium, box_min), offsetof(ptmi_medium, box_max), offsetof(ptmi_medium, reserved));\n'
                   'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    M = native.Medium
    assert got[0] == ctypes.sizeof(M) == 64
    assert got[1:] == [M.sigma_t.offset, M.albedo.offset, M.g.offset, M.box_min.offset, M.box_max.offset, M.reserved.offset]
    assert got[1:] == [0, 4, 16, 20, 32, 44]


def test_library_exports_the_new_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS


def test_interval_of_the_model_on_hand_cases():
    m = medium_ref.Medium(1.0, 1.0, 0.0, (-1, -1, -1), (1, 1, 1))
    inf = np.inf
    o = np.float32([(0, 0, 0), (-3, 0, 0), (-1, 0, 0), (0, 0, -3), (0, 5, -3), (3, 0, 0), (0, 0, 0), (-1, 0, 0)])
    d = np.float32([(1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 0, 1), (0, 0, 1), (1, 0, 0), (1, 0, 0), (0, 1, 0)])
    t = np.float32([inf, inf, inf, inf, inf, inf, 0.5, inf])
    _, _, a, b = medium_ref.interval(m, o, d, t)
    want = [(0, 1), (2, 4), (0, 2), (2, 4), None, None, (0, 0.5), None]        # inside, outside, on a face, axis-parallel, two misses,
    for k, w in enumerate(want):                                                 # a hit inside the box, on a face and parallel to it
        if w is None:
            assert not b[k] > a[k], k
        else:
            assert (a[k], b[k]) == w, k
    # min == max on an axis: no ray traverses it (but for one that lies in that plane with a direction component of exactly 0 there,
    # whose two NaNs drop out: the last assertion)
    flat = medium_ref.Medium(1.0, 1.0, 0.0, (-1, 0.25, -1), (1, 0.25, 1))
    _, _, a, b = medium_ref.interval(flat, o, d, t)
    assert not np.any(b > a)
    dd = unit(np.random.default_rng(3).normal(size=(1000, 3)))
    _, _, a, b = medium_ref.interval(flat, np.zeros((1000, 3), np.float32) + np.float32((0.1, 0.3, 0.2)), dd, np.full(1000, inf, np.float32))
    assert not np.any(b > a)
    _, _, a, b = medium_ref.interval(flat, np.float32([(0, 0.25, 0)]), np.float32([(1, 0, 0)]), np.float32([inf]))
    assert (a[0], b[0]) == (0, 1)


def test_probe_tolerance_is_four_times_the_float32_models_deviation():
    """No device call: the float32 model against the float64 model on the probes' inputs. Holds the constants beside the probes' test to what is
    measured here, the seed to fewer than 1 % of scatter decisions set aside, and the inputs to the cases they are meant to hold."""
    worst_geom = worst_dir = worst_pdf = 0.0
    for bi in range(len(G.BOXES)):
        o, d, t_hit, r = G.probe_inputs(bi)
        lo, hi = (np.float32(b) for b in G.BOXES[bi])
        inside = np.all((o > lo) & (o < hi), axis=1)
        assert inside.sum() > 1000 and (~inside).sum() > 1000 and np.any((o == lo) | (o == hi), axis=1).sum() > 100
        assert ((d == 0).sum(axis=1) == 2).sum() > 100 and (r[:, 0] == 0).sum() > 50
        for g in (0.0, 0.6, -0.8):
            m = medium_ref.Medium(1.3, 0.8, g, *G.BOXES[bi])
            m64, m32 = medium_ref.step(m, o, d, t_hit, r), medium_ref.step(m, o, d, t_hit, r, np.float32)
            has = m64["b"] > m64["a"]
            assert np.array_equal(has, m32["b"] > m32["a"])                 # the seed: no ray grazes the box within float32 rounding
            assert 1000 < has.sum() < len(o) - 500 and m64["scattered"].sum() > 500 and (has & ~m64["scattered"]).sum() > 200
            assert (has & np.isfinite(t_hit) & (m64["b"] == t_hit)).sum() > 200            # hits inside the box
            geom, dev_dir, pdf, aside = G.step_deviations(m32, m64)
            assert aside < 0.01
            o2, wi, dist = G.tr_inputs(bi)
            geom = max(geom, G.deviation(medium_ref.transmittance(m, o2, wi, dist, np.float32), medium_ref.transmittance(m, o2, wi, dist)))
            worst_geom, worst_dir, worst_pdf = max(worst_geom, geom), max(worst_dir, dev_dir), max(worst_pdf, pdf)
    print("float32 model against float64: a, b, s, x, Tr %.3g, direction %.3g, density %.3g" % (worst_geom, worst_dir, worst_pdf))
    for measured, constant in ((worst_geom, G.MEASURED_GEOM), (worst_dir, G.MEASURED_DIR), (worst_pdf, G.MEASURED_PDF)):
        # the constant is the measurement rounded up in its third digit; numpy's float32 log / sin / cos may differ by an ulp between
        # CPUs, so what is measured here may sit a little to either side of it
        assert 0.5 * constant <= measured <= 1.25 * constant
