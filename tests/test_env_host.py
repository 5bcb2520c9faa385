"""The environment map's tables without a GPU (include/ptmi.h ptmi_debug_env_table): c_t, the alias table and the weight sum against
the float64 model of tests/env_ref.py; rejected inputs; the new symbols and the layout of the two new structs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import env_ref
from ptmi import native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ptmi_upload_environment", "ptmi_set_environment", "ptmi_environment_status", "ptmi_multi_upload_environment",
       "ptmi_multi_set_environment", "ptmi_debug_env_lookup", "ptmi_debug_env_sample", "ptmi_debug_env_table"]


def make_map(W, H, content):
    t = np.ones((H, W, 4), np.float32)
    if content == "constant":
        t[..., :3] = (0.3, 0.2, 0.1)
    elif content == "gradient":
        t = scenes.sky(W, H, "gradient")
    elif content == "one_bright":
        t[..., :3] = 0.01
        t[H // 3, (2 * W) // 3, :3] = (900.0, 800.0, 700.0)
    elif content == "one_black_row":
        t = scenes.sky(W, H, "gradient")
        t[H // 2, :, :3] = 0.0
    return t


CASES = [(W, H, c) for (W, H) in ((16, 8), (64, 32), (1, 1)) for c in ("constant", "gradient", "one_bright", "one_black_row")
         if not ((W, H) == (1, 1) and c == "one_black_row")]            # (a 1 x 1 map with its one row black is the all-black map below)


@pytest.mark.parametrize("W,H,content", CASES)
def test_tables_match_the_model(W, H, content):
    t = make_map(W, H, content)
    c, prob, alias, wsum = native.env_table(t)
    w, P, c_ref, total = env_ref.weights(t)
    N = W * H
    assert abs(P.sum() - 1.0) <= 1e-12
    assert abs(wsum - total) <= 1e-12 * total
    # c_t: a double result rounded to float32 once
    assert np.all(np.abs(c.astype(np.float64) - c_ref) <= 2.0 ** -23 * c_ref)
    # what the table selects: entry k picks itself with prob[k] and alias[k] otherwise
    assert alias.max() < N and np.all((prob >= 0) & (prob <= 1))
    p64 = prob.astype(np.float64)
    implied = p64.copy()
    np.add.at(implied, alias, 1.0 - p64)
    m = np.bincount(alias[p64 < 1.0], minlength=N)              # entries aliasing to t (an entry of prob 1 never takes its alias)
    assert np.all(np.abs(implied / N - P.reshape(-1)) <= (m + 2) * 2.0 ** -24 / N)
    # a texel of probability zero is never selected
    zero = P.reshape(-1) == 0
    assert np.all(prob[zero] == 0) and not np.isin(alias[p64 < 1.0], np.flatnonzero(zero)).any()
    if content == "one_black_row":
        assert zero.sum() == W


def test_f16_map_gives_the_tables_of_its_values():
    t16 = make_map(16, 8, "gradient").astype(np.float16)
    a, b = native.env_table(t16), native.env_table(t16.astype(np.float32))
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]


def test_all_black_map_is_never_sampled():
    t = np.zeros((8, 16, 4), np.float32)
    t[..., 3] = 1.0                                              # alpha is not radiance
    c, prob, alias, wsum = native.env_table(t)
    assert wsum == 0.0 and not c.any() and not prob.any() and np.array_equal(alias, np.arange(128))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -0.5])
def test_bad_texels_are_rejected(bad):
    t = make_map(16, 8, "gradient")
    t[5, 7, 1] = bad
    with pytest.raises(native.PtmiError) as e:
        native.env_table(t)
    assert e.value.code == -1 and "(7, 5)" in str(e.value)
    t16 = make_map(16, 8, "gradient").astype(np.float16)
    t16[0, 0, 2] = bad
    with pytest.raises(native.PtmiError):
        native.env_table(t16)


def test_unknown_format_and_size_overflow_are_rejected():
    t = make_map(16, 8, "constant")
    for kw in ({"fmt": 3}, {"fmt": 0}, {"width": 0xFFFFFFFF, "height": 0xFFFFFFFF}, {"width": 1 << 20, "height": 1 << 20}):
        with pytest.raises(native.PtmiError) as e:
            native.env_table(t, **kw)
        assert e.value.code == -1


def test_new_symbols_and_struct_layout(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)
    L = native.load()
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(L, f) and f in native.EXPORTS
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ptmi.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ptmi_environment), sizeof(struct ptmi_environment_status),\n'
                   'offsetof(ptmi_environment, sample), offsetof(ptmi_environment, reserved),\n'
                   'offsetof(struct ptmi_environment_status, sampled), offsetof(struct ptmi_environment_status, weight_sum));\n'
                   'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == ctypes.sizeof(native.Environment) == 32
    assert got[1] == ctypes.sizeof(native.EnvironmentStatus) == 24
    assert got[2:] == [native.Environment.sample.offset, native.Environment.reserved.offset,
                       native.EnvironmentStatus.sampled.offset, native.EnvironmentStatus.weight_sum.offset]


def test_sky_helper_kinds():
    for kind in ("constant", "gradient", "disc"):
        t = scenes.sky(64, 32, kind)
        assert t.shape == (32, 64, 4) and t.dtype == np.float32 and np.isfinite(t).all() and (t >= 0).all()
    assert np.all(scenes.sky(16, 8, "constant")[..., :3] == np.float32((0.3, 0.2, 0.1)))
    g, d = scenes.sky(64, 32, "gradient"), scenes.sky(64, 32, "disc")
    assert np.all(g == g[:, :1]) and 0 < (d != g).any(-1).sum() <= 16          # rows are constant; the disc is small
    with pytest.raises(ValueError):
        scenes.sky(4, 2, "nope")
