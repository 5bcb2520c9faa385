"""The scene-update calls at the C ABI (include/ptmi.h ptmi_update_triangles): exported, listed by the binding, and their status struct
laid out as the binding mirrors it - by the C compiler and by ctypes, the way tests/test_abi_reproject.py checks its structs. No GPU."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wgpu-path-tracing_amd")
LIB = os.path.join(PKG, "lib", "libptmi.so")
CALLS = ("update_triangles", "update_materials", "update_lights", "scene_update_status")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", PKG, "all"], stdout=subprocess.DEVNULL)
    return ctypes.CDLL(LIB)


def test_symbols_exported(lib):
    from ptmi import native
    for prefix in ("ptmi_", "ptmi_multi_"):
        for n in CALLS:
            assert hasattr(lib, prefix + n), prefix + n
            assert prefix + n in native.EXPORTS
    for n in CALLS:
        assert n in native._SHARED and hasattr(native._Handle, n)
    assert lib.ptmi_abi_version() == 4                  # new calls only: the version stays


def test_status_struct_matches_the_header(tmp_path):
    from ptmi import native
    st, cls = "struct ptmi_scene_update_status", native.SceneUpdateStatus
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptmi.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({st}));']
    lines += [f'printf("{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines += ['printf("options %zu\\n", sizeof(ptmi_options)); printf("stats %zu\\n", sizeof(ptmi_stats));', 'return 0; }']
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 80
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    # the structs every caller already has did not grow
    assert int(got["options"]) == ctypes.sizeof(native.Options) and int(got["stats"]) == ctypes.sizeof(native.Stats)


def test_refusals_without_a_device(lib):
    """a NULL context is refused before anything is touched"""
    for n in CALLS[:3]:
        assert getattr(lib, "ptmi_" + n)(None, 0, 0, None) != 0
    assert lib.ptmi_scene_update_status(None, None) != 0
