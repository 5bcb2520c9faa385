"""The tree-rebuild calls at the C ABI (include/ptmi.h ptmi_rebuild_tree): exported, listed by the binding, and both structs laid out as
the binding mirrors them - by the C compiler and by ctypes, the way tests/test_abi_scene_update.py checks its struct. No GPU."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wgpu-path-tracing_amd")
LIB = os.path.join(PKG, "lib", "libptmi.so")
CALLS = ("rebuild_tree", "rebuild_status")


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
        assert hasattr(native.Context, n) and hasattr(native.MultiContext, n)
    assert lib.ptmi_abi_version() == 4 == native.ABI_VERSION        # new calls only: the version stays


def test_structs_match_the_header(tmp_path):
    from ptmi import native
    structs = (("ptmi_rebuild_params", native.RebuildParams), ("struct ptmi_rebuild_status", native.RebuildStatus))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ptmi.h"', 'int main(void) {']
    for i, (st, cls) in enumerate(structs):
        lines += [f'printf("size{i} %zu\\n", sizeof({st}));']
        lines += [f'printf("{i}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    lines += ['printf("options %zu\\n", sizeof(ptmi_options)); printf("stats %zu\\n", sizeof(ptmi_stats));',
              'printf("update %zu\\n", sizeof(struct ptmi_scene_update_status));', 'return 0; }']
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for i, (st, cls) in enumerate(structs):
        assert int(got[f"size{i}"]) == ctypes.sizeof(cls) == 32, st
        for f, _ in cls._fields_:
            assert int(got[f"{i}.{f}"]) == getattr(cls, f).offset, (st, f)
    # the structs every caller already has did not grow
    assert int(got["options"]) == ctypes.sizeof(native.Options) and int(got["stats"]) == ctypes.sizeof(native.Stats)
    assert int(got["update"]) == ctypes.sizeof(native.SceneUpdateStatus) == 80


def test_refusals_without_a_device(lib):
    """a NULL handle is refused before anything is touched"""
    prm, st = (ctypes.c_uint32 * 8)(), (ctypes.c_uint64 * 4)()
    for prefix in ("ptmi_", "ptmi_multi_"):
        assert getattr(lib, prefix + "rebuild_tree")(None, None) != 0
        assert getattr(lib, prefix + "rebuild_tree")(None, ctypes.byref(prm)) != 0
        assert getattr(lib, prefix + "rebuild_status")(None, ctypes.byref(st)) != 0
        assert getattr(lib, prefix + "rebuild_status")(None, None) != 0
