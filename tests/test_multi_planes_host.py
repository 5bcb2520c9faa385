"""The planes / adaptive / denoise calls of ptmi_multi without a GPU (include/ptmi.h): the ABI surface, the NULL-handle answers (no
device is touched for them), the binding's methods, and the gather bits."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["ptmi_multi_set_aovs", "ptmi_multi_get_aovs", "ptmi_multi_set_moments", "ptmi_multi_get_moments", "ptmi_multi_gather_planes",
         "ptmi_multi_read_aov", "ptmi_multi_read_moments", "ptmi_multi_dispatch_adaptive", "ptmi_multi_adaptive_status",
         "ptmi_multi_denoise", "ptmi_multi_blit_denoised"]
E_INVALID = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptmi.h")).read(), flags=re.S)


def test_every_new_symbol_is_declared_exported_and_bound():
    from ptmi import native
    h = _header()
    L = native.load()
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, h), f
        assert hasattr(L, f), f
        assert f in native.EXPORTS
    assert re.search(r"#define PTMI_ABI_VERSION 4\b", h) and L.ptmi_abi_version() == 4        # additive: the number stays
    assert not hasattr(L, "ptmi_multi_reproject")                                           # reprojection stays single-device


def test_a_null_handle_is_refused_without_touching_a_device():
    from ptmi import native
    L = native.load()
    buf = (ctypes.c_float * 16)()
    word = ctypes.c_uint32(7)
    cam = (ctypes.c_uint8 * 256)()
    prm = native.AdaptiveParams(0.35, 0.05, 4, 64, 4, 1)
    st = native.AdaptiveStatus()
    calls = {
        "ptmi_multi_set_aovs": (native.AOV_NORMAL,), "ptmi_multi_get_aovs": (ctypes.byref(word),),
        "ptmi_multi_set_moments": (1,), "ptmi_multi_get_moments": (ctypes.byref(word),),
        "ptmi_multi_gather_planes": (native.AOV_NORMAL,), "ptmi_multi_read_aov": (native.AOV_NORMAL, buf, ctypes.sizeof(buf)),
        "ptmi_multi_read_moments": (buf, 16), "ptmi_multi_dispatch_adaptive": (cam, ctypes.byref(prm), 1),
        "ptmi_multi_adaptive_status": (ctypes.byref(st),), "ptmi_multi_denoise": (None, buf, 16),
        "ptmi_multi_blit_denoised": (buf, 16, None, 0),
    }
    assert sorted(calls) == sorted(FUNCS)
    for f, args in calls.items():
        assert getattr(L, f)(None, *args) == E_INVALID, f
    assert word.value == 7 and not any(buf)


def test_the_binding_has_the_methods():
    from ptmi import native
    for name in ("set_aovs", "aovs", "set_moments", "moments", "read_aov", "read_moments", "gather_planes", "adaptive_status", "denoise",
                 "blit_denoised", "dispatch_adaptive_rounds"):
        assert callable(getattr(native.MultiContext, name, None)), name
    # one implementation for both handle types, bound by the prefix
    for name in ("set_aovs", "read_aov", "read_moments", "denoise", "blit_denoised", "adaptive_status"):
        assert getattr(native.MultiContext, name) is getattr(native.Context, name), name
    assert not hasattr(native.MultiContext, "reproject")


def test_the_gather_bits_extend_the_aov_bits():
    from ptmi import native
    h = _header()
    got = {k: int(v, 0) for k, v in re.findall(r"\b(PTMI_MULTI_PLANE_\w+|PTMI_AOV_\w+)\s*=\s*(0x[0-9a-fA-F]+|\d+)u?", h)}
    assert set(got) == {"PTMI_AOV_ALBEDO", "PTMI_AOV_NORMAL", "PTMI_AOV_ID", "PTMI_MULTI_PLANE_MOMENTS", "PTMI_MULTI_PLANE_OUTPUT"}
    bits = list(got.values())
    assert all(b and not b & (b - 1) for b in bits) and len(set(bits)) == len(bits)         # single bits, all different
    assert got["PTMI_MULTI_PLANE_MOMENTS"] == native.MULTI_PLANE_MOMENTS and got["PTMI_MULTI_PLANE_OUTPUT"] == native.MULTI_PLANE_OUTPUT
    aov = native.AOV_ALBEDO | native.AOV_NORMAL | native.AOV_ID
    assert not aov & (native.MULTI_PLANE_MOMENTS | native.MULTI_PLANE_OUTPUT)
