"""rt_shade_rays_f32 / rt_shade_rays_f32_device without a GPU: both are
exported with the types abi.SIGNATURES gives them, the header declares them
in a section of their own between the radiance queries and the helpers, and
what they check before they touch a scene fails with a code and a message."""
import ctypes as C
import os
import re

import numpy as np

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
NAMES = ("rt_shade_rays_f32", "rt_shade_rays_f32_device")


def test_signatures():
    fp, st, op = C.POINTER(C.c_float), C.POINTER(abi.rt_stats), C.POINTER(abi.rt_options)
    assert abi.SIGNATURES["rt_shade_rays_f32_device"] == (
        C.c_int, [_P, op, C.c_int64, _P, _P, C.c_int32, C.c_uint32, _P, _P, st])
    assert abi.SIGNATURES["rt_shade_rays_f32"] == (
        C.c_int, [_P, op, C.c_int64, fp, fp, C.c_int32, C.c_uint32, fp, st])


def test_exported_and_bound():
    L = lib()
    raw = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == args
    assert hasattr(raw, "rtmi_test_shade32_subset")


def test_header_declares_both_in_their_own_section():
    txt = open(os.path.join(REPO, "include", "rtmi.h")).read()
    sec = txt.index("---- float32 radiance queries")
    assert txt.index("---- radiance queries") < sec < txt.index("---- helpers")
    body = txt[sec:txt.index("---- helpers")]
    assert re.search(r"^int rt_shade_rays_f32_device\(rt_scene \*scene, const rt_options \*opts, int64_t n,\s*"
                     r"const float \*d_orig, const float \*d_dir, int32_t group,\s*"
                     r"uint32_t flags, float \*d_rgb, void \*hip_stream, rt_stats \*out\);", body, re.M)
    assert re.search(r"^int rt_shade_rays_f32\(rt_scene \*scene, const rt_options \*opts, int64_t n,\s*"
                     r"const float \*orig, const float \*dir, int32_t group,\s*"
                     r"uint32_t flags, float \*rgb, rt_stats \*out\);", body, re.M)
    # neither is declared before its section
    assert "rt_shade_rays_f32(" not in txt[:sec] and "rt_shade_rays_f32_device(" not in txt[:sec]


def test_null_scene_is_invalid_with_a_message():
    L = lib()
    o = abi.rt_options(width=1, height=1, precision=abi.RT_FP32)
    a = np.zeros(3, np.float32)
    p = a.ctypes.data_as(C.POINTER(C.c_float))
    st = abi.rt_stats()
    assert L.rt_shade_rays_f32(None, C.byref(o), 1, p, p, 1, 0, p, C.byref(st)) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_shade_rays_f32_device(None, C.byref(o), 1, None, None, 1, 0, None, None, None) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
