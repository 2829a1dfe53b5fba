"""rt_shade_rays / rt_shade_rays_device without a GPU: both are exported with
the types abi.SIGNATURES gives them, the header declares them, and what they
check before they touch a scene fails with a code and a message."""
import ctypes as C
import os
import re

import numpy as np

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p


def test_signatures():
    dp, st, op = C.POINTER(C.c_double), C.POINTER(abi.rt_stats), C.POINTER(abi.rt_options)
    assert abi.SIGNATURES["rt_shade_rays_device"] == (
        C.c_int, [_P, op, C.c_int64, _P, _P, C.c_int32, C.c_uint32, _P, _P, _P, st])
    assert abi.SIGNATURES["rt_shade_rays"] == (
        C.c_int, [_P, op, C.c_int64, dp, dp, C.c_int32, C.c_uint32, dp, C.POINTER(C.c_float), st])


def test_exported_and_bound():
    L = lib()
    raw = C.CDLL(LIB_PATH)
    for name in ("rt_shade_rays", "rt_shade_rays_device"):
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == args


def test_header_declares_both_after_the_ray_queries():
    txt = open(os.path.join(REPO, "include", "rtmi.h")).read()
    sec = txt.index("---- radiance queries")
    assert txt.index("---- ray queries") < sec < txt.index("---- helpers")
    for name in ("rt_shade_rays_device", "rt_shade_rays"):
        assert re.search(r"^int %s\(rt_scene \*scene, const rt_options \*opts, int64_t n," % name, txt[sec:], re.M)


def test_null_scene_is_invalid_with_a_message():
    L = lib()
    o = abi.rt_options(width=1, height=1, precision=abi.RT_FP64)
    a = np.zeros(3)
    p = a.ctypes.data_as(C.POINTER(C.c_double))
    st = abi.rt_stats()
    assert L.rt_shade_rays(None, C.byref(o), 1, p, p, 1, 0, p, None, C.byref(st)) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_shade_rays_device(None, C.byref(o), 1, None, None, 1, 0, None, None, None, None) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
