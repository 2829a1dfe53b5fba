"""rt_trace_rays_f32 / rt_pick_pixels_f32 and their _device forms without a
GPU: the four are exported with the types abi.SIGNATURES gives them, rt_hit32
is 16 bytes, the header declares them in a section of their own before the
helpers, and the argument errors that return before any device work fail with
their codes and a message."""
import ctypes as C
import os
import re

import numpy as np

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
NAMES = ("rt_trace_rays_f32", "rt_trace_rays_f32_device", "rt_pick_pixels_f32", "rt_pick_pixels_f32_device")


def test_hit32_is_16_bytes():
    assert C.sizeof(abi.rt_hit32) == 16
    assert [(n, t) for n, t in abi.rt_hit32._fields_] == [("t", C.c_float), ("obj", C.c_int32), ("face", C.c_int32),
                                                         ("reserved", C.c_int32)]
    assert (abi.rt_hit32.t.offset, abi.rt_hit32.obj.offset, abi.rt_hit32.face.offset,
            abi.rt_hit32.reserved.offset) == (0, 4, 8, 12)


def test_signatures():
    fp, st, op, hp = C.POINTER(C.c_float), C.POINTER(abi.rt_stats), C.POINTER(abi.rt_options), C.POINTER(abi.rt_hit32)
    assert abi.SIGNATURES["rt_trace_rays_f32_device"] == (
        C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_uint32, _P, _P, _P, st])
    assert abi.SIGNATURES["rt_trace_rays_f32"] == (C.c_int, [_P, C.c_int64, fp, fp, fp, C.c_uint32, hp, fp, st])
    assert abi.SIGNATURES["rt_pick_pixels_f32_device"] == (
        C.c_int, [_P, op, C.c_int64, _P, C.c_uint32, _P, _P, _P, st])
    assert abi.SIGNATURES["rt_pick_pixels_f32"] == (C.c_int, [_P, op, C.c_int64, fp, C.c_uint32, hp, fp, st])


def test_exported_and_bound():
    L = lib()
    raw = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == args
    assert hasattr(raw, "rtmi_test_trace32_subset")


def test_header_declares_the_four_in_their_own_section():
    txt = open(os.path.join(REPO, "include", "rtmi.h")).read()
    sec = txt.index("---- float32 ray queries")
    assert txt.index("---- float32 radiance queries") < sec < txt.index("---- helpers")
    body = txt[sec:txt.index("---- helpers")]
    assert re.search(r"typedef struct rt_hit32 \{[^}]*float\s+t;[^}]*int32_t obj;[^}]*int32_t face;[^}]*"
                     r"int32_t reserved;[^}]*\} rt_hit32;", body)
    assert re.search(r"^int rt_trace_rays_f32_device\(rt_scene \*scene, int64_t n, const float \*d_orig,\s*"
                     r"const float \*d_dir, const float \*d_tnear,\s*uint32_t flags, rt_hit32 \*d_hits, "
                     r"float \*d_normals,\s*void \*hip_stream, rt_stats \*out\);", body, re.M)
    assert re.search(r"^int rt_trace_rays_f32\(rt_scene \*scene, int64_t n, const float \*orig,\s*"
                     r"const float \*dir, const float \*tnear, uint32_t flags,\s*rt_hit32 \*hits, float \*normals, "
                     r"rt_stats \*out\);", body, re.M)
    assert re.search(r"^int rt_pick_pixels_f32_device\(rt_scene \*scene, const rt_options \*opts, int64_t n,\s*"
                     r"const float \*d_xy, uint32_t flags, rt_hit32 \*d_hits,\s*float \*d_normals, "
                     r"void \*hip_stream, rt_stats \*out\);", body, re.M)
    assert re.search(r"^int rt_pick_pixels_f32\(rt_scene \*scene, const rt_options \*opts, int64_t n,\s*"
                     r"const float \*xy, uint32_t flags, rt_hit32 \*hits,\s*float \*normals, rt_stats \*out\);",
                     body, re.M)
    # none is declared before its section; the float64 pick still refuses RT_FP32
    assert "_f32(" not in txt[:txt.index("---- float32 radiance queries")]
    assert "rt_trace_rays_f32(" not in txt[:sec].replace("rt_trace_rays_f32 ", "")
    assert "there is no float32 mode" not in txt


def test_argument_errors_before_any_device_work():
    L = lib()
    fp = C.POINTER(C.c_float)
    a = np.zeros(12, np.float32)
    p = a.ctypes.data_as(fp)
    hits = (abi.rt_hit32 * 4)()
    st = abi.rt_stats()
    o32 = abi.rt_options(width=8, height=8, precision=abi.RT_FP32)
    # a null scene, in all four
    assert L.rt_trace_rays_f32(None, 4, p, p, None, 0, hits, None, C.byref(st)) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_trace_rays_f32_device(None, 4, None, None, None, 0, None, None, None, None) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_pick_pixels_f32(None, C.byref(o32), 4, p, 0, hits, None, C.byref(st)) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_pick_pixels_f32_device(None, C.byref(o32), 4, None, 0, None, None, None, None) == abi.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
