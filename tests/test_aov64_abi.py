"""rt_render_aovs_f64 / rt_render_aovs_f64_device without a GPU: both are
exported with the types abi.SIGNATURES gives them, rt_aov_buffers64 is six
pointers (48 bytes) in the header's order, the header declares them in the
feature-buffer section after the float32 pair, and the argument errors that
return before any device work fail with their code and a message."""
import ctypes as C
import os
import re

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
NAMES = ("rt_render_aovs_f64", "rt_render_aovs_f64_device")
FIELDS = ("alpha", "depth", "object", "face", "normal", "albedo")


def test_buffers_struct_is_six_pointers():
    assert C.sizeof(abi.rt_aov_buffers64) == 48
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert [(n, t) for n, t in abi.rt_aov_buffers64._fields_] == [
        ("alpha", dp), ("depth", dp), ("object", ip), ("face", ip), ("normal", dp), ("albedo", dp)]
    assert [getattr(abi.rt_aov_buffers64, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40]


def test_signatures():
    st, op, bp = C.POINTER(abi.rt_stats), C.POINTER(abi.rt_options), C.POINTER(abi.rt_aov_buffers64)
    assert abi.SIGNATURES["rt_render_aovs_f64_device"] == (C.c_int, [_P, op, bp, C.c_int32, C.c_int32, _P, st])
    assert abi.SIGNATURES["rt_render_aovs_f64"] == (C.c_int, [_P, op, bp, C.c_int32, C.c_int32, st])


def test_exported_and_bound():
    L = lib()
    raw = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == args


def test_header_declares_them_after_the_float32_pair():
    txt = open(os.path.join(REPO, "include", "rtmi.h")).read()
    sec = txt.index("---- feature buffers")
    helpers = txt.index("---- helpers")
    body = txt[sec:helpers]
    assert "rt_render_aovs_f64" not in txt[:sec] and "rt_aov_buffers64" not in txt[:sec]
    assert body.index("} rt_aov_buffers;") < body.index("int rt_render_aovs(") < body.index("typedef struct rt_aov_buffers64")
    m = re.search(r"typedef struct rt_aov_buffers64 \{(.*?)\} rt_aov_buffers64;", body, re.S)
    assert m
    assert re.findall(r"^\s*(double|int32_t)\s*\*(\w+);", m.group(1), re.M) == [
        ("double", "alpha"), ("double", "depth"), ("int32_t", "object"), ("int32_t", "face"), ("double", "normal"),
        ("double", "albedo")]
    assert re.search(r"^int rt_render_aovs_f64_device\(rt_scene \*scene, const rt_options \*opts, "
                     r"const rt_aov_buffers64 \*d_out,\s*int32_t y0, int32_t y1, void \*hip_stream, rt_stats \*out\);",
                     body, re.M)
    assert re.search(r"^int rt_render_aovs_f64\(rt_scene \*scene, const rt_options \*opts, "
                     r"const rt_aov_buffers64 \*out_bufs,\s*int32_t y0, int32_t y1, rt_stats \*out\);", body, re.M)


def test_argument_errors_before_any_device_work():
    L = lib()
    st = abi.rt_stats()
    o = abi.rt_options(width=8, height=8, precision=abi.RT_FP64)
    b = abi.rt_aov_buffers64()
    fake = C.c_void_p(1)  # never dereferenced: the null checks come first
    for scene, opts, bufs in ((None, C.byref(o), C.byref(b)), (fake, None, C.byref(b)), (fake, C.byref(o), None)):
        assert L.rt_render_aovs_f64(scene, opts, bufs, 0, 8, C.byref(st)) == abi.RT_E_INVALID
        assert b"null" in L.rt_last_error()
        assert L.rt_render_aovs_f64_device(scene, opts, bufs, 0, 8, None, None) == abi.RT_E_INVALID
        assert b"null" in L.rt_last_error()
    # RT_FP32 belongs to rt_render_aovs, and the message says so (checked before the scene is read)
    o32 = abi.rt_options(width=8, height=8, precision=abi.RT_FP32)
    assert L.rt_render_aovs_f64(fake, C.byref(o32), C.byref(b), 0, 8, None) == abi.RT_E_INVALID
    assert b"rt_render_aovs " in L.rt_last_error() + b" "
    assert L.rt_render_aovs_f64_device(fake, C.byref(o32), C.byref(b), 0, 8, None, None) == abi.RT_E_INVALID
