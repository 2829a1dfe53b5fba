"""Ray queries (rt_trace_rays* / rt_pick_pixels*) without a GPU: rt_hit's
layout as include/rtmi.h defines it, the four entry points exported with
their signatures, and argument validation that fails with codes and messages
before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

from rtmi import abi
from rtmi._lib import lib

ENTRY_POINTS = ("rt_trace_rays_device", "rt_trace_rays", "rt_pick_pixels_device", "rt_pick_pixels")


def test_rt_hit_layout():
    assert C.sizeof(abi.rt_hit) == 16
    assert abi.rt_hit.t.offset == 0
    assert abi.rt_hit.obj.offset == 8
    assert abi.rt_hit.face.offset == 12
    from rtmi.renderer import _HIT_DTYPE
    assert _HIT_DTYPE.itemsize == 16
    assert [_HIT_DTYPE.fields[k][1] for k in ("t", "obj", "face")] == [0, 8, 12]


def test_query_flags():
    assert abi.RT_QUERY_ANY_HIT == 0x1 and abi.RT_QUERY_SORT == 0x2
    assert abi.RTMI_ABI_VERSION == 1 == lib().rt_version()


def test_signatures_present():
    L = lib()
    for name in ENTRY_POINTS:
        assert name in abi.SIGNATURES, name
        res, args = abi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res is C.c_int
        assert list(fn.argtypes) == list(args)
    assert len(abi.SIGNATURES["rt_trace_rays_device"][1]) == 10
    assert len(abi.SIGNATURES["rt_trace_rays"][1]) == 9
    assert len(abi.SIGNATURES["rt_pick_pixels_device"][1]) == 9
    assert len(abi.SIGNATURES["rt_pick_pixels"][1]) == 8


def _call_null_scene(name):
    L = lib()
    hits = (abi.rt_hit * 1)()
    d = (C.c_double * 3)(0.0, 0.0, -1.0)
    o = abi.rt_options()
    o.width, o.height, o.precision = 4, 4, abi.RT_FP64
    if name == "rt_trace_rays_device":
        return L.rt_trace_rays_device(None, 1, C.addressof(d), C.addressof(d), None, 0, C.addressof(hits), None,
                                      None, None)
    if name == "rt_trace_rays":
        return L.rt_trace_rays(None, 1, d, d, None, 0, hits, None, None)
    if name == "rt_pick_pixels_device":
        return L.rt_pick_pixels_device(None, C.byref(o), 1, C.addressof(d), 0, C.addressof(hits), None, None, None)
    return L.rt_pick_pixels(None, C.byref(o), 1, d, 0, hits, None, None)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_scene_is_invalid_with_a_message(name):
    assert _call_null_scene(name) == abi.RT_E_INVALID
    msg = lib().rt_last_error()
    assert msg and b"null scene" in msg


def test_python_layer_rejects_mismatched_host_arrays():
    """DeviceScene.trace_rays checks its arrays before it calls the library
    (no scene is needed to see that)."""
    from rtmi.renderer import DeviceScene
    ds = DeviceScene.__new__(DeviceScene)  # no device copy: the check comes first
    ds.h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.trace_rays(np.zeros((3, 3)), np.zeros((2, 3)))
