"""rt_scene_set_lights / rt_multi_set_lights without a GPU: both are exported
with the signatures abi.SIGNATURES lists, and a null handle is an error code
with a message, not a crash."""
import ctypes as C

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

NAMES = ("rt_scene_set_lights", "rt_multi_set_lights")


def test_entry_points_exported_with_signatures():
    lib()
    raw = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int
        assert args == [C.c_void_p, C.POINTER(abi.rt_light_desc), C.c_int32]
        fn = getattr(lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_null_handles_are_invalid():
    L = lib()
    lights = (abi.rt_light_desc * 1)()
    for name in NAMES:
        assert getattr(L, name)(None, lights, 1) == abi.RT_E_INVALID
        msg = L.rt_last_error()
        assert msg and b"null" in msg, msg
        assert getattr(L, name)(None, None, 0) == abi.RT_E_INVALID
        assert L.rt_last_error()
