"""rt_scene_set_objects / rt_multi_set_objects without a GPU: both are exported
with the signatures abi.SIGNATURES lists, and a null handle is an error code
with a message, not a crash; the flattening an update shares with the
constructor, and the drop-in cache's pose key."""
import ctypes as C

import numpy as np
import pytest

from rtmi import abi, scenes
from rtmi._lib import LIB_PATH, lib
from rtmi.glm import inverse, translate, vec3
from rtmi.scene import flatten, flatten_objects

NAMES = ("rt_scene_set_objects", "rt_multi_set_objects")


def test_entry_points_exported_with_signatures():
    lib()
    raw = C.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int
        assert args == [C.c_void_p, C.POINTER(abi.rt_object_desc), C.c_int32]
        fn = getattr(lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_null_handles_are_invalid():
    L = lib()
    objs = (abi.rt_object_desc * 1)()
    for name in NAMES:
        assert getattr(L, name)(None, objs, 1) == abi.RT_E_INVALID
        msg = L.rt_last_error()
        assert msg and b"null" in msg, msg
        assert getattr(L, name)(None, None, 0) == abi.RT_E_INVALID
        assert L.rt_last_error()


def test_flatten_objects_is_what_the_constructor_flattens():
    sc = scenes.mesh_mix()
    flat = flatten(sc)
    n = len(sc.objects)
    arr, meshes = flatten_objects(sc.objects, [id(g) for g in flat._meshes])
    assert meshes == []  # an update adds no mesh
    assert bytes(arr)[:n * C.sizeof(abi.rt_object_desc)] == bytes(flat._objs)[:n * C.sizeof(abi.rt_object_desc)]
    other = scenes.mesh_mix()  # equal data, other TriangleMesh objects
    with pytest.raises(ValueError, match="object"):
        flatten_objects(other.objects, [id(g) for g in flat._meshes])


def test_pose_key_splits_from_shape_key():
    from rtmi.renderer import _pose_key, _shape_key
    from rtmi.scene import Box
    sc = scenes.boxes2()
    shape, pose = _shape_key(sc), _pose_key(sc)
    ob = next(o for o in sc.objects if isinstance(o.geometry, Box))
    ob.geometry.objectToWorld = translate(ob.geometry.objectToWorld, vec3(0.5, 0.0, 0.25))
    ob.geometry.worldToObject = inverse(ob.geometry.objectToWorld)
    ob.material.albedo = vec3(0.1, 0.2, 0.3)
    assert _shape_key(sc) == shape and _pose_key(sc) != pose
    pose = _pose_key(sc)
    ob.geometry.vmax = ob.geometry.vmax + np.array([0.0, 0.35, 0.0])
    assert _shape_key(sc) != shape and _pose_key(sc) == pose
