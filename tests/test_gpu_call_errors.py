"""What the 12 query entry points (rt_trace_rays*, rt_pick_pixels*,
rt_shade_rays* and their _f32 forms) and the 4 feature-buffer entry points
(rt_render_aovs*) answer to a bad call: the exact return code and the exact
rt_last_error() text, for every entry point that has the argument. The texts
below are the library's format strings with their arguments filled in, written
out here; nothing is generated from the library. And the calls with nothing to
do (no rays, no rows): RT_OK, all-zero Stats, no message."""
import ctypes as C

import numpy as np
import pytest

from rtmi import abi, scenes
from rtmi._lib import lib
from rtmi.glm import mat4, translate, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import Material, Object, Scene, TriangleMesh, initBox

pytestmark = pytest.mark.gpu

INV, UNS = abi.RT_E_INVALID, abi.RT_E_UNSUPPORTED
W = H = 8
BYTES = 4096  # of every array a call is given: room for W x H pixels of 24 bytes, and for 8 rays

# entry point -> (family, its precision, its arguments by role in call order)
ENTRY = {
    "rt_trace_rays_device": ("trace", 64, "scene n orig dir tnear flags hits normals stream stats"),
    "rt_trace_rays": ("trace", 64, "scene n orig dir tnear flags hits normals stats"),
    "rt_pick_pixels_device": ("pick", 64, "scene opts n xy flags hits normals stream stats"),
    "rt_pick_pixels": ("pick", 64, "scene opts n xy flags hits normals stats"),
    "rt_trace_rays_f32_device": ("trace", 32, "scene n orig dir tnear flags hits normals stream stats"),
    "rt_trace_rays_f32": ("trace", 32, "scene n orig dir tnear flags hits normals stats"),
    "rt_pick_pixels_f32_device": ("pick", 32, "scene opts n xy flags hits normals stream stats"),
    "rt_pick_pixels_f32": ("pick", 32, "scene opts n xy flags hits normals stats"),
    "rt_shade_rays_device": ("shade", 64, "scene opts n orig dir group flags rgb rgb32 stream stats"),
    "rt_shade_rays": ("shade", 64, "scene opts n orig dir group flags rgb rgb32 stats"),
    "rt_shade_rays_f32_device": ("shade", 32, "scene opts n orig dir group flags rgb stream stats"),
    "rt_shade_rays_f32": ("shade", 32, "scene opts n orig dir group flags rgb stats"),
    "rt_render_aovs_device": ("aov", 32, "scene opts bufs y0 y1 stream stats"),
    "rt_render_aovs": ("aov", 32, "scene opts bufs y0 y1 stats"),
    "rt_render_aovs_f64_device": ("aov", 64, "scene opts bufs y0 y1 stream stats"),
    "rt_render_aovs_f64": ("aov", 64, "scene opts bufs y0 y1 stats"),
}
ARRAYS = ("orig", "dir", "tnear", "xy", "hits", "normals", "rgb", "rgb32")
CHANNELS = ("alpha", "depth", "object", "face", "normal", "albedo")

# bad call -> what it changes in a good call (role -> value; "precision", "width":
# fields of the options; "channels": the feature buffers wanted)
OTHER, BAD = "other", 7  # the other precision of the two; a precision that is neither
CASES = {
    "null scene": {"scene": None},
    "null options": {"opts": None},
    "negative n": {"n": -1},
    "unknown flag": {"flags": 0x8},
    "any-hit flag": {"flags": abi.RT_QUERY_ANY_HIT},  # unknown to a radiance query
    "normals with any hit": {"flags": abi.RT_QUERY_ANY_HIT},
    "null hits": {"n": 1, "hits": None},
    "null rgb": {"n": 1, "rgb": None, "rgb32": None},
    "null origins": {"n": 1, "orig": None},
    "null directions": {"n": 1, "dir": None},
    "null positions": {"n": 1, "xy": None},
    "group 0": {"group": 0},
    "5 rays in groups of 2": {"n": 5, "group": 2},
    "other precision": {"precision": OTHER},
    "bad precision": {"precision": BAD},
    "null origins, other precision": {"n": 1, "orig": None, "precision": OTHER},
    "image 0x4": {"width": 0, "height": 4},
    "misaligned hits": {"hits": "+4"},
    "rows before the image": {"y0": -1},
    "rows past the image": {"y1": H + 1},
    "rows reversed": {"y0": 5, "y1": 3},
    "every channel null": {"channels": ()},
    "null buffers": {"bufs": None},
}

F64_PICK = "ray queries are float64 only (precision %d)"
F32_PICK = "rt_pick_pixels_f32 is float32 only (precision %d): rt_pick_pixels is the float64 pick"
F64_SHADE = "radiance queries are float64 only (precision %d)"
F32_SHADE = "rt_shade_rays_f32 is float32 only (precision %d): rt_shade_rays is the float64 query"
F32_AOV = "rt_render_aovs renders the feature buffers of an RT_FP32 frame (precision %d)"
F64_AOV = "rt_render_aovs_f64 renders the feature buffers of an RT_FP64 frame: rt_render_aovs is the RT_FP32 call"
NO_RAYS = "null ray origins or directions"

# (bad call, family, precision or None for both) -> (return code, message)
EXPECT = {
    ("null scene", "trace", None): (INV, "null scene"),
    ("null scene", "pick", None): (INV, "null scene"),
    ("null scene", "shade", None): (INV, "null scene"),
    ("null scene", "aov", None): (INV, "null argument"),
    ("null options", "pick", None): (INV, "null options"),
    ("null options", "shade", None): (INV, "null options"),
    ("null options", "aov", None): (INV, "null argument"),
    ("null buffers", "aov", None): (INV, "null argument"),
    ("negative n", "trace", None): (INV, "negative ray count -1"),
    ("negative n", "pick", None): (INV, "negative ray count -1"),
    ("negative n", "shade", None): (INV, "negative ray count -1"),
    ("unknown flag", "trace", None): (INV, "unknown query flags 0x8"),
    ("unknown flag", "pick", None): (INV, "unknown query flags 0x8"),
    ("unknown flag", "shade", 64): (INV, "rt_shade_rays takes RT_QUERY_SORT only (flags 0x8)"),
    ("unknown flag", "shade", 32): (INV, "rt_shade_rays_f32 takes RT_QUERY_SORT only (flags 0x8)"),
    ("any-hit flag", "shade", 64): (INV, "rt_shade_rays takes RT_QUERY_SORT only (flags 0x1)"),
    ("any-hit flag", "shade", 32): (INV, "rt_shade_rays_f32 takes RT_QUERY_SORT only (flags 0x1)"),
    ("normals with any hit", "trace", None): (INV, "normals are not available with RT_QUERY_ANY_HIT"),
    ("normals with any hit", "pick", None): (INV, "normals are not available with RT_QUERY_ANY_HIT"),
    ("null hits", "trace", None): (INV, "null hits"),
    ("null hits", "pick", None): (INV, "null hits"),
    ("null rgb", "shade", 64): (INV, "null rgb and rgb32"),
    ("null rgb", "shade", 32): (INV, "null rgb"),
    ("null origins", "trace", None): (INV, NO_RAYS),
    ("null origins", "shade", None): (INV, NO_RAYS),
    ("null directions", "trace", None): (INV, NO_RAYS),
    ("null directions", "shade", None): (INV, NO_RAYS),
    ("null positions", "pick", None): (INV, "null pixel positions"),
    ("group 0", "shade", None): (INV, "group 0 (at least 1)"),
    ("5 rays in groups of 2", "shade", None): (INV, "5 rays are not a whole number of groups of 2"),
    ("other precision", "pick", 64): (UNS, F64_PICK % abi.RT_FP32),
    ("other precision", "pick", 32): (INV, F32_PICK % abi.RT_FP64),
    ("other precision", "shade", 64): (UNS, F64_SHADE % abi.RT_FP32),
    ("other precision", "shade", 32): (INV, F32_SHADE % abi.RT_FP64),
    ("other precision", "aov", 32): (UNS, F32_AOV % abi.RT_FP64),
    ("other precision", "aov", 64): (INV, F64_AOV),
    ("bad precision", "pick", 64): (INV, F64_PICK % BAD),
    ("bad precision", "pick", 32): (INV, F32_PICK % BAD),
    ("bad precision", "shade", 64): (INV, F64_SHADE % BAD),
    ("bad precision", "shade", 32): (INV, F32_SHADE % BAD),
    ("bad precision", "aov", None): (INV, "bad precision"),
    # the float64 radiance query names the precision before the missing rays, the float32 one after
    ("null origins, other precision", "shade", 64): (UNS, F64_SHADE % abi.RT_FP32),
    ("null origins, other precision", "shade", 32): (INV, NO_RAYS),
    ("image 0x4", "pick", None): (INV, "bad image size 0x4"),
    ("image 0x4", "aov", None): (INV, "bad image size 0x4"),
    ("misaligned hits", "trace", 32): (INV, "hits must be 16-byte aligned device memory"),
    ("misaligned hits", "pick", 32): (INV, "hits must be 16-byte aligned device memory"),
    ("rows before the image", "aov", None): (INV, "rows [-1, 8) outside [0, 8)"),
    ("rows past the image", "aov", None): (INV, "rows [0, 9) outside [0, 8)"),
    ("rows reversed", "aov", None): (INV, "rows [5, 3) outside [0, 8)"),
    ("every channel null", "aov", None): (INV, "no feature buffer requested: every channel is null"),
}


def _cases():
    out = []
    for name, (family, prec, roles) in ENTRY.items():
        for (case, fam, p), want in EXPECT.items():
            if fam != family or p not in (None, prec):
                continue
            if case == "misaligned hits" and "stream" not in roles.split():
                continue  # a host form stages the hits itself
            out.append(pytest.param(name, case, want, id=f"{name}-{case.replace(' ', '_')}"))
    return out


@pytest.fixture(scope="module")
def ds(gpu):
    """A single triangle and one box."""
    tri = TriangleMesh(np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), np.array([[0, 1, 2]], np.int32),
                       objectToWorld=translate(mat4(1.0), vec3(0.0, 0.0, -8.0)))
    box = initBox(vec3(-0.5, -0.5, -0.5), vec3(0.5, 0.5, 0.5), translate(mat4(1.0), vec3(2.0, 0.5, -8.0)))
    scene = Scene(objects=[Object("tri", tri, Material(albedo=vec3(0.8, 0.3, 0.2))),
                           Object("box", box, Material(albedo=vec3(0.2, 0.4, 0.8)))],
                  lights=scenes._warm_lights(), fov=50.0, cameraToWorld=scenes._std_camera(0.0, 1.0, 1.5),
                  bgColor=vec3(0.01, 0.03, 0.05))
    return DeviceScene(scene, device=0)


@pytest.fixture(scope="module")
def memory(gpu):
    """BYTES of host and of device memory per array role and per feature channel."""
    import torch
    names = ARRAYS + CHANNELS
    host = {k: np.zeros(BYTES, np.uint8) for k in names}
    dev = {k: torch.zeros(BYTES, dtype=torch.uint8, device="cuda:0") for k in names}
    return host, dev


def _call(ds, memory, name, change):
    """The entry point with a good call's arguments, `change` applied. Returns
    (return code, rt_last_error() text, Stats)."""
    family, prec, roles = ENTRY[name]
    roles = roles.split()
    device = "stream" in roles
    fn = getattr(lib(), name)
    host, dev = memory

    def addr(k):
        return int(dev[k].data_ptr()) if device else int(host[k].ctypes.data)

    own = abi.RT_FP64 if prec == 64 else abi.RT_FP32
    p = change.get("precision", own)
    if p == OTHER:
        p = abi.RT_FP32 if prec == 64 else abi.RT_FP64
    opts = abi.rt_options(width=change.get("width", W), height=change.get("height", H), precision=p)
    bufs = (abi.rt_aov_buffers64 if prec == 64 else abi.rt_aov_buffers)()
    for c in change.get("channels", CHANNELS):
        setattr(bufs, c, C.cast(C.c_void_p(addr(c)), dict(bufs._fields_)[c]))
    stats = abi.rt_stats(*([2 ** 64 - 1] * 5))
    good = {"scene": ds.h, "opts": C.byref(opts), "bufs": C.byref(bufs), "n": 4, "group": 1, "flags": 0, "y0": 0,
            "y1": H, "stream": None, "stats": C.byref(stats)}
    args = []
    for role, argtype in zip(roles, fn.argtypes):
        v = change.get(role, good.get(role))
        if role in ARRAYS:
            # rt_shade_rays_f32's one output is its "rgb"; tnear stays absent (it is optional)
            a = None if role == "tnear" or (role in change and change[role] is None) else addr(role)
            if change.get(role) == "+4":
                a += 4
            v = None if a is None else C.cast(C.c_void_p(a), argtype) if argtype is not C.c_void_p else C.c_void_p(a)
        args.append(v)
    rc = fn(*args)
    return rc, lib().rt_last_error().decode(), stats


@pytest.mark.parametrize("name,case,want", _cases())
def test_bad_call(ds, memory, name, case, want):
    rc, msg, _ = _call(ds, memory, name, CASES[case])
    assert (rc, msg) == want


@pytest.mark.parametrize("name", list(ENTRY))
def test_nothing_to_do(ds, memory, name):
    """No rays, or an empty row range: RT_OK, zero Stats, and no message — the
    last error stays the one an earlier call left."""
    assert lib().rt_trace_rays(ds.h, -77, None, None, None, 0, None, None, None) == INV
    left = lib().rt_last_error().decode()
    assert left == "negative ray count -77"
    empties = [{"y0": 3, "y1": 3}, {"y0": 0, "y1": 0}, {"y0": H, "y1": H}] if ENTRY[name][0] == "aov" else [{"n": 0}]
    for change in empties:
        rc, msg, st = _call(ds, memory, name, change)
        assert (rc, msg) == (abi.RT_OK, left), change
        assert [getattr(st, f) for f, _ in st._fields_] == [0] * 5, change
