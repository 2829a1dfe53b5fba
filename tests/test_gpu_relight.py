"""rt_scene_set_lights: a scene relit in place equals a scene created with the
new lights.

* the device-built light grids, records and prefix sums (rt_lights_gpu.hip)
  equal the host builders' arrays byte for byte, entry order included
  (rtmi_test_relight_diff), on the bunny, a torus and hand-made meshes that
  reach the builder's corners;
* frames in both precisions, Stats and the rt_scene_last_* diagnostics of a
  relit scene equal a fresh scene's, over the transitions a front end makes;
* the float64 frame after a relight is the oracle's, bit for bit;
* the next call's pixel records cross the device-built prefix sums with the
  host's skip proof;
* failures leave the scene as it was, earlier asynchronous calls keep their
  lights, queries do not change, repeated relights do not grow;
* the multi-rank form and the drop-in cache.
"""
import ctypes as C

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, scenes
from rtmi._lib import lib
from rtmi.abi import RT_FLAG_NO_REORDER
from rtmi.glm import X_AXIS, Y_AXIS, degToRad, mat4, normalize, point, rotate, translate, vec, vec3
from rtmi.renderer import DeviceScene, MultiDeviceScene, band_rows, deviceScene, invalidateScene, renderLine
from rtmi.scene import DistantLight, PointLight, TriangleMesh

pytestmark = pytest.mark.gpu

BIAS = 1e-4
W, H = 64, 36


def _distant(x, y, z, intensity=2.0, color=(1.0, 1.0, 1.0)):
    return DistantLight(color=vec3(*color), intensity=intensity, dir=normalize(vec(x, y, z)))


def _raw_distant(x, y, z):
    return DistantLight(color=vec3(1.0), intensity=2.0, dir=vec(x, y, z))


def _point():
    return PointLight(color=vec3(1.0, 0.9, 0.8), intensity=4000.0, pos=point(0.5, 14.0, -12.0))


def _warm():
    return scenes._warm_lights()


MOVED = [_distant(-1.0, -1.2, -0.6, 4.0), _distant(2.0, -0.8, -1.3, 1.0, (0.8, 0.3, 0.0))]
THREE = [_distant(-2.0, -0.8, -0.3, 4.0), _distant(2.0, -0.8, -1.3, 1.0), _distant(0.2, -1.0, 0.9, 0.5)]
BELOW = [_distant(0.3, 0.8, -0.2)]


def _diff(ds):
    f = lib().rtmi_test_relight_diff
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 8)()
    assert f(ds.h, out) == 0, lib().rt_last_error()
    return dict(zip(["headers", "off", "ent", "sat", "lrec", "grec", "flight", "dlight"], [int(v) for v in out]))


def _mesh_scene(vertices, faces):
    mesh = TriangleMesh(np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(faces, np.int32), None,
                        mat4(1.0))
    return scenes._mesh_scene(mesh, "m", (0.6, 0.9, 0.2))


def _tris(v):
    """(n, 3, 3) vertex triples -> (vertices, faces)."""
    v = np.asarray(v, np.float64)
    return v.reshape(-1, 3), np.arange(v.shape[0] * 3, dtype=np.int32).reshape(-1, 3)


# a triangle in the plane y = y0 that faces a light shining down (0, -1, 0):
# its winding makes (v1 - v0) x (v2 - v0) point down
def _up_tri(x, z, s, y0=1.0):
    return [[x, y0, z], [x + s, y0, z], [x, y0, z + s]]


def _single(flip):
    t = _up_tri(0.0, 0.0, 1.5)
    return _tris([t[::-1] if flip else t])


def _patch(flip):
    ts = [_up_tri(0.3 * i, 0.3 * j, 0.25, 1.0 + 0.01 * (i + j)) for i in range(7) for j in range(7)]
    return _tris([t[::-1] if flip else t for t in ts])


def _stack():
    # 300 equal triangles stacked along the light: every cell inside their
    # common projection holds 300 entries of equal coverage (ties by leaf index)
    return _tris([_up_tri(0.0, 0.0, 2.0, 1.0 + 0.01 * k) for k in range(300)])


def _span():
    # one triangle over the whole grid above 2,000 small ones (the pair dealing)
    small = [_up_tri(0.1 * i, 0.1 * j, 0.08, 1.0) for i in range(50) for j in range(40)]
    return _tris([_up_tri(-0.2, -0.2, 11.0, 2.0)] + small)


def _small_torus():
    m = scenes.torus_mesh(24, 12)
    return m.vertices, m.faces


DOWN = [_raw_distant(0.0, -1.0, 0.0)]
BUILDER_CASES = {
    "bunny": (scenes.mesh_bunny, MOVED),
    "bunny-3": (scenes.mesh_bunny, THREE),
    "torus": (lambda: scenes.torus_scene(U=200, V=100), MOVED),
    "single": (lambda: _mesh_scene(*_single(False)), DOWN),
    "single-flipped": (lambda: _mesh_scene(*_single(True)), DOWN),
    "patch": (lambda: _mesh_scene(*_patch(False)), DOWN),
    "patch-turned-away": (lambda: _mesh_scene(*_patch(True)), DOWN),
    "axis+x": (lambda: _mesh_scene(*_small_torus()), [_raw_distant(1.0, 0.0, 0.0)]),
    "axis-y": (lambda: _mesh_scene(*_small_torus()), [_raw_distant(0.0, -1.0, 0.0)]),
    "axis+z": (lambda: _mesh_scene(*_small_torus()), [_raw_distant(0.0, 0.0, 1.0)]),
    "diagonal": (lambda: _mesh_scene(*_small_torus()), [_raw_distant(1.0, 1.0, 1.0)]),
    "zero-direction": (lambda: _mesh_scene(*_small_torus()), [_raw_distant(0.0, 0.0, 0.0), _distant(-1.0, -1.0, 0.2)]),
    "point-and-distant": (lambda: _mesh_scene(*_small_torus()), [_point(), _distant(-1.0, -1.0, 0.2)]),
    "stack-300": (lambda: _mesh_scene(*_stack()), DOWN),
    "span": (lambda: _mesh_scene(*_span()), DOWN),
    "mesh-mix": (scenes.mesh_mix, MOVED),
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_device_build_equals_host_builders(gpu, name):
    make, lights = BUILDER_CASES[name]
    ds = DeviceScene(make())
    ds.set_lights(lights)
    d = _diff(ds)
    print(name, d)
    assert d == dict.fromkeys(d, 0), d
    assert ds.info()["num_lights"] == len(lights)


def _opts(prec, m, w=W, h=H, flags=0):
    return Options(width=w, height=h, antialias=Antialias(akGrid, m), bias=BIAS, precision=prec, flags=flags)


def _lean_word(ds):
    k = C.c_int32()
    assert lib().rt_scene_last_lean_kernel(ds.h, C.byref(k)) == 0
    return int(k.value)


def _render(ds, prec, m, w=W, h=H):
    import torch
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(_opts(prec, m, w, h), fb)
    diag = (_lean_word(ds), ds.last_split(), ds.last_uniform(), ds.last_ground())
    return fb.view(h, w, 3).cpu().numpy(), st, diag


def _both(ds):
    """The one-plane float32 kernels' frame (m = 16) and the float64
    one-pixel-per-wave frame (m = 8), each with Stats and diagnostics."""
    return _render(ds, Precision.fp32, 16), _render(ds, Precision.fp64, 8)


def _assert_same(got, want):
    for (gf, gs, gd), (wf, ws, wd), prec in zip(got, want, ("fp32", "fp64")):
        assert np.array_equal(gf, wf), (prec, int(np.count_nonzero(gf != wf)))
        assert gs == ws, (prec, gs, ws)
        assert gd == wd, (prec, gd, wd)


def _with_lights(make, lights):
    sc = make()
    sc.lights = list(lights)
    return sc


BUNNY_TRANSITIONS = {
    "moved": (None, MOVED),
    "2-to-1": (None, MOVED[:1]),
    "1-to-3": (MOVED[:1], THREE),
    "distant-to-point": (None, [_point()]),
    "point-to-distant": ([_point()], MOVED),
    "from-below": (None, BELOW),
    "none": (None, []),
    "none-to-2": ([], MOVED),
}


@pytest.mark.parametrize("name", list(BUNNY_TRANSITIONS))
def test_relit_bunny_equals_fresh_scene(gpu, name):
    a, b = BUNNY_TRANSITIONS[name]
    a = _warm() if a is None else a
    ds = DeviceScene(_with_lights(scenes.mesh_bunny, a))
    _both(ds)  # the float64 shadow records and the launch orders of A exist
    ds.set_lights(b)
    fresh = DeviceScene(_with_lights(scenes.mesh_bunny, b))
    _assert_same(_both(ds), _both(fresh))
    assert ds.info()["num_lights"] == len(b)


OTHER_SCENES = {
    "boxes2": (scenes.boxes2, [_distant(-3.0, -1.5, -2.0, 0.7), _distant(1.0, -0.4, 0.5, 0.3)]),
    "spheres-warm": (scenes.spheres_warm, [_distant(1.0, -2.0, -0.5, 3.0)]),
    "spheres-warm-point": (scenes.spheres_warm, [_point(), _distant(1.0, -2.0, -0.5, 3.0)]),
    "mesh-mix": (scenes.mesh_mix, MOVED),
    "mesh-mix-point": (scenes.mesh_mix, [_point()]),
    "two-meshes": (scenes.two_meshes, THREE),
}


@pytest.mark.parametrize("name", list(OTHER_SCENES))
def test_relit_scene_equals_fresh_scene(gpu, name):
    make, b = OTHER_SCENES[name]
    ds = DeviceScene(make())
    _both(ds)
    ds.set_lights(b)
    fresh = DeviceScene(_with_lights(make, b))
    _assert_same(_both(ds), _both(fresh))


def _moved_camera():
    return translate(rotate(rotate(mat4(1.0), Y_AXIS, degToRad(14.0)), X_AXIS, degToRad(-9.0)), vec3(1.2, 3.9, 4.0))


def test_camera_moves_between_relights(gpu):
    ds = DeviceScene(scenes.mesh_bunny())
    _both(ds)
    ds.set_lights(MOVED)
    ds.set_camera(_moved_camera(), 44.0)
    _both(ds)
    ds.set_lights(BELOW + MOVED[:1])
    sc = _with_lights(scenes.mesh_bunny, BELOW + MOVED[:1])
    sc.cameraToWorld, sc.fov = _moved_camera(), 44.0
    _assert_same(_both(ds), _both(DeviceScene(sc)))


def test_relit_scene_equals_oracle(gpu, oracle_mod):
    """float64 bit-exact (frame rows and Stats), float32 within
    test_gpu_parity's tolerance, against the oracle rendering lights B."""
    w, h, rows = 96, 64, list(range(20, 52))
    ds = DeviceScene(scenes.mesh_bunny())
    _render(ds, Precision.fp64, 8, w, h)
    ds.set_lights(MOVED)
    sc = _with_lights(scenes.mesh_bunny, MOVED)
    o = oracle_mod.OracleScene(sc)
    ref = np.zeros((h, w, 3), np.float32)
    _, rst, _ = o.render(_opts(Precision.fp64, 8, w, h), rows=rows, fb=ref)
    got = np.zeros((h, w, 3), np.float32)
    gst = ds.render_lines(_opts(Precision.fp64, 8, w, h), got, rows[0], rows[-1] + 1)
    assert np.array_equal(got[rows], ref[rows])
    assert gst == rst, (gst, rst)
    got32 = np.zeros((h, w, 3), np.float32)
    ds.render_lines(_opts(Precision.fp32, 8, w, h), got32, rows[0], rows[-1] + 1)
    err = np.abs(got32[rows].astype(np.float64) - ref[rows].astype(np.float64)).max(axis=2)
    print("fp32 share within 2e-3:", (err <= 2e-3).mean(), "mean abs err:", err.mean())
    assert (err <= 2e-3).mean() >= 0.995 and err.mean() <= 2e-4


# ---- the per-call records after a relight (helpers as in test_gpu_frame.py) --

def _device_lists(ds, w, h):
    L = lib()
    f = L.rtmi_test_frame_lists
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    off = np.zeros(w * h + 1, dtype=np.int32)
    info = np.zeros(w * h, dtype=np.uint32)
    cap = 1 << 22
    ent = np.zeros(cap, dtype=np.int32)
    n = f(ds.h, off.ctypes.data, ent.ctypes.data, cap, info.ctypes.data)
    assert n >= 0, L.rt_last_error()
    return off, ent, info


def _host_lists(ds, w, h, bias=BIAS):
    L = lib()
    f = L.rtmi_test_host_lists
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    off = np.zeros(w * h + 1, dtype=np.int32)
    info = np.zeros(w * h, dtype=np.uint32)
    cap = 1 << 22
    ent = np.zeros(cap, dtype=np.int32)
    n = f(ds.h, w, h, bias, off.ctypes.data, ent.ctypes.data, cap, info.ctypes.data)
    assert 0 <= n <= cap
    return off, ent, info


@pytest.mark.parametrize("lights", [MOVED, BELOW + MOVED[:1], THREE], ids=["moved", "below+1", "three"])
def test_pixel_records_after_relight(gpu, lights):
    """The skip bits of the call after a relight (the device-built prefix
    sums) equal the host builders' (the host's own prefix sums)."""
    import torch
    w, h = 160, 90
    ds = DeviceScene(scenes.mesh_bunny())
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ds.render_device(_opts(Precision.fp32, 16, w, h, RT_FLAG_NO_REORDER), fb)
    ds.set_lights(lights)
    ds.render_device(_opts(Precision.fp32, 16, w, h, RT_FLAG_NO_REORDER), fb)
    d_off, _, d_info = _device_lists(ds, w, h)
    h_off, _, h_info = _host_lists(ds, w, h)
    assert np.array_equal(d_off, h_off)
    assert np.array_equal(d_info, h_info), int(np.count_nonzero(d_info != h_info))
    skipped = int(np.count_nonzero(h_info >> 24))
    print("pixels with skip bits:", skipped)
    assert skipped > w * h // 4


# ---- failure and ordering ----------------------------------------------------

def test_bad_light_type_keeps_the_lights(gpu):
    ds = DeviceScene(scenes.mesh_bunny())
    before = _both(ds)
    arr = (abi.rt_light_desc * 2)()
    arr[0].type = abi.RT_DISTANT_LIGHT
    arr[0].dir = (C.c_double * 3)(0.0, -1.0, 0.0)
    arr[1].type = 7
    L = lib()
    assert L.rt_scene_set_lights(ds.h, arr, 2) == abi.RT_E_INVALID
    assert b"light 1" in L.rt_last_error()
    assert L.rt_scene_set_lights(ds.h, arr, -1) == abi.RT_E_INVALID
    assert L.rt_scene_set_lights(ds.h, None, 1) == abi.RT_E_INVALID
    _assert_same(_both(ds), before)
    assert ds.info()["num_lights"] == 2
    class Lamp:  # neither a DistantLight nor a PointLight
        color, intensity = vec3(1.0), 1.0

    with pytest.raises(TypeError):
        ds.set_lights([Lamp()])
    _assert_same(_both(ds), before)


def test_relight_waits_for_asynchronous_calls(gpu):
    """A relight right after a render without Stats and a pipelined band
    sequence: those frames are A's, the next one B's."""
    import torch
    w, h, bh, world = 96, 54, 4, 3
    a_ds = DeviceScene(scenes.mesh_bunny())
    b_ds = DeviceScene(_with_lights(scenes.mesh_bunny, MOVED))
    o = _opts(Precision.fp32, 16, w, h)
    rows = band_rows(h, bh, world)

    def bands(ds, stats):
        bufs = [torch.zeros(rows * w * 3, dtype=torch.float32, device="cuda") for _ in range(world)]
        for r in range(world):
            ds.render_bands_device(o, bufs[r], bh, r, world, stats=stats)
        return bufs

    ref_a, ref_b = torch.zeros(w * h * 3, device="cuda"), torch.zeros(w * h * 3, device="cuda")
    a_ds.render_device(o, ref_a)
    b_ds.render_device(o, ref_b)
    ref_bands = bands(a_ds, True)
    ds = DeviceScene(scenes.mesh_bunny())
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ds.render_device(o, fb, stats=None)
    got_bands = bands(ds, None)
    ds.set_lights(MOVED)
    assert torch.equal(fb, ref_a)
    for g, r in zip(got_bands, ref_bands):
        assert torch.equal(g, r)
    ds.render_device(o, fb)
    assert torch.equal(fb, ref_b)
    assert not torch.equal(ref_a, ref_b)


def test_queries_do_not_depend_on_the_lights(gpu):
    ds = DeviceScene(scenes.mesh_bunny())
    rng = np.random.default_rng(5)
    n = 4096
    orig = np.tile(np.array([0.0, 5.5, 1.5]), (n, 1)) + rng.normal(0.0, 0.2, (n, 3))
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.6, 0.1, n), -np.ones(n)], axis=1)
    before = ds.trace_rays(orig, d)
    ds.set_lights(BELOW)
    after = ds.trace_rays(orig, d)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.count_nonzero(before[1] >= 0) > n // 4


def test_repeated_relights_do_not_grow(gpu):
    ds = DeviceScene(scenes.mesh_bunny())
    _both(ds)
    a = _warm()
    ds.set_lights(MOVED)
    ds.set_lights(a)
    size = ds.info()["device_bytes"]
    for k in range(50):
        ds.set_lights(MOVED if k % 2 == 0 else a)
    assert ds.info()["device_bytes"] == size
    _assert_same(_both(ds), _both(DeviceScene(scenes.mesh_bunny())))


# ---- multi-rank, drop-in cache ------------------------------------------------

def test_multi_rank_relight_equals_single_device(gpu):
    w, h = 96, 54
    o = _opts(Precision.fp32, 16, w, h)
    md = MultiDeviceScene(scenes.mesh_bunny(), (0, 0))
    fb = np.zeros((h, w, 3), np.float32)
    md.render_frame(o, fb)
    md.set_lights(MOVED)
    gst = md.render_frame(o, fb)
    ref = np.zeros((h, w, 3), np.float32)
    rst = DeviceScene(_with_lights(scenes.mesh_bunny, MOVED)).render_lines(o, ref, 0, h)
    assert np.array_equal(fb, ref)
    assert gst == rst
    md.close()


def test_dropin_cache_relights_in_place(gpu, oracle_mod):
    sc = scenes.boxes2()
    o = _opts(Precision.fp64, 2, 72, 40)

    def frame():
        fb = np.zeros((40, 72, 3), np.float32)
        for y in range(40):
            renderLine(sc, o, fb, y)
        return fb

    try:
        frame()
        ds1 = deviceScene(sc)
        sc.lights = [_distant(-3.0, -1.5, -2.0, 0.7), _point()]
        got = frame()
        ref, _, _ = oracle_mod.OracleScene(sc).render(o)
        assert np.array_equal(got, ref)
        assert deviceScene(sc) is ds1  # a lights-only edit keeps the device scene (rt_scene_set_lights)
        from rtmi.scene import Box
        box = next(ob.geometry for ob in sc.objects if isinstance(ob.geometry, Box))
        box.vmax = box.vmax + np.array([0.0, 0.35, 0.0])
        got = frame()
        ref, _, _ = oracle_mod.OracleScene(sc).render(o)
        assert np.array_equal(got, ref)
        assert deviceScene(sc) is not ds1  # a resized box still replaces it
    finally:
        invalidateScene(sc)
