"""rt_scene_set_objects: a scene whose objects were moved or restyled in place
equals a scene created with the new objects.

* the object records, world boxes, object light grids (the device builder,
  rt_objgrid_gpu.hip, against the host's build_object_light_grid) and scalar
  state equal what rt_scene_create forms, byte for byte
  (rtmi_test_objects_diff), and the mesh grids stay equal to the host's
  (rtmi_test_relight_diff);
* frames in both precisions, Stats, the rt_scene_last_* diagnostics and the
  float32 specialisation of a moved scene equal a fresh scene's;
* the float64 frame after a move is the oracle's, bit for bit;
* queries see the moved objects; edits of every kind commute;
* failures leave the scene as it was, earlier asynchronous calls keep their
  objects, repeated updates do not grow;
* the multi-rank form and the drop-in cache.
"""
import ctypes as C

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, scenes
from rtmi._lib import lib
from rtmi.abi import RT_BVH_PLOC
from rtmi.glm import Y_AXIS, degToRad, inverse, mat4, normalize, rotate, scale, translate, vec, vec3
from rtmi.renderer import DeviceScene, MultiDeviceScene, band_rows, deviceScene, invalidateScene, renderLine
from rtmi.scene import (Box, Material, Object, Scene, Sphere, TriangleMesh, flatten_objects, initBox, initPlane,
                        initSphere)
from test_gpu_relight import (BIAS, H, MOVED, W, _assert_same, _diff as _relight_diff, _distant, _lean_word,
                              _mesh_scene, _moved_camera, _point, _raw_distant, _small_torus)

pytestmark = pytest.mark.gpu

DIFF_NAMES = ["objects64", "fobj", "fobjx", "objbox", "grid-headers", "grid-masks", "off-grid", "scalars"]
GRID_DTYPE = np.dtype([("e1", "<f4", 3), ("u0", "<f4"), ("e2", "<f4", 3), ("v0", "<f4"), ("inv_h", "<f4"),
                       ("rmax", "<f4"), ("gu", "<i4"), ("gv", "<i4"), ("off_base", "<i4"), ("ent_base", "<i4"),
                       ("pad", "<i4", 2)])


def _objects_diff(ds):
    f = lib().rtmi_test_objects_diff
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 8)()
    assert f(ds.h, out) == 0, lib().rt_last_error()
    return dict(zip(DIFF_NAMES, [int(v) for v in out]))


def _object_grids(ds, nl):
    """(headers, masks, off_grid) of the scene's object light grids as they lie on the device."""
    f = lib().rtmi_test_object_grids
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64)]
    hdr = np.zeros(max(1, nl), GRID_DTYPE)
    assert GRID_DTYPE.itemsize == 64
    cap = nl * 256 * 256 + 1
    masks = np.zeros(cap, np.uint64)
    og = C.c_uint64()
    n = f(ds.h, hdr.ctypes.data, max(1, nl), masks.ctypes.data, cap, C.byref(og))
    assert 0 <= n <= cap, lib().rt_last_error()
    return hdr, masks[:n], int(og.value)


def _assert_no_diff(ds):
    d = _objects_diff(ds)
    assert d == dict.fromkeys(d, 0), d
    r = _relight_diff(ds)
    assert r == dict.fromkeys(r, 0), r


def _place(ob, m):
    ob.geometry.objectToWorld = np.asarray(m, np.float64)
    ob.geometry.worldToObject = inverse(ob.geometry.objectToWorld)


def _shift(ob, x, y, z):
    _place(ob, translate(ob.geometry.objectToWorld, vec3(x, y, z)))


# ---- 1. the builders -----------------------------------------------------------

LIGHT_SETS = {
    "distant": [_distant(-1.0, -1.2, -0.6)],
    "+x": [_raw_distant(1.0, 0.0, 0.0)],
    "-x": [_raw_distant(-1.0, 0.0, 0.0)],
    "-y": [_raw_distant(0.0, -1.0, 0.0)],
    "+z": [_raw_distant(0.0, 0.0, 1.0)],
    "diagonal": [_raw_distant(1.0, 1.0, 1.0)],
    "zero-direction": [_raw_distant(0.0, 0.0, 0.0), _distant(-1.0, -1.0, 0.2)],
    "point-between": [_distant(-1.0, -1.2, -0.6), _point(), _distant(2.0, -0.8, -1.3)],
}
OBLIQUE = normalize(vec(1.0, 2.0, -0.5))[:3]


def _analytic(objects):
    return Scene(objects=objects, lights=scenes._warm_lights(), fov=50.0,
                 cameraToWorld=scenes._std_camera(1.0, 5.5, 3.5), bgColor=vec3(0.01, 0.03, 0.05))


def _ball(x, y, z, r=1.0):
    return Object("ball", initSphere(r=r, objectToWorld=translate(mat4(1.0), vec3(x, y, z))),
                  Material(albedo=vec3(0.6, 0.5, 0.2)))


def _box(x, y, z, lo, hi):
    return Object("box", initBox(objectToWorld=translate(mat4(1.0), vec3(x, y, z)), vmin=vec(*lo), vmax=vec(*hi)),
                  Material(albedo=vec3(0.5)))


def _ground():
    return Object("ground", initPlane(objectToWorld=mat4(1.0)), Material(albedo=vec3(0.4)))


def _few(n):
    return _analytic([_ball(-4.0 + 3.0 * i, 1.0, -12.0 - i) for i in range(n - 1)] + [_ground()])


def _many(n):
    # small spheres on a plane; the plane comes first, so the last sphere is bit n - 1
    return _analytic([_ground()] + [_ball(-7.0 + 2.0 * (i % 8), 0.5, -8.0 - 2.0 * (i // 8), 0.5) for i in range(n - 1)])


def _planes_only():
    return _analytic([Object(f"p{k}", initPlane(objectToWorld=translate(mat4(1.0), vec3(0.0, -0.5 * k, 0.0))),
                             Material(albedo=vec3(0.4))) for k in range(4)])


def _row():
    # flat boxes of no thickness in z in a row along x: seen along -y (and along x) the grid is one row
    # of cells; their heights differ, so that seen along x their projections nest and do not coincide
    return _analytic([_box(-150.0 + 60.0 * i, 1.0, -20.0, (-2.0, -1.0 - 0.3 * i, 0.0), (2.0, 1.0 + 0.3 * i, 0.0))
                      for i in range(6)])


def _flat_boxes():
    return _analytic([_box(-3.0, 1.0, -12.0, (-1.0, 0.0, -1.0), (1.0, 0.0, 1.0)),   # vmin == vmax in y
                      _box(3.0, 2.0, -14.0, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),      # a point
                      _box(0.0, 0.0, -16.0, (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0)),
                      _ball(0.0, 4.0, -12.0), _ground()])


def _edit_boxes2(sc, k):
    boxes = [o for o in sc.objects if isinstance(o.geometry, Box)]
    _shift(boxes[1], 0.3 + 0.1 * k, 0.0, -0.2)
    _place(boxes[2], rotate(boxes[2].geometry.objectToWorld, OBLIQUE, degToRad(25.0 + 7.0 * k)))


def _edit_first(sc, k):
    _shift(sc.objects[0], 0.4 + 0.1 * k, 0.0, 0.3)


def _edit_last_ball(sc, k):
    balls = [o for o in sc.objects if isinstance(o.geometry, Sphere)]
    _shift(balls[-1], 0.25, 0.1 * (k + 1), -0.5)
    _shift(balls[0], -0.3, 0.0, 0.1 * k)


def _edit_row(sc, k):
    _shift(sc.objects[2], 1.0 + k, 0.0, 0.0)


def _edit_flat(sc, k):
    _shift(sc.objects[0], 0.1 * (k + 1), 0.0, 0.0)
    _shift(sc.objects[1], 0.0, 0.1, 0.05 * (k + 1))
    _place(sc.objects[2], rotate(sc.objects[2].geometry.objectToWorld, OBLIQUE, degToRad(10.0 * (k + 1))))


# name: (make, edit, object bins expected, more than one mask value expected)
BUILDER_CASES = {
    "boxes2": (scenes.boxes2, _edit_boxes2, True, True),
    "spheres-warm": (scenes.spheres_warm, _edit_last_ball, True, True),
    "four-objects": (lambda: _few(4), _edit_first, True, True),
    "three-objects": (lambda: _few(3), _edit_first, False, False),
    "64-objects": (lambda: _many(64), _edit_last_ball, True, True),
    "65-objects": (lambda: _many(65), _edit_last_ball, False, False),
    "planes-only": (_planes_only, _edit_first, True, False),
    "row": (_row, _edit_row, True, True),
    "flat-boxes": (_flat_boxes, _edit_flat, True, True),
}


@pytest.mark.parametrize("name", list(BUILDER_CASES))
def test_device_state_equals_what_create_forms(gpu, name):
    make, edit, bins, varied = BUILDER_CASES[name]
    sc = make()
    ds = DeviceScene(sc)
    one_row = bit63 = False
    for k, (lname, lights) in enumerate(LIGHT_SETS.items()):
        ds.set_lights(lights)
        edit(sc, k)
        ds.set_objects()
        d = _objects_diff(ds)
        print(name, lname, d)
        assert d == dict.fromkeys(d, 0), (lname, d)
        r = _relight_diff(ds)
        assert r == dict.fromkeys(r, 0), (lname, r)
        hdr, masks, off_grid = _object_grids(ds, len(lights))
        if not bins:
            assert masks.size == 0
            continue
        for li, light in enumerate(lights):
            g = hdr[li]
            has = hasattr(light, "dir") and float(np.abs(np.asarray(light.dir)[:3]).max()) > 0.0
            assert (int(g["gu"]) > 0) == has, (lname, li)
            if not has:
                continue
            cells = masks[int(g["off_base"]):int(g["off_base"]) + int(g["gu"]) * int(g["gv"])]
            assert cells.size == int(g["gu"]) * int(g["gv"])
            assert np.all(cells & np.uint64(off_grid) == np.uint64(off_grid))
            if varied:
                assert np.unique(cells).size > 1, (lname, li)
            else:
                assert cells.size == 1 and int(cells[0]) == off_grid
            one_row = one_row or int(g["gv"]) == 1 or int(g["gu"]) == 1
            bit63 = bit63 or bool(np.any(cells >> np.uint64(63)))
    if name == "row":
        assert one_row
    if name == "64-objects":
        assert bit63


# ---- 2. a moved scene equals a fresh one -----------------------------------------

def _opts(prec, m, w=W, h=H, depth=None):
    o = Options(width=w, height=h, antialias=Antialias(akGrid, m), bias=BIAS, precision=prec)
    if depth is not None:
        o.maxRayDepth = depth
    return o


def _subset(ds, o):
    f = lib().rtmi_test_f32_subset
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(abi.rt_options)]
    oc = o.to_c()
    return int(f(ds.h, C.byref(oc)))


def _last_batch(ds):
    a, b = C.c_int64(), C.c_int64()
    assert lib().rt_scene_last_batch(ds.h, C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def _render(ds, prec, m, w=W, h=H, depth=None):
    import torch
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    o = _opts(prec, m, w, h, depth)
    st = ds.render_device(o, fb)
    diag = (_lean_word(ds), ds.last_split(), ds.last_uniform(), ds.last_ground(), _last_batch(ds), _subset(ds, o))
    return fb.view(h, w, 3).cpu().numpy(), st, diag


def _both(ds, depth=None):
    """test_gpu_relight's pair of frames (fp32 m = 16, fp64 m = 8) with Stats
    and diagnostics, plus the batch counts and the float32 specialisation."""
    return _render(ds, Precision.fp32, 16, depth=depth), _render(ds, Precision.fp64, 8, depth=depth)


def _obj(sc, name):
    return next(o for o in sc.objects if o.name == name)


def _bunny_slide(sc):
    _shift(_obj(sc, "bunny"), 1.0, 0.0, 0.5)


def _bunny_lift(sc):
    _shift(_obj(sc, "bunny"), 0.0, 1.25, 0.0)


def _bunny_turn(sc):
    ob = _obj(sc, "bunny")
    _place(ob, scale(rotate(ob.geometry.objectToWorld, Y_AXIS, degToRad(35.0)), vec3(0.8, 0.8, 0.8)))


def _bunny_back(sc):
    _place(_obj(sc, "bunny"), translate(mat4(1.0), vec3(-0.5, 0.0001, -11.0)))


def _raise_ground(sc):
    _place(_obj(sc, "ground"), translate(mat4(1.0), vec3(0.0, 0.5, 0.0)))


def _boxes2_move(sc):
    ob = _obj(sc, "box3")
    _shift(ob, 0.0, 0.7, 0.4)
    ob.material.albedo = vec3(0.9, 0.2, 0.1)


def _ball_radius(sc):
    _obj(sc, "ball2").geometry.r = 2.75


def _ball_mirror(sc):
    _obj(sc, "ball2").material.reflection = 0.6


def _ball_matte(sc):
    _obj(sc, "ball2").material.reflection = 0.0


def _mix_move(sc):
    _shift(_obj(sc, "torus"), 0.6, 0.0, 0.4)
    _shift(_obj(sc, "ballD"), -0.5, 0.2, 0.0)
    _obj(sc, "boxC").material.albedo = vec3(0.2, 0.6, 0.9)


def _two_move(sc):
    _shift(_obj(sc, "torus1"), -0.5, 0.0, 0.5)
    ob = _obj(sc, "torus2")
    _place(ob, rotate(ob.geometry.objectToWorld, Y_AXIS, degToRad(20.0)))


# name: (make, the edits in turn, max_ray_depth or None)
MOVE_CASES = {
    "bunny-slide": (scenes.mesh_bunny, [_bunny_slide], None),
    "bunny-lift": (scenes.mesh_bunny, [_bunny_lift], None),
    "bunny-turn-and-back": (scenes.mesh_bunny, [_bunny_turn, _bunny_back], None),
    "ground-raised": (scenes.mesh_bunny, [_raise_ground], None),
    "boxes2": (scenes.boxes2, [_boxes2_move], None),
    "spheres-radius": (scenes.spheres_warm, [_ball_radius], None),
    "spheres-mirror-and-back": (scenes.spheres_warm, [_ball_mirror, _ball_matte], 3),
    "mesh-mix": (scenes.mesh_mix, [_mix_move], None),
    "two-meshes": (scenes.two_meshes, [_two_move], None),
}


@pytest.mark.parametrize("name", list(MOVE_CASES))
def test_moved_scene_equals_fresh_scene(gpu, name):
    make, edits, depth = MOVE_CASES[name]
    sc = make()
    # (either tree gives the same frames, Stats and diagnostics: the device builder spares the tests' time)
    warm, cold = DeviceScene(sc), DeviceScene(sc, bvh_builder=RT_BVH_PLOC)
    last = _both(warm, depth)  # the float64 shadow records and the launch orders of the old objects exist
    for edit in edits:
        edit(sc)
        warm.set_objects()
        cold.set_objects()
        want = _both(DeviceScene(sc, bvh_builder=RT_BVH_PLOC), depth)
        got = _both(warm, depth)
        _assert_same(got, want)
        _assert_same(_both(cold, depth), want)
        assert not np.array_equal(got[0][0], last[0][0])  # not a no-op
        _assert_no_diff(warm)
        last = got


def test_general_transform_changes_the_kernel(gpu):
    """A rotated and scaled bunny leaves the translation-only specialisation
    (SUB_XF_GENERAL) and returns to it."""
    sc = scenes.mesh_bunny()
    ds = DeviceScene(sc)
    o = _opts(Precision.fp32, 16)
    base = _subset(ds, o)
    _bunny_turn(sc)
    ds.set_objects()
    turned = _subset(ds, o)
    _bunny_back(sc)
    ds.set_objects()
    assert turned != base and _subset(ds, o) == base


# ---- 3. oracle --------------------------------------------------------------------

def _bunny_move_turn(sc):
    ob = _obj(sc, "bunny")
    _place(ob, rotate(translate(ob.geometry.objectToWorld, vec3(0.8, 0.0, 0.6)), Y_AXIS, degToRad(-30.0)))


@pytest.mark.parametrize("name", ["bunny", "boxes2"])
def test_moved_scene_equals_oracle(gpu, oracle_mod, name):
    """float64 bit-exact (frame rows and Stats), float32 within the bound of
    test_gpu_relight.py::test_relit_scene_equals_oracle, against the oracle
    rendering the edited scene."""
    make, edit = {"bunny": (scenes.mesh_bunny, _bunny_move_turn), "boxes2": (scenes.boxes2, _boxes2_move)}[name]
    w, h, rows = 96, 64, list(range(20, 52))
    sc = make()
    ds = DeviceScene(sc)
    _render(ds, Precision.fp64, 8, w, h)
    edit(sc)
    ds.set_objects()
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


# ---- 4. queries -------------------------------------------------------------------

def test_queries_follow_the_objects(gpu):
    sc = scenes.mesh_bunny()
    ds = DeviceScene(sc)
    rng = np.random.default_rng(5)
    n = 4096
    orig = np.tile(np.array([0.0, 5.5, 1.5]), (n, 1)) + rng.normal(0.0, 0.2, (n, 3))
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.6, 0.1, n), -np.ones(n)], axis=1)
    before = ds.trace_rays(orig, d, normals=True)
    _bunny_move_turn(sc)
    ds.set_objects()
    after = ds.trace_rays(orig, d, normals=True)
    want = DeviceScene(sc).trace_rays(orig, d, normals=True)
    for x, y in zip(after, want):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(before[0], after[0])
    assert np.count_nonzero(after[1] == 0) > n // 20  # the moved bunny is still in the rays' way


# ---- 5. order of edits ------------------------------------------------------------

def _torus_end_state(vertices, faces):
    sc = _mesh_scene(vertices, faces)
    _place(sc.objects[0], rotate(translate(mat4(1.0), vec3(0.7, 0.0001, -11.0)), Y_AXIS, degToRad(25.0)))
    sc.objects[1].material.albedo = vec3(0.3, 0.35, 0.5)
    sc.lights = list(MOVED)
    sc.cameraToWorld, sc.fov = _moved_camera(), 44.0
    return sc


@pytest.mark.parametrize("order", ["olmc", "cmlo"])
def test_edits_of_every_kind_commute(gpu, order):
    v, f = _small_torus()
    v2 = np.ascontiguousarray(v * np.array([1.1, 0.9, 1.05]) + np.array([0.0, 0.05, 0.0]))
    end = _torus_end_state(v2, f)
    ds = DeviceScene(_mesh_scene(v, f))
    _both(ds)
    for step in order:
        if step == "o":
            ds.set_objects(_same_meshes(ds, end))
        elif step == "l":
            ds.set_lights(MOVED)
        elif step == "m":
            ds.set_mesh_vertices(0, v2)
        else:
            ds.set_camera(_moved_camera(), 44.0)
        _render(ds, Precision.fp32, 16)
    _assert_no_diff(ds)
    _assert_same(_both(ds), _both(DeviceScene(end)))


def _same_meshes(ds, other):
    """other's objects with ds's own TriangleMesh objects in their place (an
    update keeps the meshes), placed and coloured as other's."""
    out = []
    for mine, theirs in zip(ds.scene.objects, other.objects):
        if isinstance(mine.geometry, TriangleMesh):
            mine.geometry.objectToWorld = theirs.geometry.objectToWorld
            mine.geometry.worldToObject = theirs.geometry.worldToObject
            out.append(Object(theirs.name, mine.geometry, theirs.material))
        else:
            out.append(theirs)
    return out


# ---- 6. failures keep the scene -----------------------------------------------------

def test_failures_keep_the_objects(gpu):
    sc = scenes.two_meshes()
    ds = DeviceScene(sc)
    before = _both(ds)
    info = ds.info()
    L = lib()
    n = len(sc.objects)

    def arr():
        return flatten_objects(sc.objects, ds._mesh_ids)[0]

    assert L.rt_scene_set_objects(ds.h, arr(), n - 1) == abi.RT_E_INVALID
    assert b"objects" in L.rt_last_error()
    a = arr()
    a[2].type = abi.RT_SPHERE
    assert L.rt_scene_set_objects(ds.h, a, n) == abi.RT_E_INVALID
    assert b"object 2" in L.rt_last_error()
    a = arr()
    a[1].mesh = 0
    assert L.rt_scene_set_objects(ds.h, a, n) == abi.RT_E_INVALID
    assert b"object 1" in L.rt_last_error()
    a = arr()
    a[1].mesh = 7
    assert L.rt_scene_set_objects(ds.h, a, n) == abi.RT_E_INVALID
    assert b"object 1" in L.rt_last_error()
    a = arr()
    a[0].object_to_world[3] = 0.25
    assert L.rt_scene_set_objects(ds.h, a, n) == abi.RT_E_UNSUPPORTED
    assert b"object 0" in L.rt_last_error()
    a = arr()
    a[2].world_to_object[15] = 2.0
    assert L.rt_scene_set_objects(ds.h, a, n) == abi.RT_E_UNSUPPORTED
    assert b"object 2" in L.rt_last_error()
    assert L.rt_scene_set_objects(ds.h, None, n) == abi.RT_E_INVALID
    assert L.rt_scene_set_objects(ds.h, arr(), -1) == abi.RT_E_INVALID
    with pytest.raises(ValueError):
        ds.set_objects(sc.objects[:-1])
    with pytest.raises(TypeError):
        ds.set_objects([sc.objects[0], sc.objects[1], _ball(0.0, 1.0, -9.0)])
    with pytest.raises(ValueError):  # an equal mesh that is not the scene's
        ds.set_objects(scenes.two_meshes().objects)
    _assert_same(_both(ds), before)
    assert ds.info() == info
    _assert_no_diff(ds)


# ---- 7. ordering ---------------------------------------------------------------------

def test_update_waits_for_asynchronous_calls(gpu):
    """An object update right after a render without Stats and a pipelined
    band sequence: those frames are the old objects', the next one the new."""
    import torch
    w, h, bh, world = 96, 54, 4, 3
    a_sc, b_sc, sc = scenes.mesh_bunny(), scenes.mesh_bunny(), scenes.mesh_bunny()
    _bunny_move_turn(b_sc)
    a_ds, b_ds = DeviceScene(a_sc), DeviceScene(b_sc)
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
    ds = DeviceScene(sc)
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ds.render_device(o, fb, stats=None)
    got_bands = bands(ds, None)
    _bunny_move_turn(sc)
    ds.set_objects()
    assert torch.equal(fb, ref_a)
    for g, r in zip(got_bands, ref_bands):
        assert torch.equal(g, r)
    ds.render_device(o, fb)
    assert torch.equal(fb, ref_b)
    assert not torch.equal(ref_a, ref_b)


# ---- 8. no growth ----------------------------------------------------------------------

@pytest.mark.parametrize("make, name", [(scenes.mesh_bunny, "bunny"), (scenes.boxes2, "box3")])
def test_repeated_updates_do_not_grow(gpu, make, name):
    sc = make()
    ds = DeviceScene(sc)
    _both(ds)
    home = _obj(sc, name).geometry.objectToWorld
    away = translate(home, vec3(0.6, 0.0, 0.3))
    for m in (away, home):
        _place(_obj(sc, name), m)
        ds.set_objects()
    size = ds.info()["device_bytes"]
    for k in range(50):
        _place(_obj(sc, name), away if k % 2 == 0 else home)
        ds.set_objects()
    assert ds.info()["device_bytes"] == size
    _assert_same(_both(ds), _both(DeviceScene(make())))


# ---- 9. multi-rank, 10. the drop-in cache ------------------------------------------------

def test_multi_rank_update_equals_single_device(gpu):
    w, h = 96, 54
    o = _opts(Precision.fp32, 16, w, h)
    sc = scenes.mesh_bunny()
    md = MultiDeviceScene(sc, (0, 0))
    fb = np.zeros((h, w, 3), np.float32)
    md.render_frame(o, fb)
    _bunny_move_turn(sc)
    md.set_objects(sc.objects)
    gst = md.render_frame(o, fb)
    ref = np.zeros((h, w, 3), np.float32)
    rst = DeviceScene(sc).render_lines(o, ref, 0, h)
    assert np.array_equal(fb, ref)
    assert gst == rst
    with pytest.raises(ValueError):
        md.set_objects(sc.objects[:1])
    md.close()


def test_dropin_cache_moves_objects_in_place(gpu, oracle_mod):
    sc = scenes.boxes2()
    o = _opts(Precision.fp64, 2, 72, 40)

    def frame():
        fb = np.zeros((40, 72, 3), np.float32)
        for y in range(40):
            renderLine(sc, o, fb, y)
        return fb

    try:
        first = frame()
        ds1 = deviceScene(sc)
        handle = ds1.h.value
        _boxes2_move(sc)
        _obj(sc, "ball").material.albedo = vec3(0.1, 0.7, 0.3)
        got = frame()
        ref, _, _ = oracle_mod.OracleScene(sc).render(o)
        assert np.array_equal(got, ref)
        assert not np.array_equal(got, first)
        assert deviceScene(sc) is ds1 and ds1.h.value == handle  # moved in place (rt_scene_set_objects)
        box = _obj(sc, "box5").geometry
        box.vmax = box.vmax + np.array([0.0, 0.35, 0.0])
        got = frame()
        ref, _, _ = oracle_mod.OracleScene(sc).render(o)
        assert np.array_equal(got, ref)
        assert deviceScene(sc) is not ds1  # a resized box still replaces the copy
    finally:
        invalidateScene(sc)
