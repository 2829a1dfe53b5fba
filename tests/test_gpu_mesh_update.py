"""rt_scene_set_mesh_vertices: a scene whose mesh was deformed in place equals
a scene created from the deformed mesh.

* the device-resident arrays (records, normals, binned faces, node boxes of
  both trees, mesh / object records, object boxes) equal the host create path
  plus a host refit of the scene's topology, byte for byte
  (rtmi_test_mesh_update_diff), and the rebuilt light grids equal the host
  builders' (rtmi_test_relight_diff);
* frames in both precisions, Stats, rt_scene_last_split and
  rt_scene_last_lean_kernel equal a fresh scene's for both BVH builders, and
  the float64 frame and Stats are the oracle's;
* queries, orderings against set_lights / set_camera / asynchronous and
  pipelined calls, failures that leave the scene as it was, memory, the device
  form, the multi-rank form and the drop-in cache.
"""
import ctypes as C

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, scenes
from rtmi._lib import lib
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH
from rtmi.glm import X_AXIS, Y_AXIS, degToRad, mat4, normalize, rotate, translate, vec, vec3
from rtmi.renderer import (DeviceScene, MultiDeviceScene, band_rows, deviceScene, invalidateScene, renderLine,
                           updateMesh)
from rtmi.renderer import _cache
from rtmi.scene import DistantLight, TriangleMesh

from bvh_corpus import coincident as _coincident, flat_grid as _flat_grid, soup as _soup

pytestmark = pytest.mark.gpu

BIAS = 1e-4
DIFF_NAMES = ["trifast", "trif64", "n32", "n64", "bins", "boxes64", "boxes32", "children", "devmesh32", "devmesh64",
              "fmesh", "fobj", "objbox", "meshbox", "r14", "r15"]
RELIGHT_NAMES = ["headers", "off", "ent", "sat", "lrec", "grec", "flight", "dlight"]


# ---- meshes (tests/bvh_corpus.py) -----------------------------------------------

def _scene(mesh):
    return scenes._mesh_scene(mesh, "m", (0.7, 0.6, 0.5))


MESHES = {
    "one": lambda: _soup(1, 1),
    "five": lambda: _soup(5, 4),  # the first size with an inner node (leaves hold at most 4 faces)
    "soup300": lambda: _soup(300, 5),
    "coincident": _coincident,
    "grid": _flat_grid,
    "torus": lambda: scenes.torus_mesh(48, 24),
}


# ---- deformations ---------------------------------------------------------------

def _identity(v):
    return v.copy()


def _translation(v):
    return v + np.array([0.7, 0.4, -0.9])


def _twist(v, k=0.6):
    a = k * v[:, 1]
    out = v.copy()
    out[:, 0] = np.cos(a) * v[:, 0] + np.sin(a) * v[:, 2]
    out[:, 2] = -np.sin(a) * v[:, 0] + np.cos(a) * v[:, 2]
    return out


def _scramble(v):
    return v[np.random.default_rng(9).permutation(len(v))].copy()


def _collapse(v):
    return np.tile(np.array([0.3, 1.2, -0.4]), (len(v), 1))


def _around_camera(v):
    """The mesh's AABB holds the camera (world (0, 5.5, 1.5); the mesh object
    sits at translate(0, 1e-4, -12)): the reference's AABB gate hides it."""
    c = 0.5 * (v.min(0) + v.max(0))
    return v - c + np.array([0.0, 5.5, 13.5])


def _signed_zero(v):
    """The x extreme is +0.0 at a lower vertex index and -0.0 at a higher one
    (and the other way round on z): calcAABB keeps the first."""
    out = v.copy()
    out[:, 0] = -np.abs(out[:, 0]) - 0.01
    out[:, 2] = np.abs(out[:, 2]) + 0.01
    n = len(out)
    out[n // 3, 0], out[2 * n // 3, 0] = 0.0, -0.0
    out[n // 3, 2], out[2 * n // 3, 2] = -0.0, 0.0
    return out


DEFORM = {"identity": _identity, "translation": _translation, "twist": _twist, "scramble": _scramble,
          "x1000": lambda v: 1000.0 * v, "x0.001": lambda v: 0.001 * v, "collapse": _collapse,
          "around-camera": _around_camera, "signed-zero": _signed_zero}

PAIRS = [("one", "identity"), ("one", "translation"), ("one", "collapse"),
         ("five", "identity"), ("five", "twist"), ("five", "signed-zero"),
         ("soup300", "scramble"), ("soup300", "x1000"), ("soup300", "x0.001"), ("soup300", "twist"),
         ("coincident", "translation"), ("coincident", "collapse"),
         ("grid", "twist"), ("grid", "translation"),
         ("torus", "identity"), ("torus", "translation"), ("torus", "twist"), ("torus", "scramble"),
         ("torus", "x1000"), ("torus", "x0.001"), ("torus", "collapse"), ("torus", "around-camera"),
         ("torus", "signed-zero")]


# ---- hooks and renders ----------------------------------------------------------

def _mesh_diff(ds):
    f = lib().rtmi_test_mesh_update_diff
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 16)()
    assert f(ds.h, out) == 0, lib().rt_last_error()
    return dict(zip(DIFF_NAMES, [int(x) for x in out]))


def _relight_diff(ds):
    f = lib().rtmi_test_relight_diff
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 8)()
    assert f(ds.h, out) == 0, lib().rt_last_error()
    return dict(zip(RELIGHT_NAMES, [int(x) for x in out]))


def _hashes(ds, mesh=0):
    f = lib().rtmi_test_mesh_hash
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    assert f(ds.h, mesh, out) == 0, lib().rt_last_error()
    return [int(x) for x in out]


def _assert_no_diff(ds):
    d, r = _mesh_diff(ds), _relight_diff(ds)
    assert d == dict.fromkeys(d, 0), d
    assert r == dict.fromkeys(r, 0), r


def _opts(prec, kind, m, w, h, flags=0):
    return Options(width=w, height=h, antialias=Antialias(kind, m), bias=BIAS, precision=prec, flags=flags)


O64 = _opts(Precision.fp64, akNone, 1, 96, 72)
O32 = _opts(Precision.fp32, akGrid, 2, 160, 120)
# the one-plane kernels' option sets (tests/test_gpu_relight.py)
P32 = _opts(Precision.fp32, akGrid, 16, 64, 36)
P64 = _opts(Precision.fp64, akGrid, 8, 64, 36)


def _lean_word(ds):
    k = C.c_int32()
    assert lib().rt_scene_last_lean_kernel(ds.h, C.byref(k)) == 0
    return int(k.value)


def _render(ds, o):
    import torch
    fb = torch.zeros(o.width * o.height * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb)
    return fb, st, (ds.last_split(), _lean_word(ds))


def _all(ds, sets=(O64, O32)):
    return [_render(ds, o) for o in sets]


def _assert_same(got, want):
    import torch
    for k, ((gf, gs, gd), (wf, ws, wd)) in enumerate(zip(got, want)):
        assert torch.equal(gf, wf), (k, int((gf != wf).sum()))
        assert gs == ws, (k, gs, ws)
        assert gd == wd, (k, gd, wd)


def _meshes_of(sc):
    out = []
    for o in sc.objects:
        if isinstance(o.geometry, TriangleMesh) and not any(o.geometry is g for g in out):
            out.append(o.geometry)
    return out


def _deformed(make, mesh, fn):
    """make()'s scene with mesh number `mesh` deformed by fn."""
    sc = make()
    g = _meshes_of(sc)[mesh]
    g.vertices = np.ascontiguousarray(fn(g.vertices))
    return sc


def _oracle_check(oracle_mod, sc, got, o=O64):
    ref, rst, _ = oracle_mod.OracleScene(sc).render(o)
    fb, st, _ = got
    assert np.array_equal(fb.view(o.height, o.width, 3).cpu().numpy(), ref)
    assert st == rst, (st, rst)


# ---- 1. every mesh / deformation pair --------------------------------------------

@pytest.mark.parametrize("mesh,deform", PAIRS, ids=[f"{m}-{d}" for m, d in PAIRS])
def test_updated_scene_equals_fresh_scene(gpu, oracle_mod, mesh, deform):
    make = lambda: _scene(MESHES[mesh]())  # noqa: E731
    sets = (O64, O32, P32, P64) if mesh == "torus" else (O64, O32)
    b = _deformed(make, 0, DEFORM[deform])
    new_v = _meshes_of(b)[0].vertices
    want = None
    for builder in (RT_BVH_SAH, RT_BVH_PLOC):
        ds = DeviceScene(make(), bvh_builder=builder)
        _all(ds, sets)  # the float64 shadow records and the launch orders of A exist
        before = _hashes(ds)
        ds.set_mesh_vertices(0, new_v)
        _assert_no_diff(ds)
        if deform == "identity":
            assert _hashes(ds) == before
        got = _all(ds, sets)
        if want is None:
            want = _all(DeviceScene(b, bvh_builder=RT_BVH_PLOC), sets)
            _oracle_check(oracle_mod, b, got[0])
        _assert_same(got, want)
        _assert_same(_all(DeviceScene(b, bvh_builder=RT_BVH_SAH), sets[:2]), want[:2])
        ds.close()


def test_around_camera_moves_the_gate(gpu):
    """The updated box holds the camera: the reference's AABB gate
    (geom.nim:340) now decides differently for the camera rays, exactly as in
    a scene created there (the pair test above checks the frames against the
    oracle; this one the picks, which read the float64 DevMesh box)."""
    ds = DeviceScene(_scene(MESHES["torus"]()))
    xy = np.stack(np.meshgrid(np.arange(64.0), np.arange(36.0)), -1).reshape(-1, 2)
    before = ds.pick(P64, xy)
    b = _deformed(lambda: _scene(MESHES["torus"]()), 0, _around_camera)
    ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    got, want = ds.pick(P64, xy), DeviceScene(b).pick(P64, xy)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    print("pixels on the mesh before / after:", int(np.count_nonzero(before[1] == 0)),
          int(np.count_nonzero(got[1] == 0)))
    assert np.count_nonzero(before[1] == 0) > 0


@pytest.mark.parametrize("make", [scenes.mesh_mix, scenes.two_meshes], ids=["mesh_mix", "two_meshes"])
def test_scenes_with_other_objects(gpu, oracle_mod, make):
    """mesh_mix: 6 objects, so the object bins and object light grids follow
    the mesh's box; two_meshes: each mesh alone, the other's arrays untouched."""
    nm = len(_meshes_of(make()))
    for m in range(nm):
        ds = DeviceScene(make())
        _all(ds)
        others = {k: _hashes(ds, k)[:6] for k in range(nm) if k != m}
        b = _deformed(make, m, _twist)
        ds.set_mesh_vertices(m, _meshes_of(b)[m].vertices)
        _assert_no_diff(ds)
        for k, h in others.items():
            assert _hashes(ds, k)[:6] == h, k
        got = _all(ds)
        _assert_same(got, _all(DeviceScene(b, bvh_builder=RT_BVH_PLOC)))
        _oracle_check(oracle_mod, b, got[0])
        # by the TriangleMesh object too
        ds2 = DeviceScene(sc2 := make())
        ds2.set_mesh_vertices(_meshes_of(sc2)[m], _meshes_of(b)[m].vertices)
        _assert_same(_all(ds2), got)


def test_caller_normals(gpu, oracle_mod):
    """Caller-supplied normals are copied and rounded; NULL recomputes."""
    make = lambda: _scene(MESHES["torus"]())  # noqa: E731
    b = _deformed(make, 0, _twist)
    g = _meshes_of(b)[0]
    rng = np.random.default_rng(2)
    nrm = rng.normal(0.0, 1.0, (len(g.faces), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    g.normals = np.ascontiguousarray(nrm)
    ds = DeviceScene(make())
    ds.set_mesh_vertices(0, g.vertices, g.normals)
    _assert_no_diff(ds)
    got = _all(ds)
    _assert_same(got, _all(DeviceScene(b)))
    _oracle_check(oracle_mod, b, got[0])
    g.normals = None
    ds.set_mesh_vertices(0, g.vertices)
    _assert_no_diff(ds)
    _assert_same(_all(ds), _all(DeviceScene(b)))


def test_bunny_twist(gpu, oracle_mod):
    make = scenes.mesh_bunny
    b = _deformed(make, 0, lambda v: _twist(v, 0.15))
    o32 = _opts(Precision.fp32, akGrid, 4, 320, 180)
    o64 = _opts(Precision.fp64, akGrid, 2, 48, 32)
    ds = DeviceScene(make())
    _all(ds, (o32, o64))
    ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    _assert_no_diff(ds)
    got = _all(ds, (o32, o64))
    _assert_same(got, _all(DeviceScene(b, bvh_builder=RT_BVH_PLOC), (o32, o64)))
    _oracle_check(oracle_mod, b, got[1], o64)


# ---- 2. queries -------------------------------------------------------------------

def test_queries_after_an_update(gpu, oracle_mod):
    make = lambda: _scene(MESHES["torus"]())  # noqa: E731
    b = _deformed(make, 0, _twist)
    ds = DeviceScene(make())
    rng = np.random.default_rng(21)
    n = 2000
    orig = np.array([0.0, 2.0, -12.0]) + rng.uniform(-9.0, 9.0, (n, 3))
    d = np.array([0.0, 2.0, -12.0]) + rng.uniform(-4.0, 4.0, (n, 3)) - orig
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xy = np.stack(np.meshgrid(np.arange(64.0), np.arange(36.0)), -1).reshape(-1, 2)
    ds.trace_rays(orig, d)  # the query buffers exist before the update
    ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    fresh = DeviceScene(b, bvh_builder=RT_BVH_PLOC)
    got = ds.trace_rays(orig, d, normals=True)
    want = fresh.trace_rays(orig, d, normals=True)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(ds.pick(P64, xy, normals=True), fresh.pick(P64, xy, normals=True)):
        assert x.tobytes() == y.tobytes()
    osc = oracle_mod.OracleScene(b)
    t, obj, face = got[:3]
    assert np.count_nonzero(obj == 0) > n // 20
    for i in range(n):
        ob, ot, tri, _ = osc.trace(np.append(orig[i], 1.0), np.append(d[i], 0.0))
        assert ob == obj[i], i
        if ob >= 0:
            assert np.float64(ot).tobytes() == t[i].tobytes() and (tri == face[i] or ob != 0), i


# ---- 3. ordering -----------------------------------------------------------------

MOVED = [DistantLight(color=vec3(1.0), intensity=4.0, dir=normalize(vec(-1.0, -1.2, -0.6))),
         DistantLight(color=vec3(0.8, 0.3, 0.0), intensity=1.0, dir=normalize(vec(2.0, -0.8, -1.3)))]


def _moved_camera():
    return translate(rotate(rotate(mat4(1.0), Y_AXIS, degToRad(14.0)), X_AXIS, degToRad(-9.0)), vec3(1.2, 3.9, 4.0))


@pytest.mark.parametrize("order", ["mlc", "lmc", "clm", "mcl"])
def test_update_with_relight_and_camera_in_any_order(gpu, order):
    make = lambda: _scene(MESHES["torus"]())  # noqa: E731
    b = _deformed(make, 0, _twist)
    b.lights = list(MOVED)
    b.cameraToWorld, b.fov = _moved_camera(), 44.0
    ds = DeviceScene(make())
    sets = (O64, O32, P32, P64)
    _all(ds, sets)
    for step in order:
        if step == "m":
            ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
        elif step == "l":
            ds.set_lights(MOVED)
        else:
            ds.set_camera(_moved_camera(), 44.0)
        _render(ds, P32)
    _assert_no_diff(ds)
    _assert_same(_all(ds, sets), _all(DeviceScene(b), sets))


def test_update_waits_for_asynchronous_and_pipelined_calls(gpu):
    """An update right after a render without Stats and a pipelined band
    sequence (a third of the image each): those frames show the old geometry,
    the next ones the new."""
    import torch
    w, h, bh, world = 96, 54, 4, 4
    make = lambda: _scene(MESHES["torus"]())  # noqa: E731
    b = _deformed(make, 0, _twist)
    a_ds, b_ds = DeviceScene(make()), DeviceScene(b)
    o = _opts(Precision.fp32, akGrid, 16, w, h)
    rows = band_rows(h, bh, world)

    def bands(ds, stats):
        bufs = [torch.zeros(rows * w * 3, dtype=torch.float32, device="cuda") for _ in range(world)]
        for r in range(world):
            ds.render_bands_device(o, bufs[r], bh, r, world, stats=stats)
        return bufs

    ref_a, ref_b = torch.zeros(w * h * 3, device="cuda"), torch.zeros(w * h * 3, device="cuda")
    a_ds.render_device(o, ref_a)
    b_ds.render_device(o, ref_b)
    bands_a, bands_b = bands(a_ds, True), bands(b_ds, True)
    ds = DeviceScene(make())
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ds.render_device(o, fb, stats=None)
    got = bands(ds, None)
    assert ds.last_pipelined()
    ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    assert torch.equal(fb, ref_a)
    for g, r in zip(got, bands_a):
        assert torch.equal(g, r)
    got = bands(ds, None)
    ds.render_device(o, fb)
    assert torch.equal(fb, ref_b)
    for g, r in zip(got, bands_b):
        assert torch.equal(g, r)
    assert not torch.equal(ref_a, ref_b)


# ---- 4. failures -----------------------------------------------------------------

def test_failures_keep_the_geometry(gpu):
    L = lib()
    sc = _scene(MESHES["soup300"]())
    g = _meshes_of(sc)[0]
    # vertex 3 * 300 is referenced by no face
    g.vertices = np.ascontiguousarray(np.concatenate([g.vertices, [[0.0, 1.0, 0.0]]]))
    ds = DeviceScene(sc)
    before, hashes = _all(ds), _hashes(ds)
    v = g.vertices.copy()
    nv = len(v)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def unchanged():
        assert _hashes(ds) == hashes
        _assert_same(_all(ds), before)

    bad = _twist(v)
    bad[17, 2] = np.nan
    assert L.rt_scene_set_mesh_vertices(ds.h, 0, dp(bad), nv, None) == abi.RT_E_INVALID
    assert b"non-finite" in L.rt_last_error()
    unchanged()
    bad[17, 2] = np.inf
    assert L.rt_scene_set_mesh_vertices(ds.h, 0, dp(bad), nv, None) == abi.RT_E_INVALID
    unchanged()
    assert L.rt_scene_set_mesh_vertices(ds.h, 0, dp(v), nv - 1, None) == abi.RT_E_INVALID
    assert L.rt_scene_set_mesh_vertices(ds.h, 0, dp(v), nv + 1, None) == abi.RT_E_INVALID
    assert L.rt_scene_set_mesh_vertices(ds.h, -1, dp(v), nv, None) == abi.RT_E_INVALID
    assert L.rt_scene_set_mesh_vertices(ds.h, 1, dp(v), nv, None) == abi.RT_E_INVALID
    assert b"out of range" in L.rt_last_error()
    assert L.rt_scene_set_mesh_vertices(ds.h, 0, None, nv, None) == abi.RT_E_INVALID
    assert b"null" in L.rt_last_error()
    assert L.rt_scene_set_mesh_vertices_device(ds.h, 0, None, nv, None, None) == abi.RT_E_INVALID
    unchanged()
    # a NaN in the unreferenced vertex is accepted and matches a fresh create
    ok = _twist(v)
    ok[nv - 1, 0] = np.nan
    ds.set_mesh_vertices(0, ok)
    _assert_no_diff(ds)
    sc_b = _scene(TriangleMesh(ok, g.faces))
    _assert_same(_all(ds), _all(DeviceScene(sc_b)))


def test_mesh_without_faces_is_accepted(gpu):
    """A mesh of 0 faces: RT_OK, nothing launched, the frames stay."""
    sc = _scene(TriangleMesh(np.array([[0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 2.0, 0.0]]),
                             np.zeros((0, 3), np.int32)))
    ds = DeviceScene(sc)
    before, hashes = _all(ds), _hashes(ds)
    ds.set_mesh_vertices(0, np.array([[5.0, 1.0, 0.0], [6.0, 1.0, 0.0], [5.0, 2.0, 0.0]]))
    assert _hashes(ds) == hashes
    _assert_same(_all(ds), before)
    assert lib().rt_scene_set_mesh_vertices(ds.h, 0, None, 3, None) == abi.RT_E_INVALID


# ---- 5. memory, the device form, multi-rank, the drop-in cache --------------------

def test_repeated_updates_do_not_grow(gpu):
    import torch
    sc = _scene(MESHES["torus"]())
    v = _meshes_of(sc)[0].vertices
    # once through, so that the kernels' code and the runtime's own pools are resident
    ds = DeviceScene(sc)
    ds.set_mesh_vertices(0, _twist(v, 0.2))
    ds.close()
    torch.cuda.synchronize()
    start = torch.cuda.mem_get_info()[0]
    ds = DeviceScene(sc)
    ds.set_mesh_vertices(0, _twist(v, 0.1))
    size, free = ds.info()["device_bytes"], torch.cuda.mem_get_info()[0]
    for k in range(20):  # (the light grids' sizes follow the geometry: end where the sizes were taken)
        ds.set_mesh_vertices(0, _twist(v, 0.05 * k if k % 2 == 0 else 0.1))
    assert ds.info()["device_bytes"] == size
    assert torch.cuda.mem_get_info()[0] == free
    ds.close()
    assert torch.cuda.mem_get_info()[0] == start


def test_device_form_equals_host_form(gpu):
    import torch
    sc = _scene(MESHES["torus"]())
    v = _meshes_of(sc)[0].vertices
    host, dev = DeviceScene(sc), DeviceScene(sc)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_v = torch.from_numpy(v).cuda()
        moved = (d_v * 1.25 + torch.tensor([0.5, 0.25, -0.75], dtype=torch.float64, device="cuda")).contiguous()
        dev.set_mesh_vertices(0, moved, stream=stream)
    host.set_mesh_vertices(0, moved.cpu().numpy())
    assert _hashes(dev) == _hashes(host)
    _assert_no_diff(dev)
    _assert_same(_all(dev), _all(host))
    with pytest.raises(ValueError):
        dev.set_mesh_vertices(0, moved.float())


def test_multi_rank_update_equals_single_device(gpu):
    w, h = 96, 54
    make = lambda: _scene(MESHES["torus"]())  # noqa: E731
    b = _deformed(make, 0, _twist)
    o = _opts(Precision.fp32, akGrid, 16, w, h)
    md = MultiDeviceScene(make(), (0, 0))
    fb = np.zeros((h, w, 3), np.float32)
    md.render_frame(o, fb)
    md.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    gst = md.render_frame(o, fb)
    ref = np.zeros((h, w, 3), np.float32)
    ds = DeviceScene(make())
    ds.set_mesh_vertices(0, _meshes_of(b)[0].vertices)
    rst = ds.render_lines(o, ref, 0, h)
    assert np.array_equal(fb, ref)
    assert gst == rst
    md.close()


def test_dropin_cache_updates_in_place(gpu, oracle_mod):
    sc = _scene(MESHES["torus"]())
    g = _meshes_of(sc)[0]
    o = _opts(Precision.fp64, akGrid, 2, 72, 40)

    def frame():
        fb = np.zeros((40, 72, 3), np.float32)
        for y in range(40):
            renderLine(sc, o, fb, y)
        return fb

    try:
        updateMesh(sc, g)  # no device copy yet: nothing to push
        first = frame()
        ds1, handle, n = deviceScene(sc), deviceScene(sc).h.value, len(_cache)
        g.vertices[:] = _twist(g.vertices)  # in place
        updateMesh(sc, g)
        got = frame()
        ref, _, _ = oracle_mod.OracleScene(sc).render(o)
        assert np.array_equal(got, ref)
        assert not np.array_equal(got, first)
        assert deviceScene(sc) is ds1 and ds1.h.value == handle and len(_cache) == n
    finally:
        invalidateScene(sc)
