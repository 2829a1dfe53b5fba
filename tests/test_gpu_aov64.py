"""Feature buffers of an RT_FP64 frame (DeviceScene.render_aovs_f64,
rt_render_aovs_f64*) on the device. The reference is rt_pick_pixels (the
float64 pick, test_gpu_query.py) at every sample position, reduced by the host
model (aov64_model.py, anchored to the oracle by test_aov64_model_cpu.py) —
never the kernel under test. The sums are defined in sample order, so every
channel has one correct bit pattern: every comparison here is of raw bytes,
and of the three Stats counts exactly. No tolerance appears anywhere.

1. Per sample, one lane per pixel: the 16 subset scenes (96 x 64) and the five
   coverage scenes (33 x 19) at akNone and akGrid m = 2, 3; on the coverage
   scenes also every stochastic kind at m = 3 and 5 with both seeds, at the
   positions of the oracle's sample tables.
2. Per sample, one pixel per wave: akGrid m = 8 (one full step of 64 lanes),
   9 (a partial second step) and 16 (four steps) at 33 x 19 (627 pixels: no
   multiple of a pixel batch).
3. Layouts and lists agree: flags 0, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING
   and both; 1 and 8 list slots per pixel.
4. The 32-bit wave counters across their flush intervals (1024 spp).
5. Rows, single channels, the host form. 6. After scene edits. 7. The scene's
   state around a call. 8. The error codes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import aov64_model as am
import coverage_scenes as cs
import subset_scenes as ss
from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi import abi
from rtmi._lib import RtmiError, lib
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import TriangleMesh, akMultiJittered

pytestmark = pytest.mark.gpu

CHANNELS = am.CHANNELS
BIAS = 1e-4
PER_LANE, NO_BINNING = abi.RT_FLAG_F64_PER_LANE, abi.RT_FLAG_NO_BINNING


def _np(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def opts(w, h, kind, m, flags=0, seed=0, precision=Precision.fp64):
    return Options(width=w, height=h, antialias=Antialias(kind, 1 if kind == akNone else m), bias=BIAS,
                   precision=precision, flags=flags, seed=seed)


def aovs(ds, o, **kw):
    """(dict of numpy arrays, Stats) of one call."""
    res, st = ds.render_aovs_f64(o, stats=True, **kw)
    return {k: _np(v) for k, v in res.items()}, st


def last_stats(ds):
    from rtmi.scene import Stats
    st = abi.rt_stats()
    assert lib().rt_scene_last_stats(ds.h, C.byref(st)) == 0
    return Stats.from_c(st)


def raw(res):
    return b"".join(res[c].tobytes() for c in CHANNELS if c in res)


def same(a, b):
    for c in CHANNELS:
        assert a[0][c].tobytes() == b[0][c].tobytes(), (c, np.argwhere(a[0][c] != b[0][c])[:8])
    assert a[1] == b[1], (a[1], b[1])


def reference(ds, scene, w, h, kind, m, seed=0):
    """The float64 picks at every sample position, reduced by the model."""
    xy = am.sample_positions(w, h, kind, m, seed)
    spp = xy.shape[2]
    t, obj, face, nrm, st = ds.pick(opts(w, h, akNone, 1), xy.reshape(-1, 2), normals=True, stats=True)
    shape = (h, w, spp)
    assert not nrm[obj < 0].any()
    ref = am.reduce_samples(t.reshape(shape), obj.reshape(shape), face.reshape(shape), nrm.reshape(shape + (3,)),
                            am.scene_albedo(scene))
    return ref, st, spp


def judge(got, st, ref, rst, what):
    for c in CHANNELS:
        assert got[c].dtype == ref[c].dtype and got[c].shape == ref[c].shape, (what, c)
        if got[c].tobytes() != ref[c].tobytes():
            bad = np.argwhere(got[c].view(np.int64 if got[c].itemsize == 8 else np.int32)
                              != ref[c].view(np.int64 if ref[c].itemsize == 8 else np.int32))
            raise AssertionError((what, c, [(tuple(int(v) for v in b), got[c][tuple(b)], ref[c][tuple(b)])
                                            for b in bad[:6]]))
    assert (st.numPrimaryRays, st.numIntersectionTests, st.numIntersectionHits) == (
        rst.numPrimaryRays, rst.numIntersectionTests, rst.numIntersectionHits), (what, st, rst)
    assert st.numShadowRays == 0 and st.numReflectionRays == 0
    # both hitting and missing pixels
    assert (got["alpha"] == 0).any() and (got["alpha"] > 0).any(), what
    assert np.isinf(got["depth"][got["alpha"] == 0]).all() and (got["object"][got["alpha"] == 0] == -1).all()


@functools.lru_cache(maxsize=None)
def subset_ds(bits):
    return DeviceScene(ss.subset_scene(bits))


@functools.lru_cache(maxsize=None)
def coverage_ds(name):
    return DeviceScene(cs.scene(name))


def check_case(ds, scene, w, h, kind, m, seed=0, flags=0, what=None):
    ref, rst, spp = reference(ds, scene, w, h, kind, m, seed)
    got, st = aovs(ds, opts(w, h, kind, m, flags, seed))
    assert st.numPrimaryRays == w * h * spp
    judge(got, st, ref, rst, what)
    return got, st


# ---- 1. per sample, one lane per pixel -----------------------------------------------------------
SAMPLINGS = ((akNone, 1), (akGrid, 2), (akGrid, 3))
# every stochastic kind at m = 3 and m = 5, both seeds with every kind
STOCHASTIC = tuple((kind, m, cs.SEEDS[(k + i) % 2]) for k, kind in enumerate(cs.STOCHASTIC)
                   for i, m in enumerate((3, 5)))


@pytest.mark.parametrize("bits", range(16), ids=[ss.subset_name(b) for b in range(16)])
def test_subset_scenes_against_the_picks(gpu, bits):
    ds = subset_ds(bits)
    for kind, m in SAMPLINGS:
        check_case(ds, ss.subset_scene(bits), ss.W, ss.H, kind, m, what=(ss.subset_name(bits), int(kind), m))


@pytest.mark.parametrize("name", cs.SCENES)
def test_coverage_scenes_against_the_picks(gpu, name):
    ds = coverage_ds(name)
    for kind, m in SAMPLINGS:
        check_case(ds, cs.scene(name), cs.W, cs.H, kind, m, what=(name, int(kind), m))


@pytest.mark.parametrize("kind,m,seed", STOCHASTIC, ids=[f"k{int(k)}-m{m}-s{cs.SEEDS.index(s)}" for k, m, s in STOCHASTIC])
@pytest.mark.parametrize("name", cs.SCENES)
def test_stochastic_samplers_against_the_picks(gpu, name, kind, m, seed):
    check_case(coverage_ds(name), cs.scene(name), cs.W, cs.H, kind, m, seed, what=(name, int(kind), m, seed))


# ---- 2. per sample, one pixel per wave -----------------------------------------------------------
PX_M = (8, 9, 16)
PX_BITS = (ss.SPHERE | ss.BOX | ss.MESH, ss.MESH | ss.XF_GENERAL)


@pytest.mark.parametrize("m", PX_M)
@pytest.mark.parametrize("name", cs.SCENES)
def test_coverage_scenes_one_pixel_per_wave(gpu, name, m):
    check_case(coverage_ds(name), cs.scene(name), cs.W, cs.H, akGrid, m, what=(name, m))


@pytest.mark.parametrize("m", PX_M)
@pytest.mark.parametrize("bits", PX_BITS, ids=[ss.subset_name(b) for b in PX_BITS])
def test_subset_scenes_one_pixel_per_wave(gpu, bits, m):
    check_case(subset_ds(bits), ss.subset_scene(bits), cs.W, cs.H, akGrid, m, what=(ss.subset_name(bits), m))


# ---- 3. layouts and lists agree ------------------------------------------------------------------
def _slot_lg(ds, lg=-1):
    f = lib().rtmi_test_slot_lg
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32]
    r = f(ds.h, lg)
    assert r >= 0
    return r


def _list_lengths(ds, w, h):
    info = np.zeros(w * h, np.uint32)
    f = lib().rtmi_test_pixel_info
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(ds.h, info.ctypes.data_as(C.c_void_p)) == 0
    return (info & 0x00FFFFFF).astype(np.int64)


@pytest.mark.parametrize("m", PX_M)
@pytest.mark.parametrize("which", ["torus", "slats_ground"])
def test_layouts_and_lists_give_the_same_bytes(gpu, which, m):
    scene = ss.subset_scene(ss.MESH) if which == "torus" else cs.scene(which)
    ds, w, h = DeviceScene(scene), cs.W, cs.H
    try:
        want = check_case(ds, scene, w, h, akGrid, m, what=(which, m))
        listed = _list_lengths(ds, w, h)
        assert listed.max() >= 2  # the call built lists, and some hold more than one face
        assert (listed == 0).any()  # and records that rule the mesh out
        for flags in (PER_LANE, NO_BINNING, PER_LANE | NO_BINNING):
            same(aovs(ds, opts(w, h, akGrid, m, flags)), want)
        default = _slot_lg(ds)
        try:
            for lg in (0, 3):
                _slot_lg(ds, lg)
                same(aovs(ds, opts(w, h, akGrid, m)), want)
                over = _list_lengths(ds, w, h) > (1 << lg)
                print(which, m, "slots", 1 << lg, "lists past their slots", int(over.sum()))
                if lg == 0:
                    assert over.any()  # some list really overflowed: those pixels took the BVH
                same(aovs(ds, opts(w, h, akGrid, m, PER_LANE)), want)
        finally:
            _slot_lg(ds, default)
        same(aovs(ds, opts(w, h, akGrid, m)), want)
    finally:
        ds.close()


# ---- 4. counter flush ----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, PER_LANE], ids=["px", "lane"])
def test_stats_across_the_flush_intervals(gpu, flags):
    """1024 samples per pixel: 16 steps of 64 lanes per pixel in one layout,
    1024 samples in one lane in the other — past every flush interval."""
    ds = coverage_ds("blocks")
    w, h, m = 8, 4, 32
    ref, rst, spp = reference(ds, cs.scene("blocks"), w, h, akGrid, m)
    got, st = aovs(ds, opts(w, h, akGrid, m, flags))
    assert spp == 1024 and st.numPrimaryRays == w * h * spp
    judge(got, st, ref, rst, ("blocks", m, flags))


# ---- 5. rows, channels, the host form ------------------------------------------------------------
def _sentinels(w, h, host):
    import torch
    out = {}
    for c in CHANNELS:
        shape = (h, w, 3) if c in ("normal", "albedo") else (h, w)
        a = np.full(shape, -77, np.int32 if c in ("object", "face") else np.float64)
        out[c] = a if host else torch.from_numpy(a).cuda()
    return out


@pytest.mark.parametrize("kind,m", [(akGrid, 2), (akGrid, 8)], ids=["grid2", "grid8"])
def test_rows_channels_and_host_form(gpu, kind, m):
    ds = subset_ds(ss.SPHERE | ss.MESH)
    w, h = ss.W, ss.H
    o = opts(w, h, kind, m)
    whole = aovs(ds, o)
    assert all(whole[0][c].dtype == (np.int32 if c in ("object", "face") else np.float64) for c in CHANNELS)
    for host in (False, True):
        part = aovs(ds, o, y0=5, y1=14, out=_sentinels(w, h, host))
        assert part[1].numPrimaryRays == 9 * w * m * m
        for c in CHANNELS:
            assert part[0][c][5:14].tobytes() == whole[0][c][5:14].tobytes(), (host, c)
            rest = np.concatenate([part[0][c][:5], part[0][c][14:]])
            assert (rest == -77).all(), (host, c)
    same(aovs(ds, o, host=True), whole)
    for c in CHANNELS:
        one = aovs(ds, o, channels=(c,), out={c: _sentinels(w, h, False)[c]})
        assert list(one[0]) == [c] and one[0][c].tobytes() == whole[0][c].tobytes(), c
        assert one[1] == whole[1]
    # y0 == y1: nothing is launched, nothing written, the last call stays the last call
    last = last_stats(ds)
    for host in (False, True):
        none = aovs(ds, o, y0=7, y1=7, out=_sentinels(w, h, host))
        assert none[1].numPrimaryRays == 0 and all((none[0][c] == -77).all() for c in CHANNELS)
    assert last_stats(ds) == last


# ---- 6. after edits ------------------------------------------------------------------------------
def test_after_edits(gpu):
    bits = ss.SPHERE | ss.MESH
    edited = ss.subset_scene(bits)
    ds = DeviceScene(edited)
    cases = [opts(ss.W, ss.H, akGrid, 2), opts(ss.W, ss.H, akGrid, 8)]

    def check():
        other = DeviceScene(edited)
        try:
            fresh = [aovs(other, o) for o in cases]
        finally:
            other.close()
        mine = [aovs(ds, o) for o in cases]
        for a, b in zip(mine, fresh):
            same(a, b)
        return mine

    before = check()
    cam = np.array(edited.cameraToWorld, np.float64)
    cam[3, :3] += (0.4, 0.3, -0.5)
    edited.cameraToWorld = cam
    ds.set_camera(cam, edited.fov)
    moved_cam = check()
    assert raw(moved_cam[0][0]) != raw(before[0][0])
    # the lights are not read: a relight changes no byte
    from rtmi.glm import normalize, vec, vec3
    from rtmi.scene import DistantLight
    edited.lights = [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=2.0, dir=normalize(vec(1.0, -1.0, -0.2)))]
    ds.set_lights(edited.lights)
    relit = check()
    for a, b in zip(relit, moved_cam):
        same(a, b)
    # the second sphere moves and changes colour
    moved = ss.subset_scene(bits, dcam=0.0)
    ball = moved.objects[1]
    ball.geometry.objectToWorld = ss._xf(False, -1.6, 1.1, -8.5)
    ball.geometry.worldToObject = ss.inverse(ball.geometry.objectToWorld)
    ball.material.albedo = ss.vec3(0.1, 0.2, 0.7)
    edited.objects[1] = ball
    ds.set_objects(edited.objects)
    restyled = check()
    assert not np.array_equal(restyled[0][0]["albedo"], moved_cam[0][0]["albedo"])
    assert not np.array_equal(restyled[0][0]["depth"], moved_cam[0][0]["depth"])
    mesh = next(ob.geometry for ob in edited.objects if isinstance(ob.geometry, TriangleMesh))
    v = mesh.vertices.copy()
    v[:, 1] = v[:, 1] * (1.0 + 0.25 * np.sin(2.0 * v[:, 0]))  # the torus, unevenly taller
    mesh.vertices = np.ascontiguousarray(v)
    ds.set_mesh_vertices(0, mesh.vertices)
    deformed = check()
    assert not np.array_equal(deformed[0][0]["normal"], restyled[0][0]["normal"])
    ds.close()


# ---- 7. scene state ------------------------------------------------------------------------------
def _diag(ds):
    return ds.last_split(), ds.last_lean_kernel(), ds.last_batch()


def test_colour_renders_are_the_same_before_and_after(gpu):
    import torch
    from rtmi import scenes
    ds = DeviceScene(scenes.mesh_bunny())
    w, h = 128, 72
    o32 = opts(w, h, akGrid, 16, precision=Precision.fp32)  # one pixel per wave: a two-class launch
    o64 = opts(w, h, akGrid, 8)  # one pixel per wave in float64, with this call's lists

    def colour(o):
        fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        st = ds.render_device(o, fb)
        return fb.cpu().numpy().tobytes(), st, _diag(ds)

    first = colour(o32), colour(o64)
    assert first[0][2][0][0] > 0 and first[0][2][0][1] > 0  # lean and general pixels: two classes
    for oa in (o64, opts(w, h, akGrid, 2), opts(w, h, akMultiJittered, 3, seed=cs.SEEDS[0])):
        got, st = aovs(ds, oa)
        spp = oa.antialias.gridSize ** 2
        assert last_stats(ds) == st and st.numPrimaryRays == w * h * spp and st.numShadowRays == 0
        assert ds.last_split() == (0, ds.last_split()[1]) and ds.last_lean_kernel() == 0  # nothing classified
        assert (got["object"] == 0).any() and (got["object"] == 1).any() and (got["object"] == -1).any()
        assert (colour(o32), colour(o64)) == first
    got, st_aov = aovs(ds, o64)

    # three pipelined band calls, a feature-buffer call between the first and the second
    world, band_h = 3, 4
    rows = band_rows(h, band_h, world)

    def bands(with_aov):
        out = []
        for r in range(world):
            fb = torch.zeros(rows * w * 3, dtype=torch.float32, device="cuda")
            st = ds.render_bands_device(o32, fb, band_h, r, world)
            assert ds.last_pipelined()
            out.append((fb.cpu().numpy().tobytes(), st, _diag(ds)))
            if with_aov and r == 0:
                mid = aovs(ds, o64)
                assert raw(mid[0]) == raw(got) and mid[1] == st_aov
        return out

    assert bands(True) == bands(False)
    ds.close()


# ---- 8. errors -----------------------------------------------------------------------------------
def test_errors_leave_the_scene_usable(gpu):
    ds = subset_ds(ss.SPHERE | ss.MESH)
    w, h = ss.W, ss.H
    want = aovs(ds, opts(w, h, akGrid, 2))

    def code(o, call=None, **kw):
        with pytest.raises(RtmiError) as e:
            (call or ds.render_aovs_f64)(o, **kw)
        same(aovs(ds, opts(w, h, akGrid, 2)), want)  # the scene still answers as before
        return e.value

    err = code(opts(w, h, akGrid, 2, precision=Precision.fp32))
    assert err.code == abi.RT_E_INVALID and "rt_render_aovs " in str(err) + " "
    # the sampler limits are a float64 render's: no (multi-)jittered limit of 32, grid_size in [1, 256]
    got, st = aovs(ds, opts(16, 8, akMultiJittered, 33, seed=cs.SEEDS[0]), channels=("alpha",))
    assert st.numPrimaryRays == 16 * 8 * 33 * 33
    assert code(opts(w, h, akGrid, 257)).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 0)).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y0=-1).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y1=h + 1).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y0=9, y1=8).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), channels=()).code == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), channels=(), host=True).code == abi.RT_E_INVALID
    ds.render_aovs_f64(opts(w, h, akGrid, 2), channels=(), y0=3, y1=3)  # no rows: no channel is needed
    # the float32 call still refuses an RT_FP64 frame
    assert code(opts(w, h, akGrid, 2), call=ds.render_aovs).code == abi.RT_E_UNSUPPORTED
    same(aovs(ds, opts(w, h, akGrid, 2)), want)
