"""Feature buffers of an RT_FP32 frame (DeviceScene.render_aovs,
rt_render_aovs*) on the device. The reference is rt_pick_pixels_f32 (the
separately verified float32 pick, test_gpu_trace32.py) at every sample
position, reduced on the host — never the kernel under test.

1. Per sample: the 16 geometry subset scenes at 96 x 64 and the five coverage
   scenes at 33 x 19, akNone and akGrid m = 2, 4 (m = 8 on three scenes), whose
   sample positions are exact in float32. alpha, depth, object and face equal
   the reduced picks exactly; normal and albedo exactly at akNone, and
   otherwise within
       (spp + 3) * 2^-24 * mean(|x_i|)
   of the float64 mean of the picks' values (x_i = 0 for a sample that
   misses): the float32 summation bound gamma_(n-1) * sum(|x_i|) of any order
   of n = spp additions, plus one rounding of inv_len, one of the product and
   one to spare, all relative to sum(|x_i|) / spp. Derived, not measured.
2. The sample positions of every sampler: on the coverage scenes (black
   objects, sky 1) round(alpha * spp) is the hit count the RT_FP32 frame of
   the same options encodes, on every pixel.
3. The per-pixel lists against the BVH: all six channels and the Stats
   byte-identical with flags 0, RT_FLAG_NO_BINNING and lists past their slots.
4. Rows, NULL channels, the host form. 5. After scene edits. 6. The scene's
   state around a call. 7. The error codes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import coverage_scenes as cs
import subset_scenes as ss
from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi import abi
from rtmi._lib import RtmiError, lib
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import TriangleMesh, akMultiJittered

pytestmark = pytest.mark.gpu

CHANNELS = ("alpha", "depth", "object", "face", "normal", "albedo")
BIAS = 1e-4
U = 2.0 ** -24


def _np(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def opts(w, h, kind, m, flags=0, seed=0, precision=Precision.fp32):
    return Options(width=w, height=h, antialias=Antialias(kind, 1 if kind == akNone else m), bias=BIAS,
                   precision=precision, flags=flags, seed=seed)


def aovs(ds, o, **kw):
    """(dict of numpy arrays, Stats) of one call."""
    res, st = ds.render_aovs(o, stats=True, **kw)
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
        assert np.array_equal(a[0][c], b[0][c]), (c, np.argwhere(a[0][c] != b[0][c])[:8])
    assert raw(a[0]) == raw(b[0])
    assert a[1] == b[1], (a[1], b[1])


def sample_xy(w, h, kind, m):
    """(h, w, spp, 2) float32: the image positions of every akNone / akGrid
    sample, sample s = sj * m + si, exact in float32."""
    sx, sy = cs.pixel_offsets(kind, m, 0, 0, 0)
    xy = np.empty((h, w, len(sx), 2), np.float64)
    xy[..., 0] = np.arange(w, dtype=np.float64)[None, :, None] + sx[None, None, :]
    xy[..., 1] = np.arange(h, dtype=np.float64)[:, None, None] + sy[None, None, :]
    xy32 = xy.astype(np.float32)
    assert np.array_equal(xy32.astype(np.float64), xy)
    return xy32


def albedo32(scene):
    return np.array([[np.float32(c) for c in ob.material.albedo] for ob in scene.objects], np.float32)


def reference(ds, scene, w, h, kind, m):
    """The picks at every sample position, reduced per pixel on the host."""
    xy = sample_xy(w, h, kind, m)
    spp = xy.shape[2]
    t, obj, face, nrm, st = ds.pick_f32(opts(w, h, akNone, 1), xy.reshape(-1, 2), normals=True, stats=True)
    t, obj, face = t.reshape(h, w, spp), obj.reshape(h, w, spp), face.reshape(h, w, spp)
    nrm = nrm.reshape(h, w, spp, 3)
    hit = obj >= 0
    hits = hit.sum(axis=2)
    inv_len = np.float32(1.0 / float(spp))
    ref = {"alpha": hits.astype(np.float32) * inv_len}
    tk = np.where(hit, t, np.float32(np.inf))
    win = np.argmin(tk, axis=2)  # the first smallest: the lowest sample index on equal t
    ref["depth"] = np.take_along_axis(tk, win[..., None], 2)[..., 0]
    any_hit = hits > 0
    ref["object"] = np.where(any_hit, np.take_along_axis(obj, win[..., None], 2)[..., 0], -1).astype(np.int32)
    ref["face"] = np.where(any_hit, np.take_along_axis(face, win[..., None], 2)[..., 0], -1).astype(np.int32)
    alb = np.where(hit[..., None], albedo32(scene)[np.maximum(obj, 0)], np.float32(0.0))
    ref["normal_samples"] = nrm
    ref["albedo_samples"] = alb
    assert not nrm[~hit].any()
    return ref, st, spp


def judge(got, st, ref, rst, spp, what):
    for c in ("alpha", "depth", "object", "face"):
        bad = np.argwhere(got[c] != ref[c])
        assert bad.size == 0, (what, c, [(int(x), int(y), got[c][y, x], ref[c][y, x]) for y, x in bad[:6]])
    for c in ("normal", "albedo"):
        x = ref[c + "_samples"].astype(np.float64)
        if spp == 1:
            assert np.array_equal(got[c], ref[c + "_samples"][:, :, 0]), (what, c)
            continue
        mean = x.sum(axis=2) / spp
        bound = (spp + 3) * U * (np.abs(x).sum(axis=2) / spp)
        err = np.abs(got[c].astype(np.float64) - mean)
        print(what, c, "largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, (what, c, [(tuple(int(v) for v in b), err[tuple(b)], bound[tuple(b)]) for b in bad[:6]])
    assert (st.numPrimaryRays, st.numIntersectionTests, st.numIntersectionHits) == (
        rst.numPrimaryRays, rst.numIntersectionTests, rst.numIntersectionHits), (what, st, rst)
    assert st.numShadowRays == 0 and st.numReflectionRays == 0
    # both hitting and missing pixels, and both kinds of coverage
    assert (got["alpha"] == 0).any() and (got["alpha"] > 0).any(), what
    assert np.isinf(got["depth"][got["alpha"] == 0]).all() and (got["object"][got["alpha"] == 0] == -1).all()


@functools.lru_cache(maxsize=None)
def subset_ds(bits):
    return DeviceScene(ss.subset_scene(bits))


@functools.lru_cache(maxsize=None)
def coverage_ds(name):
    return DeviceScene(cs.scene(name))


# ---- 1. per sample -----------------------------------------------------------------------------
SAMPLINGS = ((akNone, 1), (akGrid, 2), (akGrid, 4))
M8_BITS = (ss.SPHERE | ss.BOX | ss.MESH, ss.MESH | ss.XF_GENERAL)
M8_NAMES = ("slats_ground",)


@pytest.mark.parametrize("bits", range(16), ids=[ss.subset_name(b) for b in range(16)])
def test_subset_scenes_against_the_picks(gpu, bits):
    ds = subset_ds(bits)
    scene = ss.subset_scene(bits)
    for kind, m in SAMPLINGS + (((akGrid, 8),) if bits in M8_BITS else ()):
        ref, rst, spp = reference(ds, scene, ss.W, ss.H, kind, m)
        got, st = aovs(ds, opts(ss.W, ss.H, kind, m))
        assert st.numPrimaryRays == ss.W * ss.H * spp
        judge(got, st, ref, rst, spp, (ss.subset_name(bits), int(kind), m))


@pytest.mark.parametrize("name", cs.SCENES)
def test_coverage_scenes_against_the_picks(gpu, name):
    ds = coverage_ds(name)
    for kind, m in SAMPLINGS + (((akGrid, 8),) if name in M8_NAMES else ()):
        ref, rst, spp = reference(ds, cs.scene(name), cs.W, cs.H, kind, m)
        got, st = aovs(ds, opts(cs.W, cs.H, kind, m))
        judge(got, st, ref, rst, spp, (name, int(kind), m))


# ---- 2. the sample positions of every sampler --------------------------------------------------
KEEP_M = (1, 3, 5, 7, 8, 9, 12, 16, 32)
COVERAGE = [c for c in cs.fp32_samplings() if c[2] in KEEP_M]


def _frame(ds, o):
    import torch
    fb = torch.zeros(o.height * o.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb)
    return fb.view(o.height, o.width, 3).cpu().numpy(), st


@pytest.mark.parametrize("name,kind,m,seed", COVERAGE, ids=[cs.case_id(*c) for c in COVERAGE])
def test_alpha_counts_the_frames_samples(gpu, name, kind, m, seed):
    ds = coverage_ds(name)
    spp = cs.spp_of(kind, m)
    o = cs.options(kind, m, seed, Precision.fp32)
    frame, fst = _frame(ds, o)
    got, st = aovs(ds, o, channels=("alpha", "object"))
    assert st.numPrimaryRays == fst.numPrimaryRays == cs.W * cs.H * spp
    counted = np.rint(got["alpha"].astype(np.float64) * spp).astype(np.int64)
    assert np.abs(got["alpha"].astype(np.float64) * spp - counted).max() <= 1e-3
    if name == "slats_mirror":  # a hit is 0.5, not 0: the frame's own decoding
        hits, off = cs.hit_counts(name, frame, spp)
        assert off.max() <= 0.05
    else:
        assert np.array_equal(frame[..., 0], frame[..., 1]) and np.array_equal(frame[..., 0], frame[..., 2])
        hits = spp - np.rint(frame[..., 0].astype(np.float64) * spp).astype(np.int64)
    bad = np.argwhere(counted != hits)
    assert bad.size == 0, [(int(x), int(y), int(counted[y, x]), int(hits[y, x])) for y, x in bad[:8]]
    assert 0 < hits.sum() < cs.W * cs.H * spp
    assert np.array_equal(got["object"] >= 0, counted > 0)


# ---- 3. lists against the BVH ------------------------------------------------------------------
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


@pytest.mark.parametrize("kind,m", [(akGrid, 4), (akGrid, 16), (akMultiJittered, 8)], ids=["grid4", "grid16", "mj8"])
@pytest.mark.parametrize("which", ["torus", "slats_ground"])
def test_lists_and_bvh_give_the_same_bytes(gpu, which, kind, m):
    if which == "torus":
        ds, w, h = DeviceScene(ss.subset_scene(ss.MESH)), ss.W, ss.H
    else:
        ds, w, h = DeviceScene(cs.scene(which)), cs.W, cs.H
    try:
        want = aovs(ds, opts(w, h, kind, m, seed=cs.SEEDS[0]))
        listed = _list_lengths(ds, w, h)
        assert listed.max() >= 2  # the call built lists, and some hold more than one face
        assert (want[0]["alpha"] > 0).any() and (want[0]["alpha"] == 0).any()
        same(aovs(ds, opts(w, h, kind, m, abi.RT_FLAG_NO_BINNING, seed=cs.SEEDS[0])), want)
        default = _slot_lg(ds)
        try:
            for lg in (0, 3):
                _slot_lg(ds, lg)
                same(aovs(ds, opts(w, h, kind, m, seed=cs.SEEDS[0])), want)
                over = _list_lengths(ds, w, h) > (1 << lg)
                print(which, int(kind), m, "slots", 1 << lg, "lists past their slots", int(over.sum()))
                if lg == 0:
                    assert over.any()  # some list really overflowed: those pixels took the BVH
        finally:
            _slot_lg(ds, default)
        same(aovs(ds, opts(w, h, kind, m, seed=cs.SEEDS[0])), want)
    finally:
        ds.close()


# ---- 4. rows, NULL channels, the host form -----------------------------------------------------
def _sentinels(w, h, host):
    import torch
    out = {}
    for c in CHANNELS:
        shape = (h, w, 3) if c in ("normal", "albedo") else (h, w)
        a = np.full(shape, -77, np.int32 if c in ("object", "face") else np.float32)
        out[c] = a if host else torch.from_numpy(a).cuda()
    return out


@pytest.mark.parametrize("kind,m", [(akGrid, 2), (akGrid, 8)], ids=["grid2", "grid8"])
def test_rows_channels_and_host_form(gpu, kind, m):
    ds = subset_ds(ss.SPHERE | ss.MESH)
    w, h = ss.W, ss.H
    o = opts(w, h, kind, m)
    whole = aovs(ds, o)
    for host in (False, True):
        part = aovs(ds, o, y0=5, y1=14, out=_sentinels(w, h, host))
        assert part[1].numPrimaryRays == 9 * w * m * m
        for c in CHANNELS:
            assert np.array_equal(part[0][c][5:14], whole[0][c][5:14]), (host, c)
            rest = np.concatenate([part[0][c][:5], part[0][c][14:]])
            assert (rest == -77).all(), (host, c)
    same(aovs(ds, o, host=True), whole)
    for c in CHANNELS:
        one = aovs(ds, o, channels=(c,), out={c: _sentinels(w, h, False)[c]})
        assert list(one[0]) == [c] and np.array_equal(one[0][c], whole[0][c]), c
        assert one[1] == whole[1]
    # y0 == y1: nothing is launched, nothing written, the last call stays the last call
    last = last_stats(ds)
    for host in (False, True):
        none = aovs(ds, o, y0=7, y1=7, out=_sentinels(w, h, host))
        assert none[1].numPrimaryRays == 0 and all((none[0][c] == -77).all() for c in CHANNELS)
    assert last_stats(ds) == last


# ---- 5. after edits ----------------------------------------------------------------------------
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


# ---- 6. scene state ----------------------------------------------------------------------------
def _diag(ds):
    return ds.last_split(), ds.last_lean_kernel(), ds.last_batch()


def test_a_colour_render_is_the_same_before_and_after(gpu):
    import torch
    from rtmi import scenes
    ds = DeviceScene(scenes.mesh_bunny())
    w, h = 128, 72
    o = opts(w, h, akGrid, 16)  # one pixel per wave: a two-class launch

    def colour():
        fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        st = ds.render_device(o, fb)
        return fb.cpu().numpy().tobytes(), st, _diag(ds)

    first = colour()
    assert first[2][0][0] > 0 and first[2][0][1] > 0  # lean and general pixels: two classes
    got, st = aovs(ds, o)
    assert last_stats(ds) == st and st.numPrimaryRays == w * h * 256 and st.numShadowRays == 0
    assert ds.last_split() == (0, ds.last_split()[1]) and ds.last_lean_kernel() == 0  # nothing classified
    assert (got["object"] == 0).any() and (got["object"] == 1).any() and (got["object"] == -1).any()
    assert colour() == first

    # three pipelined band calls, a feature-buffer call between the first and the second
    world, band_h = 3, 4
    rows = band_rows(h, band_h, world)

    def bands(with_aov):
        out = []
        for r in range(world):
            fb = torch.zeros(rows * w * 3, dtype=torch.float32, device="cuda")
            st = ds.render_bands_device(o, fb, band_h, r, world)
            assert ds.last_pipelined()
            out.append((fb.cpu().numpy().tobytes(), st, _diag(ds)))
            if with_aov and r == 0:
                mid = aovs(ds, o)
                assert raw(mid[0]) == raw(got) and mid[1] == st_aov
        return out

    st_aov = st
    assert bands(True) == bands(False)
    ds.close()


# ---- 7. errors ---------------------------------------------------------------------------------
def test_errors_leave_the_scene_usable(gpu):
    ds = subset_ds(ss.SPHERE | ss.MESH)
    w, h = ss.W, ss.H
    want = aovs(ds, opts(w, h, akGrid, 2))

    def code(o, **kw):
        with pytest.raises(RtmiError) as e:
            ds.render_aovs(o, **kw)
        return e.value.code

    assert code(opts(w, h, akGrid, 2, precision=Precision.fp64)) == abi.RT_E_UNSUPPORTED
    assert code(opts(w, h, akMultiJittered, 33)) == abi.RT_E_UNSUPPORTED
    assert code(opts(w, h, akGrid, 257)) == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y0=-1) == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y1=h + 1) == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), y0=9, y1=8) == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), channels=()) == abi.RT_E_INVALID
    assert code(opts(w, h, akGrid, 2), channels=(), host=True) == abi.RT_E_INVALID
    ds.render_aovs(opts(w, h, akGrid, 2), channels=(), y0=3, y1=3)  # no rows: no channel is needed
    same(aovs(ds, opts(w, h, akGrid, 2)), want)
