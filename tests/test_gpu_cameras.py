"""The per-call device builders (csrc/rt_frame.hip, rt_render.cpp frame_build /
frame_obj_masks) under cameras other than the standard viewpoint
(tests/cameras.py): a mesh a hair in front of the camera plane, views along,
across, from below and from exactly on the ground plane, a mesh a few pixels
wide, very wide and narrow fields of view, and a mesh box that reaches the
camera plane (the builders then decline and the kernels take the BVH).

* float64 frames and Stats equal the brute-force oracle bit for bit, one
  lane per pixel and (64 samples per pixel) one pixel per wave, whose camera
  rays read the call's device-built lists;
* float32 frames and Stats are bit-identical across every kernel variant
  (test_gpu_split.FLAG_SETS), the BVH-only kernel (RT_FLAG_NO_BINNING) being
  the anchor, whose distance to the oracle is bounded per camera;
* the device-built lists and records equal the host builders' on every
  pixel where both build them, and where the device must decline it does
  (no lists exist, and the camera rays fetch as many BVH nodes as the
  BVH-only kernel's);
* nothing of one camera survives into the next call;
* the huge-face list (rt_frame.h kBigFace / kHugeCap): below and past its
  capacity, its parity hand-over between calls, partial launches;
* the object masks of an analytic scene with boxes in front of, behind,
  across and around the camera."""
import ctypes as C
import math

import numpy as np
import pytest

import cameras
from rtmi import Antialias, Options, Precision, akGrid, akNone, scenes
from rtmi._lib import lib
from rtmi.abi import (RT_FLAG_COUNT_TRAVERSAL, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING, RT_FLAG_NO_OBJ_BATCH,
                      RT_FLAG_NO_REORDER)
from rtmi.glm import mat4, normalize, point, translate, vec, vec3
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import (DistantLight, Material, Object, PointLight, Scene, TriangleMesh, initBox, initPlane,
                        initSphere)
from test_gpu_configs import _log
from test_gpu_frame import _compare, _slot_lg
from test_gpu_split import FLAG_SETS, _assert_same, _frames
from test_gpu_split import _opts as _opts32

pytestmark = pytest.mark.gpu

BIAS = 1e-4
W32, H32 = 200, 120   # float32 frames
W64, H64 = 96, 64     # float64 / oracle frames


def _torus_scene():
    return scenes._mesh_scene(scenes.torus_mesh(24, 12), "torus", (0.9, 0.5, 0.2))


_TABLE = cameras.camera_table(_torus_scene().objects[0].geometry, _torus_scene().cameraToWorld)
CAMERAS = list(_TABLE)


def _aimed(cam, scene=None):
    """(Scene, DeviceScene) with camera `cam` set through set_camera (the
    Scene carries it too: the oracle renders from the Scene)."""
    sc = scene or _torus_scene()
    ds = DeviceScene(sc)
    if cam != "std":
        sc.cameraToWorld, sc.fov = _TABLE[cam]
        ds.set_camera()
    return sc, ds


def _render(ds, opts):
    import torch
    fb = torch.zeros(opts.height * opts.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    return fb, st


def _has_lists(ds, w, h):
    """Whether the only render call of this scene built camera-ray lists:
    the hook (rtmi_test_frame_lists) fails while the scene has never
    allocated list slots. After a declined call it would return an EARLIER
    call's lists, so the caller checks it is False before its one call."""
    f = lib().rtmi_test_frame_lists
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    off = np.zeros(w * h + 1, dtype=np.int32)
    info = np.zeros(w * h, dtype=np.uint32)
    ent = np.zeros(16, dtype=np.int32)
    return f(ds.h, off.ctypes.data, ent.ctypes.data, 16, info.ctypes.data) >= 0


def _host_accepts(ds, w, h):
    f = lib().rtmi_test_host_lists
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    off = np.zeros(w * h + 1, dtype=np.int32)
    info = np.zeros(w * h, dtype=np.uint32)
    ent = np.zeros(16, dtype=np.int32)
    return f(ds.h, w, h, BIAS, off.ctypes.data, ent.ctypes.data, 0, info.ctypes.data) >= 0


@pytest.mark.parametrize("cam", CAMERAS)
def test_fp64_equals_brute_force_oracle(gpu, oracle_mod, cam):
    sc, ds = _aimed(cam)
    ref_scene = oracle_mod.OracleScene(sc, bvh=False)
    for aa in (Antialias(akNone, 1), Antialias(akGrid, 2)):
        o = Options(width=W64, height=H64, antialias=aa, bias=BIAS, precision=Precision.fp64)
        ref, rst, _ = ref_scene.render(o)
        fb, st = _render(ds, o)
        got = fb.view(H64, W64, 3).cpu().numpy()
        assert np.array_equal(got, ref), (cam, aa, int(np.count_nonzero((got != ref).any(axis=2))))
        assert st == rst, (cam, aa, st, rst)
    # 64 samples per pixel: one pixel per wave (k_render_px64), whose camera
    # rays search this call's device-built lists in float64 (or, where the
    # builder declined and with NO_BINNING, the BVH)
    w, h = 48, 32
    o = Options(width=w, height=h, antialias=Antialias(akGrid, 8), bias=BIAS, precision=Precision.fp64)
    ref, rst, _ = ref_scene.render(o)
    for flags in (0, RT_FLAG_NO_BINNING):
        o.flags = flags
        fb, st = _render(ds, o)
        got = fb.view(h, w, 3).cpu().numpy()
        assert np.array_equal(got, ref), (cam, flags, int(np.count_nonzero((got != ref).any(axis=2))))
        assert st == rst, (cam, flags, st, rst)


@pytest.mark.parametrize("cam,lg", [(c, -1) for c in CAMERAS] + [("far_side", 0), ("far_side", 2)])
def test_fp32_kernel_variants_identical(gpu, cam, lg):
    """Every FLAG_SETS entry renders the BVH-only kernel's frame and Stats
    (far_side also with 1 and 4 slots per pixel: its few pixels list many
    faces each, so the lists overflow and those pixels take the BVH)."""
    _, ds = _aimed(cam)
    if lg >= 0:
        _render(ds, _opts32(W32, H32, 16))  # (the hook answers with the current slots: some must exist)
        _slot_lg(ds, lg)
    frames = _frames(ds, lambda f: _opts32(W32, H32, 16, f))
    if lg >= 0:
        assert _slot_lg(ds) == lg
        info = np.zeros(W32 * H32, dtype=np.uint32)
        assert lib().rtmi_test_pixel_info(ds.h, info.ctypes.data_as(C.c_void_p)) == 0
        assert ((info & 0xFFFFFF) > (1 << lg)).any()  # some list is past its slots
    assert FLAG_SETS[-1] == RT_FLAG_NO_BINNING
    _assert_same(frames[::-1], (cam, lg))  # anchored on NO_BINNING (the pairing of flags in the message is reversed)


def _point_light_scene():
    """The torus under one point light: shadow rays have no light grid and
    traverse the BVH with and without binning, so a difference in fetched
    BVH nodes between the two is the camera rays'."""
    sc = _torus_scene()
    sc.lights = [PointLight(color=vec3(1.0, 1.0, 1.0), intensity=4000.0, pos=point(0.5, 14.0, -12.0))]
    return sc


@pytest.mark.parametrize("cam", CAMERAS)
def test_device_lists_equal_host_or_decline(gpu, cam):
    sc, ds = _aimed(cam)
    assert not _has_lists(ds, W32, H32)  # a fresh scene: no call before this one
    _render(ds, _opts32(W32, H32, 16))
    built, host = _has_lists(ds, W32, H32), _host_accepts(ds, W32, H32)
    assert built == (cam not in cameras.DECLINED_ON_DEVICE), (cam, built)
    assert host == (cam not in cameras.DECLINED_ON_HOST), (cam, host)
    if built:
        entries, _ = _compare(ds, W32, H32, np.arange(W32 * H32))
        assert entries > 0 or cam == "fov_narrow"  # (sees the ground beyond the mesh: every list is empty)
        return
    # declined: the camera rays take the BVH, node for node like NO_BINNING
    _, dp = _aimed(cam, _point_light_scene())
    _render(dp, _opts32(W32, H32, 16, RT_FLAG_COUNT_TRAVERSAL))
    binned = dp.last_counters()
    _render(dp, _opts32(W32, H32, 16, RT_FLAG_COUNT_TRAVERSAL | RT_FLAG_NO_BINNING))
    bvh = dp.last_counters()
    assert binned["wave_node_fetches"] == bvh["wave_node_fetches"], (cam, binned, bvh)
    # (behind: no ray of the frame enters the mesh box, neither call fetches a node)
    assert bvh["wave_node_fetches"] > 0 or cam == "behind", (cam, bvh)


def test_node_fetches_tell_lists_from_the_bvh(gpu):
    """The control of the counter check above: where the device builds lists
    the binned call fetches fewer BVH nodes than the BVH-only one."""
    _, dp = _aimed("closeup_roll", _point_light_scene())
    _render(dp, _opts32(W32, H32, 16, RT_FLAG_COUNT_TRAVERSAL))
    binned = dp.last_counters()
    _render(dp, _opts32(W32, H32, 16, RT_FLAG_COUNT_TRAVERSAL | RT_FLAG_NO_BINNING))
    bvh = dp.last_counters()
    assert binned["wave_node_fetches"] < bvh["wave_node_fetches"], (binned, bvh)


def test_no_state_survives_a_camera(gpu):
    """std, straddle (declined), std, closeup, std on one scene: the std
    frames are bit-identical and the others equal a fresh scene's."""
    import torch
    sc, ds = _aimed("std")
    std = (np.array(sc.cameraToWorld), sc.fov)
    o = _opts32(W32, H32, 16)
    got = {}
    for k, cam in enumerate(("std", "straddle", "std", "closeup", "std")):
        ds.set_camera(*(std if cam == "std" else _TABLE[cam]))
        got[k, cam] = _render(ds, o)
    for k in (2, 4):
        assert torch.equal(got[0, "std"][0], got[k, "std"][0]) and got[0, "std"][1] == got[k, "std"][1], k
    for k, cam in ((1, "straddle"), (3, "closeup")):
        fresh = _render(_aimed(cam)[1], o)
        assert torch.equal(got[k, cam][0], fresh[0]) and got[k, cam][1] == fresh[1], cam


# Per camera: the measured distance of the float32 BVH-only frame (96 x 64,
# m = 16) to the oracle, profiles/cameras/parity_fp32.jsonl on MI355X:
# (pixels of the 6,144 off by more than 2e-3, by more than 1e-4, mean error).
MEASURED = {
    "closeup": (0, 1, 8.24e-8),           # max 4.6e-4
    "closeup_roll": (0, 2, 3.62e-7),      # max 1.5e-3
    "topdown": (1, 1, 4.53e-7),           # max 2.7e-3
    "grazing": (0, 0, 4.93e-9),           # max 1.2e-7
    "below": (0, 0, 6.61e-10),            # max 3.0e-8
    "far_side": (0, 0, 3.28e-10),         # max 1.2e-7
    "fov_wide": (0, 0, 4.49e-10),         # max 6.0e-8
    "fov_narrow": (0, 0, 0.0),            # max 0 (one colour: the ground)
    "fov_narrow_aimed": (0, 2, 2.46e-7),  # max 9.8e-4
    "straddle": (0, 1, 2.09e-8),          # max 1.3e-4
    "beside": (0, 0, 1.12e-9),            # max 3.0e-8
    "behind": (0, 0, 2.33e-10),           # max 1.5e-8
    "on_plane": (0, 0, 0.0),              # max 0 (every ray meets the plane at t = 0)
}


@pytest.mark.parametrize("cam", CAMERAS)
def test_fp32_anchor_against_oracle(gpu, oracle_mod, cam):
    """The anchor of the bit-identity checks, the float32 BVH-only frame,
    against the float64 oracle in the form of
    test_set_camera_renders_the_new_camera: share of pixels within 2e-3 and
    mean error. A float32 sample on the other side of a silhouette, a shadow
    edge or the horizon than the float64 one moves its pixel by up to about
    1 / m^2 of the contrast there; the pixels off by more than 1e-4 are those
    edge pixels, every other pixel is off by float32 rounding of its colour
    (at most 1.2e-7 measured: one float32 ulp of 1.0). Bounds per camera,
    from MEASURED with one more flipped sample on every edge pixel: every
    edge pixel may leave the 2e-3 band (pixels within 2e-3 >= the measured
    pixels within 1e-4), and the mean may grow by edge pixels / (pixels m^2),
    plus one float32 ulp of 1.0 for the rounding of the others.

    Measured on MI355X, of 6,144 pixels: at most 2 edge pixels per camera
    (closeup_roll and fov_narrow_aimed 2; closeup, topdown and straddle 1, of
    which topdown's is the only pixel of any camera beyond 2e-3, at 2.7e-3;
    the other eight cameras none), means 0 .. 4.5e-7; the figures per camera
    are MEASURED above. Every camera's error is explained by those
    silhouette pixels."""
    m = 16
    sc, ds = _aimed(cam)
    o = Options(width=W64, height=H64, antialias=Antialias(akGrid, m), bias=BIAS, precision=Precision.fp32,
                flags=RT_FLAG_NO_BINNING | RT_FLAG_NO_REORDER)
    fb, st = _render(ds, o)
    got = fb.view(H64, W64, 3).cpu().numpy()
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=True).render(o)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=2)
    _log(f"camera {cam} fp32 NO_BINNING {W64}x{H64} m={m}", err)
    assert st.numPrimaryRays == rst.numPrimaryRays
    _, edge, mean = MEASURED[cam]
    out, mean_now = int(np.count_nonzero(err > 2e-3)), float(err.mean())
    assert out <= edge and mean_now <= mean + edge / (err.size * m * m) + 2.0 ** -23, (cam, out, mean_now)


# ---- the huge-face list ------------------------------------------------------

GW, GH, GSIDE, GDIST = 640, 400, 8.6, 10.0
KBIG, KCAP, MARGIN = 64, 4096, 0.05  # rt_frame.h kBigFace, kHugeCap; rt_bins.h kPixelMargin


def _grid_scene(k):
    """A k x k quad grid (2 k^2 faces) of side 8.6 in a vertical plane, wound
    towards +z, and a camera straight in front of it."""
    t = np.linspace(-GSIDE / 2, GSIDE / 2, k + 1)
    X, Y = np.meshgrid(t, t + GSIDE / 2 + 0.2, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], axis=1)
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    a, b, c, d = i * (k + 1) + j, (i + 1) * (k + 1) + j, (i + 1) * (k + 1) + j + 1, i * (k + 1) + j + 1
    f = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    return scenes._mesh_scene(TriangleMesh(v, f.astype(np.int32)), "grid", (0.7, 0.6, 0.5))


def _grid_camera(sc, dist):
    lo, hi = cameras.world_box(sc.objects[0].geometry)
    c = 0.5 * (lo + hi)
    return cameras.lookat(c + [0.0, 0.0, dist], c), 50.0


def _huge_faces(sc, c2w, fov, w, h):
    """Faces whose grown, clipped pixel rectangle (rt_bins_geom.h
    face_project_rect) holds more than kBigFace pixels."""
    mesh = sc.objects[0].geometry
    p = cameras.world_vertices(mesh)[mesh.faces] - c2w[3, :3]  # (nf, 3, 3)
    x, y, z = p @ c2w[0, :3], p @ c2w[1, :3], p @ -c2w[2, :3]
    assert (z > 0).all()
    fo = math.tan(math.radians(fov) / 2)
    px = 0.5 * w + (x / z) / (2 * (w / h) * fo / w)
    py = 0.5 * h - (y / z) / (2 * fo / h)
    x0 = np.maximum(0, np.floor(px.min(1) - MARGIN))
    x1 = np.minimum(w - 1, np.floor(px.max(1) + MARGIN))
    y0 = np.maximum(0, np.floor(py.min(1) - MARGIN))
    y1 = np.minimum(h - 1, np.floor(py.max(1) + MARGIN))
    on = (px.max(1) + MARGIN >= 0) & (py.max(1) + MARGIN >= 0) & (px.min(1) - MARGIN < w) & (py.min(1) - MARGIN < h)
    area = np.where(on, (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    return int(np.count_nonzero(area > KBIG))


def _grid_aimed(k, dist=GDIST):
    sc = _grid_scene(k)
    ds = DeviceScene(sc)
    sc.cameraToWorld, sc.fov = _grid_camera(sc, dist)
    ds.set_camera()
    return sc, ds


@pytest.mark.parametrize("k", [46, 32])
def test_huge_face_list_below_and_past_its_capacity(gpu, oracle_mod, k):
    """k = 46: 4,232 huge faces, more than the list holds (the rest are
    walked by their blocks); k = 32: 2,048, all listed."""
    import torch
    sc, ds = _grid_aimed(k)
    n = _huge_faces(sc, sc.cameraToWorld, sc.fov, GW, GH)
    assert (n > KCAP) if k == 46 else (0 < n < KCAP), n
    frames = _frames(ds, lambda f: _opts32(GW, GH, 16, f))
    _assert_same(frames[::-1], ("grid", k))
    _render(ds, _opts32(GW, GH, 16))
    entries, _ = _compare(ds, GW, GH, np.arange(GW * GH))
    assert entries > GW * GH // 4  # the grid fills the middle of the frame
    o = Options(width=160, height=100, antialias=Antialias(akGrid, 2), bias=BIAS, precision=Precision.fp64)
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=False).render(o)
    fb, st = _render(ds, o)
    assert np.array_equal(fb.view(100, 160, 3).cpu().numpy(), ref) and st == rst
    # the full-size lists (the huge ones) read in float64: one pixel per wave
    # (64 spp) equals the one-lane-per-pixel BVH kernel on the whole frame,
    # and the oracle on rows through the grid, its edges and the ground
    o = Options(width=GW, height=GH, antialias=Antialias(akGrid, 8), bias=BIAS, precision=Precision.fp64)
    fb, st = _render(ds, o)
    o.flags = RT_FLAG_F64_PER_LANE
    fb_lane, st_lane = _render(ds, o)
    assert torch.equal(fb, fb_lane) and st == st_lane
    o.flags = 0
    rows = [3, 16, 17, 123, 200, 201, 383, 384, 396]
    ref = np.zeros((GH, GW, 3), np.float32)
    oracle_mod.OracleScene(sc, bvh=True).render(o, rows=rows, fb=ref)
    got = fb.view(GH, GW, 3).cpu().numpy()
    assert np.array_equal(got[rows], ref[rows])


def test_huge_face_list_parity_between_calls(gpu):
    """The list's two length words alternate between calls and each call
    zeroes the other's: a full list, none at all (camera at 40), a full list
    twice. Lists equal the host's on every pixel after every call."""
    import torch
    sc, ds = _grid_aimed(46)
    near, far = _grid_camera(sc, GDIST), _grid_camera(sc, 40.0)
    assert _huge_faces(sc, *far, GW, GH) == 0 and _huge_faces(sc, *near, GW, GH) > KCAP
    o = _opts32(GW, GH, 16)
    pix = np.arange(GW * GH)
    got = []
    for cam in (near, far, near, near):
        ds.set_camera(*cam)
        got.append(_render(ds, o))
        entries, _ = _compare(ds, GW, GH, pix)
        assert entries > 0
    for k in (2, 3):
        assert torch.equal(got[0][0], got[k][0]) and got[0][1] == got[k][1], k
    assert not torch.equal(got[0][0], got[1][0])


def test_huge_face_list_partial_launches(gpu):
    """A band launch, a row range and a progressive pass past the list's
    capacity: each equals the same launch without binning."""
    import torch
    _, ds = _grid_aimed(46)
    rows = band_rows(GH, 4, 3)
    res = []
    for flags in (0, RT_FLAG_NO_BINNING):
        b = torch.full((rows * GW * 3,), -7.0, dtype=torch.float32, device="cuda")
        res.append((b, ds.render_bands_device(_opts32(GW, GH, 16, flags), b, 4, 1, 3)))
    assert res[0][1] == res[1][1] and torch.equal(res[0][0], res[1][0])
    for kw in (dict(y0=37, y1=121), dict(step=2, maxStep=4)):
        res = []
        for flags in (0, RT_FLAG_NO_BINNING):
            fb = torch.full((GH * GW * 3,), -7.0, dtype=torch.float32, device="cuda")
            res.append((fb, ds.render_device(_opts32(GW, GH, 16, flags), fb, **kw)))
        assert res[0][1] == res[1][1] and torch.equal(res[0][0], res[1][0]), kw


# ---- object masks ------------------------------------------------------------

def _boxes_scene():
    """Nine analytic objects (the object-mask path takes 4..64) around the
    standard camera: boxes wholly in front of it, wholly behind it, across
    the camera plane off to the side (not around the camera) and around the
    camera; two more boxes, two spheres, the ground; one distant light."""
    cam = scenes._std_camera(0.0, 5.5, 1.5)
    eye, right, fwd = cam[3, :3], cam[0, :3], -cam[2, :3]

    def box(name, centre, half, albedo):
        return Object(name, initBox(objectToWorld=translate(mat4(1.0), vec3(*centre)), vmin=vec(-half, -half, -half),
                                    vmax=vec(half, half, half)), Material(albedo=vec3(*albedo)))

    objects = [
        Object("ground", initPlane(objectToWorld=mat4(1.0)), Material(albedo=vec3(0.4))),
        Object("ballA", initSphere(r=1.5, objectToWorld=translate(mat4(1.0), vec3(-3.0, 1.5, -10.0))),
               Material(albedo=vec3(0.9, 0.3, 0.2))),
        Object("ballB", initSphere(r=1.0, objectToWorld=translate(mat4(1.0), vec3(2.5, 1.0, -7.0))),
               Material(albedo=vec3(0.2, 0.5, 0.9))),
        box("front", eye + 10.0 * fwd, 1.0, (0.6, 0.9, 0.2)),
        box("behind", eye - 6.0 * fwd, 1.0, (0.9, 0.9, 0.2)),
        box("across", eye + 3.0 * right, 2.5, (0.9, 0.5, 0.2)),
        box("around", eye, 0.75, (0.5, 0.5, 0.5)),
        box("boxE", (-5.0, 0.6, -14.0), 0.6, (0.3, 0.8, 0.8)),
        box("boxF", (4.5, 0.8, -16.0), 0.8, (0.8, 0.3, 0.8)),
    ]
    lights = [DistantLight(color=vec3(1.0), intensity=4.0, dir=normalize(vec(-2.0, -0.8, -0.3)))]
    return Scene(objects=objects, lights=lights, fov=50.0, cameraToWorld=cam, bgColor=vec3(0.01, 0.03, 0.05))


def _box_depths(sc, name):
    ob = next(o for o in sc.objects if o.name == name)
    g = ob.geometry
    centre = np.asarray(g.objectToWorld, np.float64)[3, :3]
    return cameras.depths(sc.cameraToWorld, cameras.box_corners(centre + g.vmin, centre + g.vmax)), centre + g.vmin, centre + g.vmax


def test_object_masks_around_the_camera_plane(gpu, oracle_mod):
    import torch
    sc = _boxes_scene()
    eye = np.asarray(sc.cameraToWorld)[3, :3]
    d, lo, hi = _box_depths(sc, "front")
    assert d.min() > 0.0
    d, lo, hi = _box_depths(sc, "behind")
    assert d.max() < 0.0
    d, lo, hi = _box_depths(sc, "across")
    assert d.min() < 0.0 < d.max() and not ((lo <= eye) & (eye <= hi)).all()
    d, lo, hi = _box_depths(sc, "around")
    assert ((lo < eye) & (eye < hi)).all()
    assert 4 <= len(sc.objects) <= 64
    ds = DeviceScene(sc)
    for m in (8, 16):
        res = []
        for flags in (0, RT_FLAG_NO_OBJ_BATCH, RT_FLAG_NO_BINNING, RT_FLAG_NO_OBJ_BATCH | RT_FLAG_NO_BINNING):
            res.append((flags, *_render(ds, _opts32(W32, H32, m, flags))))
        for flags, fb, st in res[:-1]:
            assert st == res[-1][2], (m, flags, st, res[-1][2])
            assert torch.equal(fb, res[-1][1]), (m, flags, float((fb - res[-1][1]).abs().max()))
    o = Options(width=W64, height=H64, antialias=Antialias(akGrid, 2), bias=BIAS, precision=Precision.fp64)
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=False).render(o)
    fb, st = _render(ds, o)
    got = fb.view(H64, W64, 3).cpu().numpy()
    assert np.array_equal(got, ref) and st == rst
    # the across box shows in the frame (its visible part is in front of the camera plane)
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 50


# ---- a scene's float64 shadow records are released with it -------------------

def test_fp64_shadow_records_are_released_with_the_scene(gpu):
    """rt_scene::sh64 (built by the first float64 call that searches the
    light grids) goes with the scene: five create / render / close cycles in
    float64 lose no more device memory than the same cycles in float32."""
    import torch
    scene = scenes.mesh_bunny()

    def lost(prec):
        free = []
        for _ in range(5):
            ds = DeviceScene(scene)
            fb = torch.zeros(48 * 32 * 3, dtype=torch.float32, device="cuda")
            ds.render_device(Options(width=48, height=32, antialias=Antialias(akGrid, 8), bias=BIAS, precision=prec), fb)
            ds.close()
            del fb
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
        return free[0] - free[4]

    control = lost(Precision.fp32)
    assert lost(Precision.fp64) <= max(control, 0)
