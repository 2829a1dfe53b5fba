"""Frames at the counts of lights, objects and planes where the render
kernels and the per-call build change behaviour (DESIGN.md "Count limits"):
8 / 9 lights (a pixel record's eight skip bits, the two-class launch, the LDS
cache of k_render_px64), 32 / 33 lights (the 32-bit light masks), 3 / 4,
16 / 17 and 64 / 65 objects (object light grids, the LDS cache, the 64-bit
object masks and trace()'s walk in chunks of 64), 8 / 9 planes beside a mesh
(the shadow-skip proofs). tests/capacity_scenes.py has a scene either side of
each; test_capacity_scenes_cpu.py proves on the oracle that every object and
light of each decides pixels.

* float64 frames and Stats equal the oracle's bit for bit: one pixel per wave
  (akGrid m = 8, k_render_px64), one lane per pixel (m = 2,
  RT_FLAG_F64_PER_LANE), and on the light-axis mesh scenes one stochastic
  kind at m = 3;
* float32 frames against the same oracle frames as test_gpu_subsets._compare32
  compares them (equal primary rays, the other counts within rel 1e-2,
  DESIGN.md (c)'s tolerance, error <= 1e-4 on every smooth pixel): m = 4
  under the default dispatch and the plain flags, m = 8, and RT_FLAG_COMPACT
  on the mirror scene. RTMI_PARITY_LOG=<file> appends the measured distances
  (profiles/capacity/parity_fp32.jsonl);
* the rt_scene_last_* diagnostics, the float32 specialisation and the object
  light grids show that the intended side of each limit ran;
* rt_scene_set_lights through 2, 9, 8, 33, 32, 4 lights and
  rt_scene_set_objects at 64 and 65 objects equal a fresh scene;
* ray, pick and radiance queries at 65 objects and at 33 lights equal the
  oracle's; band launches equal the whole frame's rows."""
import json
import os

import numpy as np
import pytest

import capacity_scenes as cs
import shade_cases as sc
from query_checks import Got, Ref, _dev, check, check_stats, trace
from rtmi import Precision, akGrid
from rtmi.abi import (RT_FLAG_COMPACT, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING, RT_FLAG_NO_OBJ_BATCH,
                      RT_FLAG_NO_REORDER, RT_FLAG_NO_SPLIT)
from rtmi.dist import rank_rows
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import Sphere
from subset_scenes import MESH, POINT, pixel_error
from test_gpu_objects import _object_grids, _shift
from test_gpu_relight import _assert_same, _render as _render_diag

pytestmark = pytest.mark.gpu

PLAIN = RT_FLAG_NO_BINNING | RT_FLAG_NO_SPLIT | RT_FLAG_NO_OBJ_BATCH | RT_FLAG_NO_REORDER
FLAG_NAMES = {0: "default", PLAIN: "plain", RT_FLAG_COMPACT: "compact"}


def _render(ds, o):
    import torch
    fb = torch.zeros(o.height * o.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb)
    return fb.view(o.height, o.width, 3).cpu().numpy(), st


def _record(what, err, mask):
    path = os.environ.get("RTMI_PARITY_LOG")
    row = {"what": what, "pixels": int(err.size), "beyond_2e-3": int(np.count_nonzero(err > 2e-3)),
           "beyond_1e-4": int(np.count_nonzero(err > 1e-4)), "mean": float(err.mean()),
           "smooth_share": float(mask.mean()), "smooth_max": float(err[mask].max())}
    print(json.dumps(row))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")
    return row


def _compare64(oracle_mod, ds, name, kind, m, flags=0):
    ref, rst = cs.oracle_frame(oracle_mod, name, kind, m)
    got, st = _render(ds, cs.options(name, kind, m, Precision.fp64, flags))
    what = (name, int(kind), m, flags)
    assert np.array_equal(got, ref), (what, int(np.count_nonzero((got != ref).any(axis=2))))
    assert st == rst, (what, st, rst)


def _compare32(oracle_mod, ds, name, m, flags=0):
    ref, rst, _, mask = cs.oracle_frames(oracle_mod, name, akGrid, m)
    got, st = _render(ds, cs.options(name, akGrid, m, Precision.fp32, flags))
    err = pixel_error(got, ref)
    what = f"capacity {name} fp32 {FLAG_NAMES[flags]} m={m}"
    row = _record(what, err, mask)
    assert st.numPrimaryRays == rst.numPrimaryRays, (what, st, rst)
    assert st.numIntersectionTests == pytest.approx(rst.numIntersectionTests, rel=1e-2), (what, st, rst)
    assert st.numShadowRays == pytest.approx(rst.numShadowRays, rel=1e-2), (what, st, rst)
    assert st.numReflectionRays == pytest.approx(rst.numReflectionRays, rel=1e-2), (what, st, rst)
    assert row["smooth_share"] >= 0.65, row
    assert float((err <= 2e-3).mean()) >= 0.995, row
    assert row["mean"] <= 2e-4, row
    assert row["smooth_max"] <= 1e-4, (row, [tuple(p) for p in np.argwhere(mask & (err > 1e-4))[:8]])


def _counts(ds, name):
    scene = cs.scene(name)
    info = ds.info()
    assert info["num_lights"] == len(scene.lights) and info["num_objects"] == len(scene.objects), (name, info)


# ---- float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.NAMES)
def test_fp64_equals_oracle(gpu, oracle_mod, name):
    ds = DeviceScene(cs.scene(name))
    _counts(ds, name)
    _compare64(oracle_mod, ds, name, akGrid, 8)                        # k_render_px64
    _compare64(oracle_mod, ds, name, akGrid, 2, RT_FLAG_F64_PER_LANE)
    if name in cs.LIGHT_MESH:
        _compare64(oracle_mod, ds, name, cs.STOCHASTIC, 3)


# ---- float32, and the side of each limit that ran ---------------------------------------
@pytest.mark.parametrize("name", cs.NAMES)
def test_fp32_against_oracle(gpu, oracle_mod, name):
    scene = cs.scene(name)
    ds = DeviceScene(scene)
    _counts(ds, name)
    for flags in (0, PLAIN):
        _compare32(oracle_mod, ds, name, 4, flags)
        assert not ds.last_compacted()
    if name == "mirror-last":
        _compare32(oracle_mod, ds, name, 4, RT_FLAG_COMPACT)
        assert ds.last_compacted()
    _compare32(oracle_mod, ds, name, 8)  # one pixel per wave: records, the two-class launch
    w, h = cs.size(name)
    lean, general = ds.last_split()
    k = ds.last_lean_kernel()
    sub = ds.f32_subset(cs.options(name, akGrid, 8, Precision.fp32))
    assert bool(sub & POINT) == (name in cs.MIXED), (name, sub)
    assert bool(sub & MESH) == cs.has_mesh(name), (name, sub)
    if name in cs.LIGHT_MESH:
        n = len(scene.lights)
        if name in cs.MIXED:
            # a point light has no skip proof: no pixel is lean beside one
            assert k & 3 == 0 and lean == 0, (name, k, lean, general)
        elif n <= 8:
            # a lean and a general-list kernel ran; every pixel is in one of the lists, and a
            # lean pixel has every light's skip bit (all eight of a record at 8 lights)
            assert k & 3 and k >> 2, (name, k)
            assert lean > 0 and general > 0 and lean + general == w * h, (name, lean, general)
        else:
            assert k == 0 and lean == 0, (name, k, lean, general)
    if name.startswith("lights-warm-") and len(scene.lights) > 8:
        assert k == 0 and lean == 0, (name, k, lean, general)


@pytest.mark.parametrize("n", cs.OBJECT_COUNTS)
def test_object_light_grids_exist_from_4_to_64_objects(gpu, n):
    ds = DeviceScene(cs.objects_scene(n))
    hdr, masks, off_grid = _object_grids(ds, 2)
    if n in (3, 65, 130):
        assert masks.size == 0, (n, masks.size)
        return
    assert masks.size > 0
    bit63 = False
    for li in range(2):
        g = hdr[li]
        cells = masks[int(g["off_base"]):int(g["off_base"]) + int(g["gu"]) * int(g["gv"])]
        assert cells.size == int(g["gu"]) * int(g["gv"]) > 0
        assert np.unique(cells).size > 1
        bit63 = bit63 or bool(np.any(cells >> np.uint64(63)))
    assert bit63 == (n == 64)


# ---- crossing a limit in place -------------------------------------------------------------
RELIT_W, RELIT_H = cs.SMALL


def _both(ds):
    """The float32 and the float64 one-pixel-per-wave frames (m = 8), each with Stats and diagnostics."""
    return tuple(_render_diag(ds, prec, 8, RELIT_W, RELIT_H) for prec in (Precision.fp32, Precision.fp64))


def test_relight_across_the_light_limits(gpu):
    ds = DeviceScene(cs.lights_mesh(2))
    _both(ds)
    for n in (9, 8, 33, 32, 4):
        lights = cs.cone_lights(n)
        ds.set_lights(lights)
        got = _both(ds)
        _assert_same(got, _both(DeviceScene(cs.lights_mesh(n))))
        assert ds.info()["num_lights"] == n
        lean_word = got[0][2][0]
        assert bool(lean_word & 15) == (n <= 8), (n, lean_word)


@pytest.mark.parametrize("n", (64, 65))
def test_moved_object_at_the_object_limit(gpu, n):
    scene = cs.objects_scene(n)
    ds = DeviceScene(scene)
    before = _both(ds)
    last = [o for o in scene.objects if isinstance(o.geometry, Sphere)][-1]
    assert scene.objects.index(last) >= 62
    _shift(last, 0.3, 0.2, -0.25)
    ds.set_objects()
    got = _both(ds)
    _assert_same(got, _both(DeviceScene(scene)))
    assert not np.array_equal(got[0][0], before[0][0]) and not np.array_equal(got[1][0], before[1][0])
    assert ds.info()["num_objects"] == n


# ---- queries --------------------------------------------------------------------------------
QUERY_SCENES = ("objects-65", "lights-mesh-33p8p32")


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_ray_queries(gpu, oracle_mod, name):
    scene = cs.scene(name)
    ds = DeviceScene(scene)
    osc = oracle_mod.OracleScene(scene)
    orig, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, sc.W1, sc.H1)
    assert len(orig) == 165
    want = Ref(osc, orig, d)
    assert len(set(want.obj.tolist())) >= 2  # (the mesh scene: the torus and the ground)
    got = trace(ds, orig, d)
    check(got, want)
    check_stats(got, want)
    # any hit: t_near half of and twice the closest hit's t, in turn
    tn = want.t * np.where(np.arange(165) % 2 == 0, 0.5, 2.0)
    any_want = Ref(osc, orig, d, tn)
    assert 0.05 <= float((any_want.obj >= 0).mean()) <= 0.95
    any_got = trace(ds, orig, d, tn, any_hit=True)
    assert np.array_equal(any_got.obj >= 0, any_want.obj >= 0)
    check_stats(any_got, any_want)
    # pick: castPrimaryRay through the scene's camera at the same image positions
    opts = sc.options(sc.W1, sc.H1, 0, cs.BIAS, cs.depth(name))
    picked = Got(ds.pick(opts, _dev(np.array(sc.sample_xy(sc.W1, sc.H1))), stats=True))
    check(picked, want)
    assert picked.stats.numPrimaryRays == 165
    assert picked.stats.numIntersectionTests == int(want.tests.sum())
    assert picked.stats.numIntersectionHits == int(want.hits.sum())


@pytest.mark.parametrize("w,h,m", [(sc.W1, sc.H1, 0), (sc.W2, sc.H2, 3)], ids=["group1", "group9"])
@pytest.mark.parametrize("name", QUERY_SCENES)
def test_radiance_queries(gpu, oracle_mod, name, w, h, m):
    """group 1 over the 165 rays of a 15 x 11 image; group 9 over the 180
    rays of a 5 x 4 image at akGrid m = 3 (n must be a multiple of the group)."""
    scene = cs.scene(name)
    ds = DeviceScene(scene)
    orig, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, w, h, m)
    rgb, fb, rst, _ = sc.oracle_image(oracle_mod, scene, w, h, m, cs.BIAS, cs.depth(name))
    opts = sc.options(w, h, m, cs.BIAS, cs.depth(name))
    got, st = ds.shade_rays(opts, orig, d, group=max(1, m * m), stats=True)
    assert sc.same_bits(got, rgb), np.argwhere(got != rgb)[:5]
    assert st == rst, (st, rst)
    got32 = ds.shade_rays(opts, orig, d, group=max(1, m * m), f32=True)
    assert sc.same_bits(got32, fb)
    assert rst.numShadowRays > 0 and len(np.unique(rgb, axis=0)) > 3


# ---- bands -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("lights-mesh-8", "objects-65"))
def test_bands_equal_the_frames_rows(gpu, name):
    import torch
    world, band_h = 3, 4
    ds = DeviceScene(cs.scene(name))
    o = cs.options(name, akGrid, 8, Precision.fp32)
    whole, _ = _render(ds, o)
    rows = band_rows(o.height, band_h, world)
    seen = np.zeros(o.height, bool)
    for r in range(world):
        b = torch.full((rows * o.width * 3,), -7.0, dtype=torch.float32, device="cuda")
        ds.render_bands_device(o, b, band_h, r, world)
        band = b.view(rows, o.width, 3).cpu().numpy()
        ys = rank_rows(o.height, band_h, r, world)
        assert np.array_equal(band[ys >= 0], whole[ys[ys >= 0]]), (name, r)
        seen[ys[ys >= 0]] = True
    assert seen.all()
