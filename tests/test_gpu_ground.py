"""Ground pixels of one-plane launches (rt_frame.hip k_frame_lists, rt_fast.h
ground1_batch): a general pixel with an empty camera-ray list that the
per-call build proves uniform-lit is flat ground whose shadow rays may meet
the mesh; the batched kernel runs only the shadow searches for it.

Every comparison is for bit-identical frames and equal Stats between flags 0
(the ground loop), RT_FLAG_NO_GROUND1 (the same kernels, gen1_batch for every
general pixel) and RT_FLAG_NO_SPLIT (k_render_fast, which shares none of this
code); only flags 0 may tag a pixel, and the (lean, general) and batched
counts do not depend on the tag."""
import math

import pytest

from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.abi import (RT_FLAG_BATCH_FALLBACK, RT_FLAG_NO_GROUND1, RT_FLAG_NO_MIX, RT_FLAG_NO_REORDER,
                      RT_FLAG_NO_SPLIT)
from rtmi.dist import band_rows
from rtmi.glm import X_AXIS, Z_AXIS, degToRad, inverse, mat4, normalize, rotate, translate, vec, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import DistantLight

pytestmark = pytest.mark.gpu


def _torus():
    """A small mesh on the ground plane, the two warm distant lights."""
    return scenes._mesh_scene(scenes.torus_mesh(96, 48), "t", (0.9, 0.5, 0.2))


def _opts(w, h, m, flags=0, bias=1e-4):
    # NO_REORDER as in test_gpu_split.py: small frames keep the two-class launch
    return Options(width=w, height=h, antialias=Antialias(akGrid, m), bias=bias, precision=Precision.fp32,
                   flags=flags | RT_FLAG_NO_REORDER)


def _whole(ds, o, fb):
    yield ds.render_device(o, fb)


def _compare(ds, w, h, m, bias=1e-4, calls=_whole, rows=None, extra=0, what=""):
    """Renders with flags 0, NO_GROUND1 (both with `extra`) and NO_SPLIT,
    asserts equal frames and Stats, that only flags 0 tags, and that the tag
    leaves the list lengths and the batched count alone. Returns (general,
    ground, fallback) summed over the calls made with flags 0."""
    import torch
    ref, counts = None, []
    for flags in (extra, extra | RT_FLAG_NO_GROUND1, RT_FLAG_NO_SPLIT):
        o = _opts(w, h, m, flags, bias)
        fb = torch.full(((rows or h) * w * 3,), -7.0, dtype=torch.float32, device="cuda")
        lean = general = ground = batched = fallback = 0
        sts = []
        for st in calls(ds, o, fb):  # a generator: the counters are read after each call
            sts.append(st)
            sp = ds.last_split()
            lean += sp[0]
            general += sp[1]
            ground += ds.last_ground()
            b = ds.last_batch()
            batched += b[0]
            fallback += b[1]
        counts.append((lean, general, batched, ground, fallback))
        if ref is None:
            ref = (fb, sts)
        else:
            assert sts == ref[1], (what, flags)
            assert torch.equal(fb, ref[0]), (what, flags, float((fb - ref[0]).abs().max()))
    print(what, "(lean, general, batched, ground, fallback):", counts)
    assert counts[1][3] == 0 and counts[2][3] == 0, (what, counts)
    assert counts[0][:3] == counts[1][:3], (what, counts)
    lean, general, batched, ground, fallback = counts[0]
    assert 0 <= ground <= general, (what, counts)
    return general, ground, fallback


def _lights(*dirs):
    return [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=3.0 - k, dir=normalize(vec(*d)))
            for k, d in enumerate(dirs)]


@pytest.mark.parametrize("m", [16, 32])
def test_whole_frame(gpu, m):
    """The torus's two shadows on the ground in front of the camera."""
    ds = DeviceScene(_torus())
    general, ground, fallback = _compare(ds, 192, 108, m, what=("whole", m))
    assert ground > 0, (general, ground)


def test_one_light(gpu):
    s = _torus()
    s.lights = _lights((-2.0, -0.8, -0.3))
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, what="one light")
    assert ground > 0, (general, ground)


def test_two_lights_five_degrees_apart(gpu):
    """The two shadows overlap almost everywhere: most ground pixels have
    both skip bits clear and search both lights' grids."""
    a = math.radians(5.0)
    d = (-2.0, -0.8, -0.3)
    d2 = (d[0] * math.cos(a) - d[2] * math.sin(a), d[1], d[0] * math.sin(a) + d[2] * math.cos(a))
    s = _torus()
    s.lights = _lights(d, d2)
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, what="5 degrees")
    assert ground > 0, (general, ground)


def test_plane_first(gpu):
    """The scene's objects in the other order: the plane, then the mesh."""
    s = _torus()
    s.objects = s.objects[::-1]
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, what="plane first")
    assert ground > 0, (general, ground)


def test_scanlines(gpu):
    """One call per scanline: short launches (16 lanes per lean pixel)."""
    ds = DeviceScene(_torus())
    w, h = 96, 64
    lanes = set()

    def lines(ds, o, fb):
        for y in range(h):
            yield ds.render_device(o, fb, y0=y, y1=y + 1)
            if ds.last_split()[0] > 0 and not o.flags & RT_FLAG_NO_SPLIT:
                lanes.add(ds.last_lean_lanes())

    general, ground, _ = _compare(ds, w, h, 16, calls=lines, what="scanlines")
    assert ground > 0, (general, ground)
    assert lanes == {16}, lanes


def test_bands(gpu):
    """A rank's round-robin bands (world 3): band rows and out_row."""
    ds = DeviceScene(_torus())
    w, h, world = 192, 108, 3
    rows = band_rows(h, 4, world)
    total = 0
    for r in range(world):
        def bands(ds, o, fb, r=r):
            yield ds.render_bands_device(o, fb, 4, r, world)
        total += _compare(ds, w, h, 16, calls=bands, rows=rows, what=("bands", r))[1]
    assert total > 0


def test_progressive(gpu):
    """renderLine's progressive passes: skipped pixels and step x step block
    fills of a ground pixel's sum."""
    ds = DeviceScene(_torus())
    for step, mx in ((4, 4), (2, 4), (1, 2)):
        def one(ds, o, fb, step=step, mx=mx):
            yield ds.render_device(o, fb, step=step, maxStep=mx)
        general, ground, _ = _compare(ds, 192, 108, 16, calls=one, what=("progressive", step, mx))
        assert ground > 0, (step, mx, general, ground)


def test_no_mix(gpu):
    """k_render_gen1 on its own (two kernels): the same general-pixel loop."""
    ds = DeviceScene(_torus())
    general, ground, _ = _compare(ds, 192, 108, 16, extra=RT_FLAG_NO_MIX, what="no mix")
    assert ground > 0, (general, ground)


def test_forced_fallback(gpu):
    """RT_FLAG_BATCH_FALLBACK: every tagged pixel's batch is discarded and the
    pixel rendered by the one-sample loop."""
    ds = DeviceScene(_torus())
    general, ground, fallback = _compare(ds, 192, 108, 16, extra=RT_FLAG_BATCH_FALLBACK, what="fallback")
    assert ground > 0 and fallback == general, (general, ground, fallback)


# (bias, lights or None for the scene's two): the per-call condition of the
# uniform-lit proof (rt_render.cpp uniform_cam) fails, so nothing may be tagged
NOT_LIT = [
    (0.0, None),
    (1e-7, None),                          # bias below the rounding error of the shadow origin's height
    (1e-4, ((-2.0, 0.0, -0.3),)),          # a light along the plane
    (1e-4, ((-2.0, -0.8, -0.3), (2.0, 0.8, -1.3))),  # one of two below the plane
]


@pytest.mark.parametrize("bias,dirs", NOT_LIT)
def test_condition_fails(gpu, bias, dirs):
    s = _torus()
    if dirs is not None:
        s.lights = _lights(*dirs)
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, bias=bias, what=("not lit", bias, dirs))
    assert general > 0 and ground == 0, (bias, dirs, general, ground)


def test_rolled_camera(gpu):
    """Rolled and pitched: the horizon crosses the frame on a slant; its
    pixels (hit and miss samples) stay plain general pixels, the shadows
    below it are tagged."""
    s = _torus()
    s.cameraToWorld = translate(rotate(rotate(mat4(1.0), Z_AXIS, degToRad(25.0)), X_AXIS, degToRad(-8.0)),
                                vec3(0.0, 5.5, 1.5))
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, what="rolled")
    assert 0 < ground < general, (general, ground)


def test_camera_far_above(gpu):
    """1e4 above the plane: 16 eps (|oy| + |ty| + |nroy|) = 0.038 is far above
    the bias, so the call's condition fails and nothing is tagged."""
    s = _torus()
    s.cameraToWorld = scenes._std_camera(0.0, 1e4, 1.5)
    general, ground, _ = _compare(DeviceScene(s), 192, 108, 16, what="1e4 above")
    assert ground == 0, (general, ground)


def test_origins_beyond_the_grid_radius(gpu):
    """A mesh whose vertices lie within 1.7 of its origin (its light grid's
    float32-safe radius rmax = 100 x that, under 170) placed 200 above the
    plane, still in front of the camera plane, and lit from above so that its
    shadow falls in front of the camera: every shadow origin in the shadow
    has |ro.y| = 200 > rmax, the batch declines and the one-sample loop
    renders the pixel."""
    s = scenes._mesh_scene(scenes.torus_mesh(48, 24, R=0.6, r=0.2), "t", (0.9, 0.5, 0.2))
    g = s.objects[0].geometry
    g.objectToWorld = translate(mat4(1.0), vec3(0.0, 200.0, -50.0))
    g.worldToObject = inverse(g.objectToWorld)
    s.lights = _lights((0.0, -200.0, 36.0))  # from the mesh towards (0, 0, -14)
    general, ground, fallback = _compare(DeviceScene(s), 192, 108, 16, what="beyond rmax")
    assert ground > 0 and fallback > 0, (general, ground, fallback)
