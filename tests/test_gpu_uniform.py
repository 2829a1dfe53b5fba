"""Uniform lean pixels of one-plane launches (rt_bins_geom.h uniform_class,
rt_fast.h lean1q_loop): the per-call build proves, in the lean kernel's own
float32 arithmetic, which lean pixels have samples that all hit the plane
unshadowed (uniform-lit) or all miss it (uniform-sky); the kernel writes such
a pixel's fixed sum of one constant without running its sample loop.

Every comparison is for bit-identical frames and equal Stats between flags 0
(the shortcut), RT_FLAG_NO_UNIFORM (the same kernels, every pixel's samples)
and RT_FLAG_NO_SPLIT (k_render_fast, which shares none of this code)."""
import pytest

from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.abi import RT_FLAG_NO_REORDER, RT_FLAG_NO_SPLIT, RT_FLAG_NO_UNIFORM
from rtmi.dist import band_rows
from rtmi.glm import X_AXIS, Z_AXIS, degToRad, mat4, normalize, rotate, translate, vec, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import DistantLight

pytestmark = pytest.mark.gpu

FLAGS = (0, RT_FLAG_NO_UNIFORM, RT_FLAG_NO_SPLIT)


def _torus():
    """A small mesh on the ground plane, the two warm distant lights."""
    return scenes._mesh_scene(scenes.torus_mesh(96, 48), "t", (0.9, 0.5, 0.2))


def _opts(w, h, m, flags=0, bias=1e-4):
    # NO_REORDER as in test_gpu_split.py: small frames keep the two-class launch
    return Options(width=w, height=h, antialias=Antialias(akGrid, m), bias=bias, precision=Precision.fp32,
                   flags=flags | RT_FLAG_NO_REORDER)


def _whole(ds, o, fb):
    return [ds.render_device(o, fb)]


def _compare(ds, w, h, m, bias=1e-4, calls=_whole, rows=None, what=""):
    """Renders with each of FLAGS, asserts equal frames and Stats (and that
    only flags 0 classifies), and returns (lean, lit, sky) summed over the
    calls made with flags 0."""
    import torch
    ref, counts = None, {}
    for flags in FLAGS:
        o = _opts(w, h, m, flags, bias)
        fb = torch.full(((rows or h) * w * 3,), -7.0, dtype=torch.float32, device="cuda")
        lean = lit = sky = 0
        sts = []
        for st in calls(ds, o, fb):  # a generator: the counters are read after each call
            sts.append(st)
            lean += ds.last_split()[0]
            u = ds.last_uniform()
            lit += u[0]
            sky += u[1]
        counts[flags] = (lean, lit, sky)
        if ref is None:
            ref = (fb, sts)
        else:
            assert sts == ref[1], (what, flags)
            assert torch.equal(fb, ref[0]), (what, flags, float((fb - ref[0]).abs().max()))
    assert counts[RT_FLAG_NO_UNIFORM][1:] == (0, 0) and counts[RT_FLAG_NO_SPLIT] == (0, 0, 0), (what, counts)
    assert counts[0][0] == counts[RT_FLAG_NO_UNIFORM][0], (what, counts)  # lean includes the uniform pixels
    lean, lit, sky = counts[0]
    assert 0 <= lit and 0 <= sky and lit + sky <= lean, (what, counts)
    return counts[0]


def _rolled(roll=25.0, pitch=-8.0):
    s = _torus()
    s.cameraToWorld = translate(rotate(rotate(mat4(1.0), Z_AXIS, degToRad(roll)), X_AXIS, degToRad(pitch)),
                                vec3(0.0, 5.5, 1.5))
    return s


@pytest.mark.parametrize("m", [16, 32])
def test_rolled_camera_whole_frame(gpu, m):
    """Rolled and pitched: the horizon crosses the frame on a slant, so many
    pixels have hit and miss samples (the build's shadow-skip test leaves most
    of them to the general list) and uniform pixels of both kinds border them
    in every column."""
    ds = DeviceScene(_rolled())
    lean, lit, sky = _compare(ds, 192, 108, m, what=("rolled", m))
    print("rolled", m, "lean", lean, "lit", lit, "sky", sky)
    assert lit > 0 and sky > 0, (lean, lit, sky)


def test_rolled_camera_scanlines(gpu):
    """One call per scanline: short launches (16 lanes per lean pixel)."""
    ds = DeviceScene(_rolled())
    w, h = 96, 64
    lanes = set()

    def lines(ds, o, fb):
        for y in range(h):
            yield ds.render_device(o, fb, y0=y, y1=y + 1)
            if o.flags == RT_FLAG_NO_REORDER and ds.last_split()[0] > 0:
                lanes.add(ds.last_lean_lanes())

    lean, lit, sky = _compare(ds, w, h, 16, calls=lines, what="scanlines")
    assert lit > 0 and sky > 0, (lean, lit, sky)
    assert lanes == {16}, lanes


def test_rolled_camera_progressive(gpu):
    """renderLine's progressive passes: skipped pixels and step x step block
    fills of a uniform pixel's constant."""
    ds = DeviceScene(_rolled())
    for step, mx in ((4, 4), (2, 4), (1, 2)):
        def one(ds, o, fb, step=step, mx=mx):
            yield ds.render_device(o, fb, step=step, maxStep=mx)
        lean, lit, sky = _compare(ds, 192, 108, 16, calls=one, what=("progressive", step, mx))
        assert lit > 0 and sky > 0, (step, mx, lean, lit, sky)


def test_rolled_camera_bands(gpu):
    """A rank's round-robin bands (world 3): band rows and out_row."""
    ds = DeviceScene(_rolled())
    w, h, world = 240, 135, 3
    rows = band_rows(h, 4, world)
    for r in range(world):
        def bands(ds, o, fb, r=r):
            yield ds.render_bands_device(o, fb, 4, r, world)
        lean, lit, sky = _compare(ds, w, h, 16, calls=bands, rows=rows, what=("bands", r))
        assert lit > 0 and sky > 0, (r, lean, lit, sky)


@pytest.mark.parametrize("cam_y", [2.0, -2.0])
@pytest.mark.parametrize("fov", [0.01, 0.2])
def test_grazing_view(gpu, cam_y, fov):
    """A level camera with a field of view far under 1 degree, aimed at the
    horizon: |dy| passes through the kernel's 1e-6 threshold inside the frame
    (fov 0.01: about 3e-6 per pixel row), above and below the plane (both
    signs of nroy)."""
    s = _torus()
    s.fov = fov
    s.cameraToWorld = translate(mat4(1.0), vec3(0.0, cam_y, 1.5))
    ds = DeviceScene(s)
    for m in (16, 32):
        lean, lit, sky = _compare(ds, 96, 64, m, what=("grazing", cam_y, fov, m))
        # (from above the plane the build leaves the far ground to the general
        # list: its shadow skips cannot be proved; from below most pixels are lean)
        print("grazing", cam_y, fov, m, "lean", lean, "lit", lit, "sky", sky)


def _lights(*dirs, raw=False):
    return [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=3.0 - k, dir=vec(*d) if raw else normalize(vec(*d)))
            for k, d in enumerate(dirs)]


# (bias, camera height, lights or None for the scene's two, whether uniform-lit pixels may exist)
CONDITIONS = [
    (1e-4, 5.5, None, True),
    (1e-7, 5.5, None, False),     # bias below the rounding error of the shadow origin's height
    (0.0, 5.5, None, False),
    (1e-4, 1e4, None, False),     # the same bound, 1e4 above the plane
    (1e-4, 5.5, ((-2.0, -0.8, -0.3),), True),                      # one light
    (1e-4, 5.5, ((2.0, 0.8, -1.3),), False),                       # one light below the plane
    (1e-4, 5.5, ((-2.0, -0.8, -0.3), (2.0, 0.8, -1.3)), False),    # one of two below
    (1e-4, 5.5, ((-2.0, 0.0, -0.3),), False),                      # along the plane
    (1e-4, 5.5, ((-2.0, -0.8, -0.3), (2.0, -1e-6, -1.3)), False),  # |dir.y| <= 1e-6 after normalising
]


@pytest.mark.parametrize("bias,cam_y,dirs,may_lit", CONDITIONS)
def test_per_call_condition(gpu, bias, cam_y, dirs, may_lit):
    """The call's condition for uniform-lit pixels: where it must fail no
    pixel is uniform-lit, uniform-sky pixels stay, and the frames match
    either way."""
    s = _torus()
    s.cameraToWorld = scenes._std_camera(0.0, cam_y, 1.5)
    if dirs is not None:
        s.lights = _lights(*dirs)
    ds = DeviceScene(s)
    lean, lit, sky = _compare(ds, 192, 108, 16, bias=bias, what=("condition", bias, cam_y, dirs))
    print("condition", bias, cam_y, dirs, "lean", lean, "lit", lit, "sky", sky)
    assert lean > 0 and (lit > 0) == may_lit, (bias, cam_y, dirs, lean, lit, sky)


def test_camera_on_the_plane(gpu):
    """nroy == 0: t is a zero whose sign decides the hit, sample by sample;
    no pixel is uniform-lit."""
    s = _torus()
    s.cameraToWorld = rotate(translate(mat4(1.0), vec3(0.0, 0.0, 1.5)), X_AXIS, degToRad(-12.0))
    assert s.cameraToWorld[3][1] == 0.0  # (column 3: the camera's position)
    ds = DeviceScene(s)
    for m in (16, 32):
        lean, lit, sky = _compare(ds, 192, 108, m, what=("on the plane", m))
        assert lit == 0, (lean, lit, sky)


def test_it_fires_on_c3(gpu):
    """The C3 scene and camera: the per-call condition holds, and a pixel can
    fail the proof only within a fraction of a pixel of the horizon (N changes
    by about 1e-2 per pixel row there against a threshold near 1e-6): at most
    3 of 135 rows. So at least 90 % of the lean pixels are uniform. The whole
    1080p frame (4 lanes per lean pixel) as well."""
    ds = DeviceScene(scenes.mesh_bunny())
    lean, lit, sky = _compare(ds, 240, 135, 16, what="C3 240x135")
    print("C3 240x135: lean", lean, "lit", lit, "sky", sky)
    assert lean > 0 and lit > 0 and sky > 0 and lit + sky >= 0.9 * lean, (lean, lit, sky)
    lanes = []

    def whole(ds, o, fb):
        yield ds.render_device(o, fb)
        lanes.append(ds.last_lean_lanes())

    lean, lit, sky = _compare(ds, 1920, 1080, 16, calls=whole, what="C3 1080p")
    print("C3 1920x1080: lean", lean, "lit", lit, "sky", sky)
    assert lanes[0] == 4 and lit + sky >= 0.9 * lean, (lanes, lean, lit, sky)
