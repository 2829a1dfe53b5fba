"""The one-plane float32 kernels (k_render_mix1 / _gen1 / _lean1q) away from
the ground at y = 0, on the thresholds of their per-call proofs (rt_render.cpp
uniform_cam, rt_bins_geom.h uniform_class, the ground tag of k_frame_lists,
rt_fast.h lean1q_loop's constant sum and ground1_batch) and across a seeded
population of cameras (cameras.oneplane_case).

Every comparison is for bit-identical frames and equal Stats across FLAGS,
anchored on the BVH-only kernel (RT_FLAG_NO_BINNING), and every test asserts
from the flags-0 call's counters that the path it is about really ran. The
float64 oracle anchors the translated plane independently: bit for bit in
float64 (one pixel per wave, k_render_px64), and within the measured float32
distance for the BVH-only frame."""
import ctypes as C
import math

import numpy as np
import pytest

import cameras
from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi._lib import lib
from rtmi.abi import (RT_FLAG_BATCH_FALLBACK, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING, RT_FLAG_NO_GEN1,
                      RT_FLAG_NO_GROUND1, RT_FLAG_NO_LEAN1, RT_FLAG_NO_MIX, RT_FLAG_NO_REORDER, RT_FLAG_NO_SPLIT,
                      RT_FLAG_NO_UNIFORM)
from rtmi.glm import inverse, mat4, translate, vec3
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import Material, Object, Scene, initPlane
from test_gpu_configs import _log
from test_gpu_split import _opts
from test_gpu_uniform import _lights
from test_uniform_cpu import LIT, bound, classify

pytestmark = pytest.mark.gpu

# (test_gpu_split._frames renders its own FLAG_SETS; these are this file's,
# with the same _opts: every call carries RT_FLAG_NO_REORDER)
FLAGS = (0, RT_FLAG_NO_UNIFORM, RT_FLAG_NO_GROUND1, RT_FLAG_NO_MIX, RT_FLAG_NO_LEAN1 | RT_FLAG_NO_GEN1,
         RT_FLAG_BATCH_FALLBACK, RT_FLAG_NO_SPLIT, RT_FLAG_NO_BINNING)
BIAS = 1e-4
W, H = 96, 64
KPIX_COUNT = 0xFFFFFF  # rt_frame.h: a pixel record's list length; its shadow skip bits sit above bit 24


def _torus():
    return scenes.torus_mesh(24, 12)


def _scene(gy, mesh_t=(0.0, 0.0001, -12.0), plane_xz=(0.0, 0.0), plane_first=False, lights=None, c2w=None, fov=50.0,
           mesh=None):
    """The torus scene with its ground, mesh and standard camera lifted by gy
    (mesh_t, c2w: relative to the ground)."""
    mesh = mesh or _torus()
    mesh.objectToWorld = translate(mat4(1.0), vec3(mesh_t[0], gy + mesh_t[1], mesh_t[2]))
    mesh.worldToObject = inverse(mesh.objectToWorld)
    objects = [Object("torus", mesh, Material(albedo=vec3(0.9, 0.5, 0.2))),
               Object("ground", initPlane(translate(mat4(1.0), vec3(plane_xz[0], gy, plane_xz[1]))),
                      Material(albedo=vec3(0.4)))]
    cam = np.array(scenes._std_camera(0.0, 5.5, 1.5) if c2w is None else c2w, np.float64)
    cam[3][1] += gy
    return Scene(objects=objects[::-1] if plane_first else objects, lights=lights or scenes._warm_lights(), fov=fov,
                 cameraToWorld=cam, bgColor=vec3(0.01, 0.03, 0.05))


def _whole(ds, o, fb):
    yield ds.render_device(o, fb)


class Counts:
    def __init__(self):
        self.lean = self.general = self.lit = self.sky = self.ground = self.batched = self.fallback = 0
        self.kernels = set()

    def read(self, ds):
        sp = ds.last_split()
        self.lean += sp[0]
        self.general += sp[1]
        u = ds.last_uniform()
        self.lit += u[0]
        self.sky += u[1]
        self.ground += ds.last_ground()
        b = ds.last_batch()
        self.batched += b[0]
        self.fallback += b[1]
        self.kernels.add(ds.last_lean_kernel())

    def __repr__(self):
        return (f"lean {self.lean} general {self.general} lit {self.lit} sky {self.sky} ground {self.ground} "
                f"batched {self.batched} fallback {self.fallback} kernels {sorted(self.kernels)}")


def _compare(ds, w, h, m, bias=BIAS, calls=_whole, rows=None, what=""):
    """Renders with each of FLAGS; asserts frames and Stats equal to the
    RT_FLAG_NO_BINNING call's. Returns the flags-0 calls' counters (summed)
    and the anchor frame (rows, w, 3) on the host."""
    import torch
    res, cnt = [], Counts()
    for flags in FLAGS:
        o = _opts(w, h, m, flags, bias=bias)
        fb = torch.full(((rows or h) * w * 3,), -7.0, dtype=torch.float32, device="cuda")
        sts = []
        for st in calls(ds, o, fb):  # a generator: the counters are read after each call
            sts.append(st)
            if flags == 0:
                cnt.read(ds)
        res.append((fb, sts))
    assert FLAGS[-1] == RT_FLAG_NO_BINNING
    ref, rsts = res[-1]
    for flags, (fb, sts) in zip(FLAGS[:-1], res[:-1]):
        assert sts == rsts, (what, hex(flags), sts, rsts)
        assert torch.equal(fb, ref), (what, hex(flags), float((fb - ref).abs().max()),
                                      int(((fb != ref).view(-1, 3).any(dim=1)).sum()))
    return cnt, ref.view(rows or h, w, 3).cpu().numpy()


def _bound(scene):
    """uniform_cam's bound for this scene: (bound, nroy)."""
    plane = next(o for o in scene.objects if not hasattr(o.geometry, "faces")).geometry
    return bound(scene.cameraToWorld[3][1], plane.worldToObject[3][1])


# ---- a. translated ground -----------------------------------------------------

GYS = [-3.0, 2.5, 700.0]
PLANE_XZ = (13.0, -7.0)


@pytest.mark.parametrize("plane_first", [False, True])
@pytest.mark.parametrize("m", [16, 32, 64])
@pytest.mark.parametrize("gy", GYS)
def test_translated_ground(gpu, gy, m, plane_first):
    """Ground, mesh and camera lifted by gy, the plane also moved in x and z
    (which changes nothing). At gy = 700 the bound 16 eps (|oy| + |ty| +
    |nroy|) = 2.7e-3 is set by |ty|: bias 1e-4 is below it (nothing is
    uniform-lit or tagged), bias 1e-2 above."""
    sc = _scene(gy, plane_xz=PLANE_XZ, plane_first=plane_first)
    ds = DeviceScene(sc)
    bnd, _ = _bound(sc)
    for bias in ((1e-4, 1e-2) if gy == 700.0 else (1e-4,)):
        cnt, _ = _compare(ds, W, H, m, bias=bias, what=("translated", gy, m, plane_first, bias))
        print("translated", gy, m, plane_first, bias, "bound", bnd, cnt)
        assert cnt.kernels == {15}, cnt  # k_render_mix1
        assert cnt.sky > 0 and cnt.general > 0 and cnt.batched == cnt.general, cnt
        if bias > bnd:
            assert cnt.lit > 0 and cnt.ground > 0, cnt
        else:
            assert gy == 700.0 and bias == 1e-4 and cnt.lit == 0 and cnt.ground == 0, (bnd, cnt)
    assert (bnd > 1e-4) == (gy == 700.0) and bnd < 1e-2, bnd


def test_plane_xz_translation_changes_nothing(gpu):
    import torch
    frames = []
    for xz in ((0.0, 0.0), PLANE_XZ):
        ds = DeviceScene(_scene(2.5, plane_xz=xz))
        fb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
        st = ds.render_device(_opts(W, H, 16), fb)
        assert ds.last_lean_kernel() == 15
        frames.append((fb, st))
    assert frames[0][1] == frames[1][1] and torch.equal(frames[0][0], frames[1][0])


# ---- b. ground through the mesh -----------------------------------------------

def _through_scene(cam):
    """The plane at the height of the torus's box centre (gy = 2.5: the plane
    is off y = 0 as well); cam: "std" or "below" (looking up at the mesh)."""
    mesh = _torus()
    lo, hi = mesh.vertices.min(axis=0), mesh.vertices.max(axis=0)
    half = 0.5 * (lo[1] + hi[1])
    gy = 2.5
    c2w = None
    if cam == "below":
        c2w = cameras.lookat([1.0, -4.0, -5.0], [0.0, 0.0, -12.0])
    return _scene(gy, mesh_t=(0.0, -half, -12.0), c2w=c2w, mesh=mesh)


def _pixel_info(ds, w, h):
    info = np.zeros(w * h, dtype=np.uint32)
    f = lib().rtmi_test_pixel_info
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(ds.h, info.ctypes.data) == 0
    return info.reshape(h, w)


def _plane_hits(sc, w, h):
    """The plane hit points of the pixel centres' camera rays, float64: (h, w, 3)."""
    c2w = np.asarray(sc.cameraToWorld, np.float64)
    gy = next(o for o in sc.objects if not hasattr(o.geometry, "faces")).geometry.objectToWorld[3][1]
    fo = math.tan(math.radians(sc.fov) / 2)
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    cx, cy = (xs - w / 2) * (2 * (w / h) * fo / w), (h / 2 - ys) * (2 * fo / h)
    d = cx[..., None] * c2w[0, :3] + cy[..., None] * c2w[1, :3] - c2w[2, :3]
    with np.errstate(all="ignore"):
        t = (gy - c2w[3][1]) / d[..., 1]
    return c2w[3, :3] + t[..., None] * d, t


@pytest.mark.parametrize("cam", ["std", "below"])
def test_ground_through_the_mesh(gpu, cam):
    """The mesh box straddles the plane, so ground pixels inside the box's
    footprint start their shadow rays inside the box: the reference's "a ray
    that starts inside the box misses the mesh" quirk, which ground1_batch's
    mesh gate must reproduce (k_render_fast and the BVH-only kernel are the
    anchors)."""
    sc = _through_scene(cam)
    ds = DeviceScene(sc)
    for m in (16, 32):
        cnt, _ = _compare(ds, W, H, m, what=("through", cam, m))
        print("through", cam, m, cnt)
        assert cnt.kernels == {15} and cnt.general > 0 and cnt.batched == cnt.general, cnt
        if cam == "std":
            assert cnt.ground > 0 and cnt.lit > 0, cnt
    if cam != "std":
        return
    # which pixels the flags-0 call tagged: general (some skip bit clear), an
    # empty camera list, uniform-lit (the host's uniform_class: the same
    # function on the same inputs) — their number is the call's ground count
    import torch
    fb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    ds.render_device(_opts(W, H, 16), fb)
    info = _pixel_info(ds, W, H)
    full = (1 << len(sc.lights)) - 1
    plane = sc.objects[1].geometry
    cls, ok, _ = classify(sc.cameraToWorld, sc.fov, W, H, 16, plane.worldToObject[3][1], BIAS,
                          [li.dir[:3] for li in sc.lights])
    tagged = ((info & KPIX_COUNT) == 0) & (((info >> 24) & full) != full) & (cls == LIT)
    assert ok == 1 and int(tagged.sum()) == ds.last_ground() > 0, (int(tagged.sum()), ds.last_ground())
    hits, t = _plane_hits(sc, W, H)
    origin = hits + np.array([0.0, BIAS, 0.0])
    lo, hi = cameras.world_box(sc.objects[0].geometry)
    inside = ((origin > lo) & (origin < hi)).all(axis=2) & (t > 0)
    assert (tagged & inside).any(), (int(tagged.sum()), int(inside.sum()))
    print("through: tagged", int(tagged.sum()), "of them starting inside the mesh box", int((tagged & inside).sum()))


# ---- c. the per-call thresholds, one float32 apart ------------------------------

def _f32_above(x):
    """The smallest float32 > x and the largest float32 <= x (x a float64)."""
    lo = np.float32(x)
    if float(lo) > x:
        lo = np.nextafter(lo, np.float32(-np.inf))
    return float(np.nextafter(lo, np.float32(np.inf))), float(lo)


@pytest.mark.parametrize("gy", [0.0, 2.5])
def test_bias_either_side_of_the_bound(gpu, gy):
    sc = _scene(gy)
    ds = DeviceScene(sc)
    bnd, _ = _bound(sc)
    above, below = _f32_above(bnd)
    assert below <= bnd < above and float(np.float32(above)) == above and float(np.float32(below)) == below
    cnt, _ = _compare(ds, W, H, 16, bias=above, what=("bias above", gy))
    print("bias", gy, "bound", bnd, "above", above, cnt)
    assert cnt.kernels == {15} and cnt.lit > 0 and cnt.ground > 0, cnt
    cnt, _ = _compare(ds, W, H, 16, bias=below, what=("bias below", gy))
    print("bias", gy, "bound", bnd, "below", below, cnt)
    assert cnt.kernels == {15} and cnt.lit == 0 and cnt.ground == 0 and cnt.sky > 0 and cnt.general > 0, cnt


F1E_6, F1E6 = np.float32(1e-6), np.float32(1e6)
LIGHT_HEIGHTS = [
    # (dir.y, dir.x, dir.z, whether uniform-lit pixels may exist): not normalised
    (-float(np.nextafter(F1E_6, np.float32(1.0))), -1.0, -0.25, True),
    (-float(F1E_6), -1.0, -0.25, False),
    (-float(F1E6), -2.0e6, -0.5e6, True),
    (-float(np.nextafter(F1E6, np.float32(np.inf))), -2.0e6, -0.5e6, False),
]


@pytest.mark.parametrize("y,x,z,may_lit", LIGHT_HEIGHTS)
def test_light_height_either_side(gpu, y, x, z, may_lit):
    """One light that is not normalised, sd.y = -dir.y one float32 either
    side of 1e-6 (a light all but along the plane: the torus's shadow is a
    strip from the mesh to the frame's edge) and of 1e6 (the warm light's
    direction, scaled)."""
    sc = _scene(0.0, lights=_lights((x, y, z), raw=True))
    assert float(np.float32(sc.lights[0].dir[1])) == y
    ds = DeviceScene(sc)
    cnt, _ = _compare(ds, W, H, 16, what=("light height", y))
    print("light height", y, cnt)
    # the one-plane lean kernel ran (merged or on its own; a light along the
    # plane may have no grid for the batched general kernel to search)
    assert cnt.lean > 0 and all(kind & 3 >= 2 for kind in cnt.kernels) and cnt.sky > 0 and cnt.general > 0, cnt
    if not may_lit:
        assert cnt.lit == 0 and cnt.ground == 0, cnt
    elif abs(y) > 1.0:
        assert cnt.kernels == {15} and cnt.lit > 0 and cnt.ground > 0, cnt


# ---- d. a seeded population ------------------------------------------------------
#
# cameras.oneplane_case: with every parameter drawn independently (seed
# 20261019) the mesh box is in front of the camera plane in 34 of the 48 cases,
# the per-call condition holds in 9, uniform-lit pixels exist in 3 and no frame
# sees a shadow, so the quotas of test_population_is_not_vacuous cannot hold;
# the generator couples the pitch or the camera's height to the mesh's distance
# in two cases of three and mirrors the lights to above the plane in three of
# four (cameras.AIMED_SHARE, SHADOW_SHARE, ABOVE_SHARE), and the seed is
# cameras.ONEPLANE_SEED. Measured on MI355X: k_render_mix1 in 45 cases,
# uniform-lit, uniform-sky and ground pixels in 19 each, a listed pixel in 23.

NCASES = 48
_RNG = np.random.default_rng(cameras.ONEPLANE_SEED)
CASES = [cameras.oneplane_case(_RNG) for _ in range(NCASES)]
SEEN = {}  # case index -> the flags-0 counters and whether a general pixel has a non-empty camera list


def _case_scene(c):
    mesh = _torus()
    sections = mesh.vertices.reshape(24, 12, 3).mean(axis=1)  # the tube's centre line: inside the solid
    t = cameras.oneplane_mesh_translation(c, mesh.vertices, sections[np.argmax(sections[:, 1])])
    mesh.objectToWorld = translate(mat4(1.0), vec3(*t))
    mesh.worldToObject = inverse(mesh.objectToWorld)
    objects = [Object("torus", mesh, Material(albedo=vec3(0.9, 0.5, 0.2))),
               Object("ground", initPlane(translate(mat4(1.0), vec3(0.0, c["gy"], 0.0))), Material(albedo=vec3(0.4)))]
    from rtmi.glm import vec
    from rtmi.scene import DistantLight
    lights = [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=3.0 - k, dir=vec(*d)) for k, d in enumerate(c["lights"])]
    return Scene(objects=objects, lights=lights, fov=c["fov"], cameraToWorld=np.array(c["c2w"]),
                 bgColor=vec3(0.01, 0.03, 0.05))


def _case_calls(k, c):
    """(calls generator, rows of the buffer or None) of the case's call shape."""
    h, shape = c["h"], c["shape"]
    if shape == "whole":
        return _whole, None
    if shape == "rows":
        y0, y1 = h // 4, max(h // 4 + 1, (3 * h) // 4)
        return (lambda ds, o, fb: iter([ds.render_device(o, fb, y0=y0, y1=y1)])), None
    if shape == "scanlines":
        y0 = max(0, h // 2 - 4)

        def lines(ds, o, fb):
            for y in range(y0, min(h, y0 + 8)):
                yield ds.render_device(o, fb, y0=y, y1=y + 1)
        return lines, None
    if shape == "band_rank":
        return (lambda ds, o, fb: iter([ds.render_bands_device(o, fb, 4, k % 3, 3)])), band_rows(h, 4, 3)
    assert shape == "progressive"
    return (lambda ds, o, fb: iter([ds.render_device(o, fb, step=2, maxStep=4)])), None


@pytest.mark.parametrize("k", range(NCASES))
def test_population(gpu, k):
    c = CASES[k]
    print("case", k, {q: c[q] for q in ("gy", "cam_h", "pitch", "roll", "fov", "lights", "bias", "m", "w", "h", "shape",
                                       "dist", "cut", "aimed", "aim_shadow")})
    sc = _case_scene(c)
    ds = DeviceScene(sc)
    calls, rows = _case_calls(k, c)
    cnt, _ = _compare(ds, c["w"], c["h"], c["m"], bias=c["bias"], calls=calls, rows=rows, what=("case", k))
    listed = False
    if cnt.general > 0 and 15 in cnt.kernels:
        info = _pixel_info(ds, c["w"], c["h"])  # (the last call's pixels; the others hold earlier calls' records or 0)
        listed = bool(((info & KPIX_COUNT) > 0).any())
    print("case", k, cnt, "listed", listed)
    SEEN[k] = (cnt, listed)


def test_population_is_not_vacuous(gpu):
    if len(SEEN) < NCASES:
        pytest.skip("the population's cases were deselected")
    mix = sum(1 for cnt, _ in SEEN.values() if 15 in cnt.kernels)
    lit = sum(1 for cnt, _ in SEEN.values() if cnt.lit > 0)
    sky = sum(1 for cnt, _ in SEEN.values() if cnt.sky > 0)
    ground = sum(1 for cnt, _ in SEEN.values() if cnt.ground > 0)
    listed = sum(1 for _, li in SEEN.values() if li)
    sizes = [(c["w"] % 64 != 0, c["h"] % 4 != 0) for c in CASES]
    print("population: mix1", mix, "lit", lit, "sky", sky, "ground", ground, "listed", listed)
    assert mix >= 36 and min(lit, sky, ground, listed) >= 12, (mix, lit, sky, ground, listed)
    assert any(a for a, _ in sizes) and any(b for _, b in sizes)
    assert {c["shape"] for c in CASES} == set(cameras.ONEPLANE_SHAPES) and {c["m"] for c in CASES} == {16, 32, 64}


# ---- e. the float64 anchor --------------------------------------------------------

def _anchor_scenes():
    out = {}
    for gy in GYS:
        for pf in (False, True):
            out[f"translated {gy} {'plane' if pf else 'mesh'} first"] = lambda gy=gy, pf=pf: _scene(gy, plane_xz=PLANE_XZ,
                                                                                                   plane_first=pf)
    for cam in ("std", "below"):
        out[f"through {cam}"] = lambda cam=cam: _through_scene(cam)
    return out


ANCHORS = _anchor_scenes()
ANCHORS64 = dict(ANCHORS, **{f"case {k}": (lambda k=k: _case_scene(CASES[k])) for k in range(0, NCASES, 4)})


@pytest.mark.parametrize("name", list(ANCHORS64))
def test_fp64_equals_oracle(gpu, oracle_mod, name):
    """64 samples per pixel in float64: one pixel per wave (k_render_px64,
    whose lean samples transform into the plane's space with ty != 0), one
    lane per pixel, and the BVH only, against the oracle bit for bit."""
    import torch
    sc = ANCHORS64[name]()
    ds = DeviceScene(sc)
    w, h = 48, 32
    bias = CASES[int(name.split()[1])]["bias"] if name.startswith("case") else BIAS
    o = Options(width=w, height=h, antialias=Antialias(akGrid, 8), bias=bias, precision=Precision.fp64)
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=True).render(o)
    for flags in (0, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING):
        o.flags = flags
        fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        st = ds.render_device(o, fb)
        got = fb.view(h, w, 3).cpu().numpy()
        assert np.array_equal(got, ref), (name, flags, int(np.count_nonzero((got != ref).any(axis=2))))
        assert st == rst, (name, flags, st, rst)


# ---- f. the float32 anchor --------------------------------------------------------

# Per scene: the measured distance of the float32 BVH-only frame (96 x 64,
# m = 16) to the oracle, profiles/cameras/parity_fp32.jsonl on MI355X:
# (pixels of the 6,144 off by more than 2e-3, by more than 1e-4, mean error).
MEASURED = {
    "translated -3.0 mesh first": (0, 1, 7.45e-8),     # max 4.2e-4
    "translated -3.0 plane first": (0, 1, 7.45e-8),    # max 4.2e-4
    "translated 2.5 mesh first": (0, 0, 6.13e-9),      # max 1.2e-7
    "translated 2.5 plane first": (0, 0, 6.13e-9),     # max 1.2e-7
    # (700 up, a float32 world coordinate has steps of 6e-5: silhouettes and
    # shadow edges move by that much, all 64 pixels are edge pixels)
    "translated 700.0 mesh first": (2, 64, 5.51e-6),   # max 3.0e-3
    "translated 700.0 plane first": (2, 64, 5.51e-6),  # max 3.0e-3
    "through std": (0, 0, 1.31e-8),                    # max 6.2e-5
    "through below": (0, 0, 3.46e-10),                 # max 1.5e-8
}


@pytest.mark.parametrize("name", list(ANCHORS))
def test_fp32_anchor_against_oracle(gpu, oracle_mod, name):
    """The form of test_gpu_cameras.test_fp32_anchor_against_oracle: from
    MEASURED with one more flipped sample on every edge pixel, every edge
    pixel may leave the 2e-3 band and the mean may grow by edge pixels /
    (pixels m^2) plus one float32 ulp of 1.0. Every pixel off by more than
    1e-4 must be an edge pixel of the oracle's frame (a silhouette, a shadow
    edge or the horizon: a neighbour differs by more than 1e-2): any other
    would be an error of the float32 plane code that the kernels share."""
    import torch
    m = 16
    sc = ANCHORS[name]()
    ds = DeviceScene(sc)
    o = Options(width=W, height=H, antialias=Antialias(akGrid, m), bias=BIAS, precision=Precision.fp32,
                flags=RT_FLAG_NO_BINNING | RT_FLAG_NO_REORDER)
    fb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb)
    got = fb.view(H, W, 3).cpu().numpy()
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=True).render(o)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=2)
    _log(f"oneplane {name} fp32 NO_BINNING {W}x{H} m={m}", err)
    out, fine, mean_now = int(np.count_nonzero(err > 2e-3)), int(np.count_nonzero(err > 1e-4)), float(err.mean())
    print("fp32 anchor", name, "beyond 2e-3:", out, "beyond 1e-4:", fine, "mean:", mean_now, "max:", float(err.max()))
    assert st.numPrimaryRays == rst.numPrimaryRays
    pad = np.pad(ref.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    edge_px = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            edge_px |= np.abs(pad[dy:dy + H, dx:dx + W] - ref).max(axis=2) > 1e-2
    off = err > 1e-4
    assert not (off & ~edge_px).any(), (name, np.argwhere(off & ~edge_px)[:5], float(err[off & ~edge_px].max()))
    _, edge, mean = MEASURED[name]
    assert out <= edge and mean_now <= mean + edge / (err.size * m * m) + 2.0 ** -23, (name, out, mean_now)
