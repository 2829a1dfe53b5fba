"""The rays and expected answers of the radiance-query tests
(DeviceScene.shade_rays, rt_shade_rays*): shared by test_gpu_shade_rays.py,
which sends the rays to the device, and test_shade_cases_cpu.py, which proves
on the oracle and tests/truth.py alone that the rays leave the device
comparisons room. Nothing here touches a GPU.

* camera batches: the rays oracle.cast_primary_ray forms for an image, one
  per integer pixel (calcPixelNoSampling) or m x m per pixel at akGrid's
  positions (calcPixel), so the oracle's own calc_pixel is the expected
  colour, bit for bit. Every expected answer is computed once and shared.
* the four cameras of the camera-independence test on subset 63;
* truth rays: 96 seeded rays with unnormalised directions on subsets 35 and
  63, which the oracle's camera cannot form, with the multiprecision truth of
  their colour (truth._trace + truth.shade), recorded by
  tests/golden/make_truth_shade.py in truth_shade_<bits>.npz."""
import dataclasses
import functools

import numpy as np

from rtmi import Antialias, Options, Precision, akGrid, akNone, scenes
from rtmi.scene import Box, DistantLight, Plane, Sphere, TriangleMesh

import cameras
import truth
import truth_cases as tc
from subset_scenes import REFLECT, subset_scene

SCENES = {**{f"s{bits}": functools.partial(subset_scene, bits) for bits in tc.FRAME_BITS},
          "two_meshes": scenes.two_meshes}
REFLECTIVE = tuple(f"s{bits}" for bits in tc.FRAME_BITS if bits & REFLECT)
BIAS, DEPTH = tc.BIAS, tc.DEPTH
W1, H1 = 15, 11             # 165 rays: two full waves and a 37-lane tail
W2, H2 = 5, 4
GRID_M = (2, 3, 8)          # groups of 4 (divides a wave), 9 (straddles waves), 64 (one wave)

TRUTH_BITS = (35, 63)
N_TRUTH = 96
TRUTH_SCALES = (0.25, 0.5, 1.0, 3.0)


def options(w, h, m=0, bias=BIAS, depth=DEPTH):
    return Options(width=w, height=h, antialias=Antialias(akGrid if m else akNone, max(m, 1)), bias=bias,
                   maxRayDepth=depth, precision=Precision.fp64)


def with_camera(scene, c2w, fov):
    return dataclasses.replace(scene, cameraToWorld=np.asarray(c2w, np.float64), fov=float(fov))


# ---- camera batches ----------------------------------------------------------
def sample_xy(w, h, m=0):
    """Image positions of an image's primary rays in calcPixel's order: the
    pixels row by row; per pixel the one corner sample (m = 0) or grid()'s
    m x m positions x + (i*xs + xoffs), y + (j*ys + yoffs), j outer."""
    if m == 0:
        return [(float(x), float(y)) for y in range(h) for x in range(w)]
    xs = ys = 1.0 / float(m)
    xoffs = yoffs = xs * 0.5
    return [(float(x) + (float(i) * xs + xoffs), float(y) + (float(j) * ys + yoffs))
            for y in range(h) for x in range(w) for j in range(m) for i in range(m)]


def camera_rays(oracle_mod, c2w, fov, w, h, m=0):
    """(orig (n, 3), dir (n, 3)): castPrimaryRay at sample_xy's positions."""
    rays = [oracle_mod.cast_primary_ray(w, h, x, y, float(fov), c2w) for x, y in sample_xy(w, h, m)]
    return (np.ascontiguousarray([o[:3] for o, _ in rays]), np.ascontiguousarray([d[:3] for _, d in rays]))


@functools.lru_cache(maxsize=None)
def scene_rays(oracle_mod, name, w, h, m=0):
    sc = SCENES[name]()
    o, d = camera_rays(oracle_mod, sc.cameraToWorld, sc.fov, w, h, m)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def stats_tuple(st):
    return (st.numPrimaryRays, st.numIntersectionTests, st.numIntersectionHits, st.numShadowRays,
            st.numReflectionRays)


def oracle_image(oracle_mod, scene, w, h, m=0, bias=BIAS, depth=DEPTH):
    """The oracle's answers for an image, pixels row by row: calc_pixel's
    float64 colours (h * w, 3) and per-pixel Stats (h * w, 5: stats_tuple's
    order), render_line's float32 rows (h * w, 3) and the image's Stats."""
    osc = oracle_mod.OracleScene(scene)
    opts = options(w, h, m, bias, depth)
    px = [osc.calc_pixel(opts, x, y) for y in range(h) for x in range(w)]
    rgb = np.array([c for c, _ in px])
    per_px = np.array([stats_tuple(st) for _, st in px], np.int64)
    fb, st, _ = osc.render(opts, nthreads=4)
    assert stats_tuple(st) == tuple(per_px.sum(0))
    return rgb, fb.reshape(-1, 3), st, per_px


@functools.lru_cache(maxsize=None)
def expected(oracle_mod, name, w, h, m=0, bias=BIAS, depth=DEPTH):
    out = oracle_image(oracle_mod, SCENES[name](), w, h, m, bias, depth)
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


def ordered_mean(colours, group):
    """calcPixel's expression (renderer.nim:147-159) over each run of `group`
    colours: from 0, added in index order in float64, times 1.0 / group."""
    c = np.asarray(colours, np.float64).reshape(-1, group, 3)
    acc = np.zeros((len(c), 3))
    for j in range(group):
        acc = acc + c[:, j]
    return acc * (1.0 / float(group))


def same_bits(a, b):
    """Equal as bit patterns (so -0.0 differs from 0.0), NaN equal to NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


# ---- the four cameras of the independence test (subset 63) --------------------------
CAM_W, CAM_H = 12, 9


def cameras63():
    """name -> (cameraToWorld, fov): the scene's own camera; one inside the
    torus's world box (TriangleMesh.intersect's AABB gate, geom.nim:339-358:
    its rays miss the torus they start in); one below the ground looking up
    (no ray misses: each meets the plane from below, or an object the
    reference's t places before it); the scene's camera at fov 120."""
    sc = subset_scene(63)
    mesh = next(o.geometry for o in sc.objects if isinstance(o.geometry, TriangleMesh))
    lo, hi = cameras.world_box(mesh)
    c = 0.5 * (lo + hi)
    return {
        "default": (np.asarray(sc.cameraToWorld, np.float64), sc.fov),
        "in_mesh_box": (cameras.lookat(c, [-3.5, 1.6, -11.0]), 70.0),   # at ballA, through the torus's hole side
        "below_ground": (cameras.lookat([c[0] + 1.0, -4.0, hi[2] + 5.0], c), sc.fov),
        "fov120": (np.asarray(sc.cameraToWorld, np.float64), 120.0),
    }


# ---- what a batch hits (the CPU proofs) ------------------------------------------------
def kind_of(geometry):
    return {Sphere: "sphere", Plane: "plane", Box: "box", TriangleMesh: "mesh"}[type(geometry)]


def classify(oracle_mod, scene, orig, d, bias=BIAS):
    """Per ray the object the oracle's trace hits (-1: none) and whether any
    of the scene's lights is hidden from the hit / seen from it: the shadow
    rays formed as shade forms them (in numpy: these flags only prove that
    both cases occur, they are not compared with anything)."""
    osc = oracle_mod.OracleScene(scene)
    obj = np.full(len(orig), -1)
    shadowed = np.zeros(len(orig), bool)
    lit = np.zeros(len(orig), bool)
    for i, (o, dd) in enumerate(zip(orig, d)):
        o4, d4 = np.append(o, 1.0), np.append(dd, 0.0)
        ob, t, tri, _ = osc.trace(o4, d4)
        obj[i] = ob
        if ob < 0:
            continue
        hw = o + dd * t
        n = osc.hit_normal(o4, d4, ob, t, tri)[:3]
        for L in scene.lights:
            if isinstance(L, DistantLight):
                to_light, dist = -np.asarray(L.dir, np.float64)[:3], float("inf")
            else:
                v = hw - np.asarray(L.pos, np.float64)[:3]
                dist = float(np.linalg.norm(v))
                to_light = -v / dist
            s_ob, _, _, _ = osc.trace(np.append(hw + n * bias, 1.0), np.append(to_light, 0.0), dist)
            shadowed[i] |= s_ob >= 0
            lit[i] |= s_ob < 0
    return obj, shadowed, lit


# ---- truth rays: unnormalised directions ------------------------------------------------
def truth_rays(bits, n=N_TRUTH):
    """(orig (n, 3), dir (n, 3)) on subset `bits`, built as
    truth_cases.make_rays builds its rays (seed 900 + bits, origins above the
    ground) except that every direction points at a random point of the
    scene's bounds; the directions are normalised, then scaled by the cycle
    0.25, 0.5, 1, 3."""
    lo, hi = tc.bounds(subset_scene(bits))
    rng = np.random.default_rng(900 + bits)
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    orig[:, 1] = 0.25 + np.abs(orig[:, 1])          # above the ground
    d = rng.uniform(lo, hi, (n, 3)) - orig
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.resize(TRUTH_SCALES, n)[:, None]
    return np.ascontiguousarray(orig), np.ascontiguousarray(d)


def truth_shade(bits, idx=None):
    """truth_shade_<bits>.npz (its rays idx): the rays, per ray the colour
    rounded to float64, the Counts (primary, tests, hits, shadow, reflection),
    the primary hit's object, both margins and the float32 query margins
    (truth.Margin.h32, n32: a radiance is decided at normal32)."""
    mp = truth._mp()
    orig, d = truth_rays(bits)
    idx = np.arange(len(orig)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(subset_scene(bits))
    rgb, counts, obj, margin, margin32, hit32, normal32 = [], [], [], [], [], [], []
    for i in idx:
        st, mg = truth.Counts(), truth.Margin()
        o, dd = truth._vec(orig[i]), truth._vec(d[i])
        st.primary += 1
        ob, face, t, tests, hits = truth._trace(ts, o, dd, mp.inf, mg)
        st.tests += tests
        st.hits += hits
        col = truth.shade(ts, o, dd, ob, face, t, 1, mp.mpf(float(BIAS)), DEPTH, st, mg)
        rgb.append([float(x) for x in col])
        counts.append(st.tuple())
        obj.append(ob)
        margin.append(mg.m)
        margin32.append(mg.m32)
        hit32.append(mg.h32)
        normal32.append(mg.n32)
    return {"orig": orig[idx], "dir": d[idx], "rgb": np.array(rgb, np.float64), "counts": np.array(counts, np.int64),
            "obj": np.array(obj, np.int32), "margin": np.array(margin, np.float64),
            "margin32": np.array(margin32, np.float64), "hit32": np.array(hit32, np.float64),
            "normal32": np.array(normal32, np.float64)}
