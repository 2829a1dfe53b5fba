"""Scenes whose float32 frames are exact integers: per pixel, the number of
samples that hit something. Shared by test_coverage_cpu.py (model against
oracle, on the CPU) and test_gpu_coverage.py (kernels against model).

Every scene has bgColor (1, 1, 1) and albedo (0, 0, 0) on every object, so a
sample that misses contributes exactly 1.0f and a sample that hits exactly
0.0f: every partial sum is an integer below 2^24, whatever the lane order,
the reduction or the fixed-point accumulation, and round(value * spp) is the
pixel's miss count (slats_mirror: reflection 0.5 under a sky of 1, so a hit
is exactly 0.5 and value = 1 - 0.5 * hits / spp). The camera is the identity
with fov = 90, so the sample at pixel position (px, py) looks along
((2 px/w - 1) * aspect * f, (1 - 2 py/h) * f, -1), f = tan(45 deg), and
which samples hit is plain float64 geometry (`classify`) on the positions
the reference's samplers give (`row_positions`: grid()'s formula, or
oracle.sample_table). The image is 33 x 19: neither side a multiple of a
wave tile (8x8 ... 2x1 pixels).

A sample whose ray passes within DELTA pixels of a silhouette edge (or of a
slat's inner diagonal, where a float32 ray may slip between the two
triangles) is undecided: it counts in k_hi but not in k_lo. A kernel's
integer must lie in [k_lo, k_hi] on every pixel; on the pixels without an
undecided sample that pins the count exactly, and with it where the kernel
put every sample and which sx it paired with which sy.

Scenes (`scene(name)`):
  slats         nine parallelogram slats (18 triangles) in the plane z = -1,
                turned 27 degrees: slanted edges make the count depend on
                the pairing of sx and sy. Mesh only.
  slats_mirror  the same with reflection 0.5.
  blocks        six boxes around z = -1.2, turned about Z by 17 + 23 k
                degrees (general transforms), and two spheres.
  blocks2       one of those boxes and one of the spheres.
  slats_ground  slats and a Plane at y = -1: the one-plane shape. The plane
                is hit where the ray points down, below image row h / 2.
"""
import functools
import math

import numpy as np

import oracle  # sample_table only
from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi.glm import Z_AXIS, degToRad, inverse, mat4, normalize, rotate, translate, vec, vec3
from rtmi.scene import (DistantLight, Material, Object, Scene, TriangleMesh, akCorrelatedMultiJittered, akJittered,
                        akMultiJittered, initBox, initPlane, initSphere)

W, H, BIAS = 33, 19, 1e-4
SEEDS = (99, 2 ** 40 + 7)
STOCHASTIC = (akJittered, akMultiJittered, akCorrelatedMultiJittered)
SCENES = ("slats", "slats_mirror", "blocks", "blocks2", "slats_ground")

# Exclusion distance in pixels (not a tolerance: a sample nearer than this to
# an edge is left out of k_lo and let into k_hi). The float32 kernels place a
# sample's ray within about 2e-5 pixel of the float64 one (position rounding
# at x <= 33: 2e-6; the normalised direction and the triangle, slab and
# sphere tests: a few ulps of 1 each), so 1e-3 leaves a factor of 50.
DELTA = 1e-3

_F = math.tan(90.0 * (math.pi / 180.0) / 2)  # castPrimaryRay's f
_R = W / H
_PIX = 2.0 * _F / H  # one pixel in world units on the plane z = -1 (2 r f / w is the same number)

# slats: local frame (u along a slat, v across), turned by _THETA in z = -1
_THETA = math.radians(27.0)
# (half length 0.9: with 0.8 only 24.6 % of the pixels are partly covered at akGrid m = 2, and
# test_coverage_cpu.py asks 25 %; the large box and sphere of the block scenes likewise give
# blocks2 its 8 %)
_PITCH, _HW, _HL, _OFF0 = 0.31, 0.085, 0.9, 0.013
_KS = range(-4, 5)

# blocks: (centre, angle about Z in degrees, half extents); spheres: (centre, radius)
_BOX_HALF, _BIG_HALF = (0.24, 0.15, 0.1), (0.55, 0.35, 0.1)
_BOXES = tuple(((x, y, -1.2), 17.0 + 23.0 * k, _BOX_HALF if k else _BIG_HALF)
               for k, (x, y) in enumerate(((-1.1, 0.5), (-1.45, -0.6), (-0.75, -0.65), (0.0, 0.65), (0.75, 0.5),
                                           (1.0, -0.55))))
_SPHERES = (((0.1, -0.4, -1.6), 0.6), ((1.6, 0.3, -1.4), 0.2))
_GROUND_Y = -1.0


def _slat_mesh():
    c, s = math.cos(_THETA), math.sin(_THETA)
    verts, faces = [], []
    for k in _KS:
        off = k * _PITCH + _OFF0
        base = len(verts)
        # counter-clockwise seen from +z: the single-sided triangle test faces the camera
        for u, v in ((-_HL, off - _HW), (_HL, off - _HW), (_HL, off + _HW), (-_HL, off + _HW)):
            verts.append((u * c - v * s, u * s + v * c, -1.0))
        faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)]  # the diagonal: corner 0 to corner 2
    return TriangleMesh(np.array(verts, np.float64), np.array(faces, np.int32))


def _box_xf(centre, deg):
    return rotate(translate(mat4(1.0), vec3(*centre)), Z_AXIS, degToRad(deg))


def _objects(name):
    black = lambda refl=0.0: Material(albedo=vec3(0.0), reflection=refl)  # noqa: E731
    if name in ("slats", "slats_mirror", "slats_ground"):
        objs = [Object("slats", _slat_mesh(), black(0.5 if name == "slats_mirror" else 0.0))]
        if name == "slats_ground":
            objs.append(Object("ground", initPlane(translate(mat4(1.0), vec3(0.0, _GROUND_Y, 0.0))), black()))
        return objs
    boxes = [Object(f"box{k}", initBox(vmin=vec(*[-e for e in half]), vmax=vec(*half), objectToWorld=_box_xf(c, deg)),
                    black()) for k, (c, deg, half) in enumerate(_BOXES)]
    balls = [Object(f"ball{k}", initSphere(r=r, objectToWorld=translate(mat4(1.0), vec3(*c))), black())
             for k, (c, r) in enumerate(_SPHERES)]
    if name == "blocks":
        return boxes[:3] + balls[:1] + boxes[3:] + balls[1:]
    assert name == "blocks2", name
    return [boxes[0], balls[0]]


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(objects=_objects(name),
                 lights=[DistantLight(color=vec3(1.0), intensity=3.0, dir=normalize(vec(0.0, -1.0, -1.0)))],
                 fov=90.0, cameraToWorld=mat4(1.0), bgColor=vec3(1.0))


def options(kind, m, seed=SEEDS[0], precision=Precision.fp32, flags=0, depth=5):
    return Options(width=W, height=H, antialias=Antialias(kind, 1 if kind == akNone else m), bias=BIAS,
                   maxRayDepth=depth, precision=precision, flags=flags, seed=seed)


def spp_of(kind, m):
    return 1 if kind == akNone else m * m


# ---- sample positions -------------------------------------------------------

def grid_offsets(m):
    """grid() (sampling.nim:5-18) as calcPixel walks it: entry j * m + i."""
    xs = 1.0 / m
    a = np.arange(m, dtype=np.float64) * xs + xs * 0.5
    return np.tile(a, m), np.repeat(a, m)


def pixel_offsets(kind, m, seed, x, y):
    """(sx, sy) inside pixel (x, y) of every sample, in the sampler's order."""
    if kind == akNone:
        return np.zeros(1), np.zeros(1)  # calcPixelNoSampling: the pixel's corner
    if kind == akGrid:
        return grid_offsets(m)
    return oracle.sample_table(kind, m, seed, x, y)


def row_positions(kind, m, seed, y, table=pixel_offsets):
    """(px, py), each (W, spp): the image positions of row y's samples."""
    px = np.empty((W, spp_of(kind, m)))
    py = np.empty_like(px)
    for x in range(W):
        sx, sy = table(kind, m, seed, x, y)
        px[x] = x + sx
        py[x] = y + sy
    return px, py


# ---- the float64 model ------------------------------------------------------

def _rays(px, py):
    """castPrimaryRay's direction before it is normalised: (cx, cy, -1)."""
    return ((2.0 * px * _R) / W - _R) * _F, (1.0 - 2.0 * py / H) * _F


def _slat_margin(cx, cy):
    """(margin, diag) in pixels: how far inside (+) or outside (-) the nearest
    slat the point (cx, cy, -1) lies, and its distance to that slat's diagonal."""
    c, s = math.cos(_THETA), math.sin(_THETA)
    u = cx * c + cy * s
    v = -cx * s + cy * c
    k = np.clip(np.rint((v - _OFF0) / _PITCH), _KS[0], _KS[-1])
    dv = v - (k * _PITCH + _OFF0)
    margin = np.minimum(_HW - np.abs(dv), _HL - np.abs(u))
    diag = np.abs((u + _HL) * (2 * _HW) - (dv + _HW) * (2 * _HL)) / math.hypot(2 * _HL, 2 * _HW)
    return margin / _PIX, diag / _PIX


def _box_margin(cx, cy, centre, deg, half):
    """By how much (pixels at the box's far face) the box must shrink for the
    ray to miss it (+), or grow for the ray to hit it (-): the slab test of
    AABB.intersect in object space, solved for the change of the half extents.
    Slab i is entered at near_i - e / |d_i| and left at far_i + e / |d_i| when
    the box grows by e; the ray hits while every entry precedes every exit."""
    w2o = inverse(_box_xf(centre, deg))
    o = w2o[3][:3]  # the camera (the origin) in object space
    d = [cx * w2o[0][i] + cy * w2o[1][i] - w2o[2][i] for i in range(3)]
    near, far, inv = [], [], []
    for i in range(3):
        di = np.where(np.abs(d[i]) < 1e-300, 1e-300, d[i])
        t0, t1 = (-half[i] - o[i]) / di, (half[i] - o[i]) / di
        near.append(np.minimum(t0, t1))
        far.append(np.maximum(t0, t1))
        inv.append(1.0 / np.abs(di))
    margin = np.full(np.shape(cx), np.inf)
    for i in range(3):
        for j in range(3):
            margin = np.minimum(margin, (far[j] - near[i]) / (inv[i] + inv[j]))
    assert (near[2] > 0).all()  # the box lies in front of the camera: a line that hits it hits it at t > 0
    return margin / (_PIX * (abs(centre[2]) + half[2]))


def _sphere_margin(cx, cy, centre, r):
    """Radius minus the distance of the centre from the ray, in pixels at the sphere's far side."""
    n2 = cx * cx + cy * cy + 1.0
    tca = (centre[0] * cx + centre[1] * cy - centre[2]) / np.sqrt(n2)
    d2 = centre[0] ** 2 + centre[1] ** 2 + centre[2] ** 2 - tca * tca
    return (r - np.sqrt(np.maximum(d2, 0.0))) / (_PIX * (abs(centre[2]) + r))


def _parts(name):
    """The scene's shapes as (kind, args, (centre, radius) of a bounding sphere or None)."""
    if name in ("slats", "slats_mirror"):
        return [("slats", (), None)]
    if name == "slats_ground":
        return [("slats", (), None), ("plane", (), None)]
    boxes = [("box", b, (b[0], math.sqrt(sum(e * e for e in b[2])))) for b in _BOXES]
    balls = [("sphere", s, s) for s in _SPHERES]
    return boxes + balls if name == "blocks" else [boxes[0], balls[0]]


def classify(name, px, py, delta=DELTA):
    """(sure_hit, may_hit) of the samples at image positions (px, py), arrays
    of shape (pixels, spp) whose row p lies inside one pixel."""
    sure = np.zeros(px.shape, bool)
    may = np.zeros(px.shape, bool)
    for what, args, ball in _parts(name):
        rows = slice(None)
        if ball is not None:
            # only the pixels whose rays can come near the shape: a pixel's rays stay within
            # 0.0745 (half its diagonal on z = -1) x depth of the ray through its middle
            mx, my = _rays(np.floor(px[:, 0]) + 0.5, np.floor(py[:, 0]) + 0.5)
            c, r = ball
            reach = math.sqrt(sum(e * e for e in c)) + r
            tca = (c[0] * mx + c[1] * my - c[2]) / np.sqrt(mx * mx + my * my + 1.0)
            dist = np.sqrt(np.maximum(sum(e * e for e in c) - tca * tca, 0.0))
            rows = np.flatnonzero(dist <= r + 0.1 * reach + 2 * delta)
            if rows.size == 0:
                continue
        cx, cy = _rays(px[rows], py[rows])
        diag = None
        if what == "slats":
            margin, diag = _slat_margin(cx, cy)
        elif what == "plane":
            # Plane.intersect: hit where the normalised direction's y is below -1e-6, which
            # is 2.3e-5 pixel below the horizon at most: far inside delta
            margin = -cy / _PIX
        elif what == "box":
            margin = _box_margin(cx, cy, *args)
        else:
            margin = _sphere_margin(cx, cy, *args)
        s = margin > delta
        if diag is not None:
            s &= diag > delta
        sure[rows] |= s
        may[rows] |= margin > -delta
    return sure, may


@functools.lru_cache(maxsize=None)
def _bounds(name, kind, m, seed, delta):
    k_lo = np.zeros((H, W), np.int64)
    k_hi = np.zeros((H, W), np.int64)
    for y in range(H):
        sure, may = classify(name, *row_positions(kind, m, seed, y), delta)
        k_lo[y] = sure.sum(axis=1)
        k_hi[y] = may.sum(axis=1)
    k_lo.setflags(write=False)
    k_hi.setflags(write=False)
    return k_lo, k_hi


def bounds(name, kind, m, seed=0, delta=DELTA):
    """(k_lo, k_hi), each (H, W): per pixel the samples that surely hit and
    those that may. Computed once per case, shared, read-only."""
    return _bounds(name, kind, m, seed if kind in STOCHASTIC else 0, delta)


def table_bounds(name, kind, m, seed, table, delta=DELTA):
    """bounds() of another sample table(kind, m, seed, x, y) -> (sx, sy): the mutants of the CPU file."""
    k_lo = np.zeros((H, W), np.int64)
    k_hi = np.zeros((H, W), np.int64)
    for y in range(H):
        sure, may = classify(name, *row_positions(kind, m, seed, y, table), delta)
        k_lo[y] = sure.sum(axis=1)
        k_hi[y] = may.sum(axis=1)
    return k_lo, k_hi


def undecided_share(name, kind, m, seed=0):
    k_lo, k_hi = bounds(name, kind, m, seed)
    return float((k_hi - k_lo).sum()) / (W * H * spp_of(kind, m))


def edge_distance(name, kind, m, seed, x, y, count):
    """For a pixel whose count left [k_lo, k_hi]: the smallest exclusion
    distance (pixels, of the ladder below) at which it would lie inside, i.e.
    how near an edge the samples in question are; inf when no distance up to
    1e-2 explains the count."""
    sx, sy = pixel_offsets(kind, m, seed, x, y)
    for d in (DELTA, 2e-3, 4e-3, 8e-3, 1e-2):
        sure, may = classify(name, (x + sx)[None, :], (y + sy)[None, :], d)
        if sure.sum() <= count <= may.sum():
            return d
    return math.inf


# ---- frames and counts ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_frame(name, kind, m, seed):
    o = options(kind, m, seed, Precision.fp64)
    ref, st, _ = oracle.OracleScene(scene(name)).render(o)
    ref.setflags(write=False)
    return ref, st


def oracle_frame(name, kind, m, seed=0):
    """The oracle's frame and Stats of a case: computed once, shared, read-only."""
    return _oracle_frame(name, kind, m, seed if kind in STOCHASTIC else SEEDS[0])


def hit_counts(name, frame, spp):
    """(hits, off): per pixel the hit count a frame of this scene encodes and
    how far value * spp lay from an integer; raises when the channels differ."""
    f = np.asarray(frame, np.float64)
    assert np.array_equal(f[..., 0], f[..., 1]) and np.array_equal(f[..., 0], f[..., 2]), "channels differ"
    scaled = (2.0 * (1.0 - f[..., 0]) if name == "slats_mirror" else 1.0 - f[..., 0]) * spp
    hits = np.rint(scaled)
    return hits.astype(np.int64), np.abs(scaled - hits)


# ---- the cases of the GPU file ----------------------------------------------

M_STOCHASTIC = (1, 2, 3, 5, 6, 8, 9, 11, 16, 23, 32)  # L = 1, 4, 4, 16, 32, 64 ...; 16-lane object batches at 8, 9, 11
M_GRID = (3, 5, 6, 7, 10, 12, 100, 255, 256)          # not powers of two (div_small), and the largest grids
M_JITTERED_BIG = (33, 100, 256)                       # above the table kinds' limit of 32
M_BOUNDS_ONLY = 100                                   # from here on no oracle frame: the bounds and the 1 % cap


def fp32_samplings():
    """(scene, kind, m, seed) of every float32 case of test_gpu_coverage.py,
    without the flags; a non-stochastic kind's seed is 0."""
    out = []
    for name in ("slats", "blocks"):
        out.append((name, akNone, 1, 0))
        for kind in STOCHASTIC:
            out += [(name, kind, m, seed) for m in M_STOCHASTIC for seed in SEEDS]
        out += [(name, akGrid, m, 0) for m in M_GRID]
        out += [(name, akJittered, m, SEEDS[k % 2]) for k, m in enumerate(M_JITTERED_BIG)]
    for k, m in enumerate((4, 9)):
        out.append(("blocks2", akGrid, m, 0))
        out += [("blocks2", kind, m, SEEDS[k]) for kind in STOCHASTIC]
    for k, m in enumerate((2, 8, 16)):
        out.append(("slats_mirror", akGrid, m, 0))
        out += [("slats_mirror", kind, m, SEEDS[k % 2]) for kind in STOCHASTIC[1:]]
    out += [("slats_ground", akGrid, m, 0) for m in (16, 32)]
    out += [("slats_ground", kind, 8, seed) for kind in STOCHASTIC[1:] for seed in SEEDS]
    return out


# float64, bit-exact against the oracle: the per-lane tables at m = 5, and the scratch cap
FP64_SAMPLINGS = tuple((name, kind, 5, SEEDS[k % 2]) for name in ("slats", "blocks")
                       for k, kind in enumerate(STOCHASTIC)) + (
    ("slats", akMultiJittered, 64, SEEDS[0]), ("slats", akCorrelatedMultiJittered, 256, SEEDS[1]))


def case_id(name, kind, m, seed, *more):
    return "-".join([name, f"k{int(kind)}", f"m{m}", f"s{SEEDS.index(seed) if seed in SEEDS else 0}", *more])
