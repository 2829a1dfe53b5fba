"""Scenes at the counts where the render kernels and the per-call build change
behaviour (DESIGN.md "Count limits"): shared by test_gpu_capacity.py and
test_capacity_scenes_cpu.py (which proves, on the oracle alone, that every
object and every light of every scene decides pixels of its frame, so that a
guard wrong at one count cannot leave the frame as it was).

SCENES maps a name to a builder `f(dcam=0.0)`; `dcam` moves the camera as
subset_scenes.subset_scene does. Nothing here draws a random number.

* lights-mesh-<n>: the 576-face torus on the y = 0 plane under n distant
  lights, n in 4, 8, 9, 32, 33; -8p7 has a point light at index 7, -33p8p32
  at indices 8 and 32;
* lights-warm-<n>: scenes.spheres_warm's objects under n = 8, 9, 33 lights;
* objects-<n>: the ground at index 0, then n - 1 spheres and boxes
  alternating on a lattice that recedes from the camera, n in 3, 4, 16, 17,
  64, 65, 130;
* mesh-first-<n> / mesh-last-<n>: the torus, the ground and n - 2 spheres,
  n in 16, 17, 64, 65, the mesh at index 0 or at index n - 1;
* mirror-last: objects-65 with its plane at index 64 and reflective, and
  three reflective spheres, rendered at maxRayDepth 3;
* planes-<p>: the torus, the ground and p - 1 further planes, p in 8, 9.

Lights: light k of n shines down a cone about -y, at azimuth 360 k / n + 17
degrees and 30, 40 or 50 degrees off the axis (k mod 3), in a colour of its
own, with intensity TOTAL / n times 0.7 .. 1.3 by index, so a frame is as
bright at 33 lights as at 4."""
import functools
import math

import numpy as np

from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.scene import akJittered
from rtmi.glm import X_AXIS, Y_AXIS, Z_AXIS, degToRad, inverse, mat4, point, rotate, translate, vec, vec3
from rtmi.scene import DistantLight, Material, Object, PointLight, Scene, initBox, initPlane, initSphere
from subset_scenes import SHIFT, smooth_mask

W, H, BIAS = 64, 48, 1e-4
SMALL = (48, 32)            # the 33-light frames: 34 rays a sample
TOTAL = 5.0                 # summed intensity of a light set: scenes._warm_lights' 4 + 1
POINT_DIST = 14.0           # a point light stands this far up its direction from the scene's middle
MIDDLE = (0.0, 2.0, -12.0)
STOCHASTIC = akJittered

LIGHT_COUNTS = (4, 8, 9, 32, 33)
WARM_COUNTS = (8, 9, 33)
OBJECT_COUNTS = (3, 4, 16, 17, 64, 65, 130)
MESH_COUNTS = (16, 17, 64, 65)
PLANE_COUNTS = (8, 9)


# ---- lights ---------------------------------------------------------------------
def light_dir(k, n):
    az = math.radians(360.0 * k / n + 17.0)
    off = math.radians((30.0, 40.0, 50.0)[k % 3])
    return np.array([math.sin(off) * math.cos(az), -math.cos(off), math.sin(off) * math.sin(az), 0.0])


def light_color(k, n):
    ph = 2.0 * math.pi * k / n
    return vec3(*(0.6 + 0.4 * math.cos(ph + s) for s in (0.0, 2.1, 4.2)))


def light_intensity(k, n):
    spread = 0.0 if n == 1 else 0.3 * (2.0 * ((k * 7) % n) / (n - 1) - 1.0)
    return TOTAL / n * (1.0 + spread)


def cone_lights(n, points=()):
    """n lights; those at the indices `points` are point lights POINT_DIST up
    their direction from MIDDLE, as bright there as the distant light would be."""
    out = []
    for k in range(n):
        d, c, i = light_dir(k, n), light_color(k, n), light_intensity(k, n)
        if k in points:
            pos = np.asarray(MIDDLE) - POINT_DIST * d[:3]
            out.append(PointLight(color=c, intensity=i * 4.0 * math.pi * POINT_DIST ** 2, pos=point(*pos)))
        else:
            out.append(DistantLight(color=c, intensity=i, dir=d))
    return out


TWO_LIGHTS = (  # the object and plane axes
    dict(color=(1.0, 0.95, 0.9), intensity=2.6, dir=(-0.8, -1.0, -0.4)),
    dict(color=(0.5, 0.7, 1.0), intensity=1.4, dir=(0.7, -1.0, 0.5)),
)


def two_lights(spec=TWO_LIGHTS):
    out = []
    for s in spec:
        d = np.array(s["dir"] + (0.0,))
        out.append(DistantLight(color=vec3(*s["color"]), intensity=s["intensity"], dir=d / np.linalg.norm(d)))
    return out


# ---- objects ---------------------------------------------------------------------
def _moved(cam, dcam):
    cam = np.array(cam, np.float64)
    cam[3, :3] += np.asarray(dcam, np.float64) * ((1.0, 1.0, -1.0) if np.ndim(dcam) == 0 else 1.0)
    return cam


def _scene(objects, lights, cam, dcam, fov=50.0):
    return Scene(objects=objects, lights=lights, fov=fov, cameraToWorld=_moved(cam, dcam),
                 bgColor=vec3(0.01, 0.03, 0.05))


def _ground(reflection=0.0):
    return Object("ground", initPlane(objectToWorld=mat4(1.0)), Material(albedo=vec3(0.4), reflection=reflection))


def _torus(at=(0.0, 1e-4, -12.0), size=1.0):
    mesh = scenes.torus_mesh(24, 12, R=3.0 * size, r=size)  # size 1: test_gpu_relight._small_torus
    mesh.objectToWorld = translate(mat4(1.0), vec3(*at))
    mesh.worldToObject = inverse(mesh.objectToWorld)
    return Object("torus", mesh, Material(albedo=vec3(0.9, 0.5, 0.2)))


def _camera(tilt, x, y, z):
    """Looks along -z turned `tilt` degrees down, from (x, y, z)."""
    m = np.array(rotate(mat4(1.0), X_AXIS, degToRad(-tilt)), np.float64)
    m[3, :3] = (x, y, z)
    return m


MESH_CAMERA = _camera(38.0, 0.0, 15.0, 4.0)
WARM_CAMERA = _camera(50.0, 1.0, 30.0, 6.0)


def lights_mesh(n, points=(), dcam=0.0):
    return _scene([_torus(), _ground()], cone_lights(n, points), MESH_CAMERA, dcam)


def lights_warm(n, dcam=0.0):
    sc = scenes.spheres_warm()
    return _scene(sc.objects, cone_lights(n), WARM_CAMERA, dcam)


# Two lattices that recede from the camera, seen from above through a long lens: the spheres (radius 0.5,
# strong colours) COLS a row, and behind them the boxes, SLAB_COLS a row. The boxes are slabs SLAB_TOP high
# within 0.0015 of the ground's albedo: 129 objects in strong relief would leave no smooth pixels in a
# 64 x 48 frame, while a slab that goes missing, or whose shadow does, moves smooth pixels, which are held
# to 1e-4, by 1e-3 and more. (A sample that float32 rounding puts on the other side of a slab's edge moves
# its pixel by 0.0012 / 16 at most, below that bound.)
COLS, PITCH_X, PITCH_Z, Z0 = 13, 1.0, 1.18, -6.0
SLAB_COLS, SLAB_SCALE, SLAB_Z0 = 12, 1.5, -13.1
SLAB_HALF, SLAB_TOP, SLAB_DX = 0.68, 0.02, 0.0
LATTICE_FOV = 27.0
LATTICE_CAMERA = _camera(58.0, 0.0, 30.0, 6.5)


def _albedo(i, swing=0.25):
    return vec3(*(0.4 + swing * math.cos(0.9 * i + s) for s in (0.0, 2.1, 4.2)))


def sphere_xz(k):
    return (PITCH_X * (k % COLS - (COLS - 1) / 2.0), Z0 - PITCH_Z * (k // COLS))


def slab_xz(k):
    return (SLAB_DX + SLAB_SCALE * PITCH_X * (k % SLAB_COLS - (SLAB_COLS - 1) / 2.0),
            SLAB_Z0 - SLAB_SCALE * PITCH_Z * (k // SLAB_COLS))


def lattice_object(i, spheres_only=False, reflection=0.0):
    """Object i of a lattice scene: spheres and boxes alternating (spheres_only: sphere i)."""
    if spheres_only or i % 2 == 0:
        x, z = sphere_xz(i if spheres_only else i // 2)
        return Object(f"ball{i}", initSphere(r=0.5, objectToWorld=translate(mat4(1.0), vec3(x, 0.5, z))),
                      Material(albedo=_albedo(i), reflection=reflection))
    x, z = slab_xz(i // 2)
    box = initBox(objectToWorld=translate(mat4(1.0), vec3(x, 0.0, z)), vmin=vec(-SLAB_HALF, 0.0, -SLAB_HALF),
                  vmax=vec(SLAB_HALF, SLAB_TOP, SLAB_HALF))
    return Object(f"box{i}", box, Material(albedo=_albedo(i, 0.0015)))


def objects_scene(n, dcam=0.0):
    objs = [_ground()] + [lattice_object(i) for i in range(n - 1)]
    return _scene(objs, two_lights(), LATTICE_CAMERA, dcam, LATTICE_FOV)


MIRRORS = (6, 30, 58)  # lattice places of the three reflective spheres (even: spheres)


def mirror_last(dcam=0.0):
    objs = [lattice_object(i, reflection=0.5 if i in MIRRORS else 0.0) for i in range(64)]
    return _scene(objs + [_ground(reflection=0.3)], two_lights(), LATTICE_CAMERA, dcam, LATTICE_FOV)


MIRROR_DEPTH = 3

# the torus beside the lattice's spheres: the camera stands back to hold both
MESH_LATTICE_CAMERA = _camera(58.0, 0.0, 34.0, 6.0)
MESH_LATTICE_TORUS = (0.0, 1e-4, -16.5)


def mesh_objects_scene(n, mesh_last, dcam=0.0):
    balls = [lattice_object(i, spheres_only=True) for i in range(n - 2)]
    torus = _torus(MESH_LATTICE_TORUS, 0.65)
    objs = [_ground()] + balls + [torus] if mesh_last else [torus, _ground()] + balls
    return _scene(objs, two_lights(), MESH_LATTICE_CAMERA, dcam, LATTICE_FOV)


# further planes: (name, rotations (axis, degrees) applied in turn, a point of the plane)
_PLANES = (
    ("back", ((X_AXIS, 90.0),), (0.0, 0.0, -26.0)),
    ("left", ((Z_AXIS, -90.0), (Y_AXIS, -32.0)), (-15.0, 0.0, -12.0)),
    ("right", ((Z_AXIS, 90.0), (Y_AXIS, 32.0)), (15.0, 0.0, -12.0)),
    ("ceiling", ((X_AXIS, 145.0),), (0.0, 13.0, -26.0)),
    ("back-ramp", ((X_AXIS, 40.0),), (0.0, 0.0, -21.0)),
    ("left-ramp", ((Z_AXIS, -40.0), (Y_AXIS, -32.0)), (-11.0, 0.0, -12.0)),
    ("right-ramp", ((Z_AXIS, 40.0), (Y_AXIS, 32.0)), (11.0, 0.0, -12.0)),
    ("ceiling-ramp", ((X_AXIS, 118.0),), (0.0, 11.0, -26.0)),
)
PLANE_LIGHTS = (  # low, from behind the camera, where the planes leave the sky open
    dict(color=(1.0, 0.95, 0.9), intensity=2.6, dir=(-0.3, -0.45, -0.8)),
    dict(color=(0.5, 0.7, 1.0), intensity=1.4, dir=(0.35, -0.5, -0.8)),
)
PLANE_CAMERA = _camera(4.0, 0.0, 7.0, 8.0)


def _plane(name, turns, at, k):
    m = translate(mat4(1.0), vec3(*at))
    for axis, deg in reversed(turns):
        m = rotate(m, axis, degToRad(deg))
    return Object(name, initPlane(objectToWorld=m), Material(albedo=_albedo(3 * k + 1)))


def planes_scene(p, dcam=0.0):
    objs = [_ground()] + [_plane(*_PLANES[k], k) for k in range(p - 1)] + [_torus()]
    return _scene(objs, two_lights(PLANE_LIGHTS), PLANE_CAMERA, dcam)


def _named():
    out = {}
    for n in LIGHT_COUNTS:
        out[f"lights-mesh-{n}"] = functools.partial(lights_mesh, n, ())
    out["lights-mesh-8p7"] = functools.partial(lights_mesh, 8, (7,))
    out["lights-mesh-33p8p32"] = functools.partial(lights_mesh, 33, (8, 32))
    for n in WARM_COUNTS:
        out[f"lights-warm-{n}"] = functools.partial(lights_warm, n)
    for n in OBJECT_COUNTS:
        out[f"objects-{n}"] = functools.partial(objects_scene, n)
    for n in MESH_COUNTS:
        out[f"mesh-first-{n}"] = functools.partial(mesh_objects_scene, n, False)
        out[f"mesh-last-{n}"] = functools.partial(mesh_objects_scene, n, True)
    out["mirror-last"] = mirror_last
    for p in PLANE_COUNTS:
        out[f"planes-{p}"] = functools.partial(planes_scene, p)
    return out


SCENES = _named()
NAMES = tuple(SCENES)
LIGHT_MESH = tuple(n for n in NAMES if n.startswith("lights-mesh-"))
MIXED = ("lights-mesh-8p7", "lights-mesh-33p8p32")


def scene(name, dcam=0.0):
    return SCENES[name](dcam=dcam)


def size(name):
    return SMALL if len(scene(name).lights) >= 32 else (W, H)


def depth(name):
    return MIRROR_DEPTH if name == "mirror-last" else 5


def has_mesh(name):
    return name.startswith(("lights-mesh-", "mesh-", "planes-"))


def options(name, kind, m, prec=Precision.fp64, flags=0):
    w, h = size(name)
    return Options(width=w, height=h, antialias=Antialias(kind, m), bias=BIAS, maxRayDepth=depth(name),
                   precision=prec, flags=flags)


# ---- the oracle's frames: computed once, shared, read-only -------------------------
def _oracle_render(oracle_mod, sc, o, mesh):
    # (bvh=True: the brute-force face loop's answers and Stats from a per-ray float64 BVH)
    ref, st, _ = oracle_mod.OracleScene(sc, bvh=mesh).render(o)
    ref.setflags(write=False)
    return ref, st


@functools.lru_cache(maxsize=None)
def oracle_frame(oracle_mod, name, kind, m, dcam=0.0):
    return _oracle_render(oracle_mod, scene(name, dcam), options(name, kind, m), has_mesh(name))


@functools.lru_cache(maxsize=None)
def oracle_frames(oracle_mod, name, kind, m):
    """oracle_frame, its Stats, the frames from the cameras moved by +SHIFT
    and -SHIFT, and the smooth-pixel mask those three give."""
    ref, st = oracle_frame(oracle_mod, name, kind, m)
    shifted = tuple(oracle_frame(oracle_mod, name, kind, m, d)[0] for d in (SHIFT, -SHIFT))
    mask = smooth_mask(ref, shifted)
    mask.setflags(write=False)
    return ref, st, shifted, mask


@functools.lru_cache(maxsize=None)
def oracle_variant(oracle_mod, name, m, without_object=None, only_light=None, without_light=None):
    """The akGrid oracle frame of the scene less one object, under one of its
    lights alone, or less one light."""
    sc = scene(name)
    if without_object is not None:
        sc.objects = [o for i, o in enumerate(sc.objects) if i != without_object]
    if only_light is not None:
        sc.lights = [sc.lights[only_light]]
    if without_light is not None:
        sc.lights = [l for i, l in enumerate(sc.lights) if i != without_light]
    return _oracle_render(oracle_mod, sc, options(name, akGrid, m), has_mesh(name))[0]


@functools.lru_cache(maxsize=None)
def closest_hits(oracle_mod, name):
    """(h, w) object index under every pixel centre (-1: none): the oracle's trace."""
    sc = scene(name)
    w, h = size(name)
    osc = oracle_mod.OracleScene(sc, bvh=has_mesh(name))
    out = np.full((h, w), -1, np.int32)
    for y in range(h):
        for x in range(w):
            o, d = oracle_mod.cast_primary_ray(w, h, x + 0.5, y + 0.5, sc.fov, sc.cameraToWorld)
            out[y, x] = osc.trace(o, d)[0]
    out.setflags(write=False)
    return out
