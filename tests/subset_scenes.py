"""One scene for each of the 64 feature subsets the float32 render kernel is
specialised on (csrc/rt_common.h SUB_*, rt_kernels_f32_part.hip): shared by
test_gpu_subsets.py and test_subset_scenes_cpu.py (which proves, on the
oracle alone, that the scenes leave the comparisons of the GPU file room).

subset_scene(bits) has exactly the features of `bits` (SUB_* bit order; the
stochastic bit, 64, is an option of the call, not of the scene) and always a
ground plane:

* SPHERE: two spheres, of which only the first takes the general transform
  and the reflection, so one kernel sees both transform classes and both
  kinds of material;
* BOX: one box;
* MESH: a 256-face torus, standing on the ground, or lifted clear of it
  where the general transform turns it;
* XF_GENERAL: translate, rotate Y 35, rotate X -20, then a non-uniform
  scale (1.3, 0.8, 1.1) on the first sphere, the box and the mesh. The scale
  is what makes the reference's `objectToWorld * n`, never re-normalised
  (DESIGN.md (c)), differ from a unit normal. A scene of the plane alone
  tilts the plane instead;
* POINT: a point light in front of the distant one;
* REFLECT: reflection 0.5 on the first sphere, the box and the mesh, 0.3 on
  the ground.

`dcam` moves the camera by (+d, +d, -d): the CPU file and the smooth-pixel
mask of the GPU file render the oracle from cameras 2^-16 either side."""
import functools

import numpy as np

from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.scene import akCorrelatedMultiJittered, akJittered, akMultiJittered
from rtmi.glm import X_AXIS, Y_AXIS, degToRad, inverse, mat4, normalize, point, rotate, scale, translate, vec, vec3
from rtmi.scene import (DistantLight, Material, Object, PointLight, Scene, initBox, initPlane, initSphere)

SPHERE, BOX, MESH, XF_GENERAL, POINT, REFLECT, STOCHASTIC = 1, 2, 4, 8, 16, 32, 64  # rt_common.h SUB_*
NAMES = ("sphere", "box", "mesh", "general", "point", "reflect", "stochastic")

SHIFT = 2.0 ** -16  # about 16 float32 ulps of the scenes' largest coordinate (12)


def subset_name(bits):
    return "+".join(n for k, n in enumerate(NAMES) if bits >> k & 1) or "plane"


def _xf(general, tx, ty, tz):
    m = translate(mat4(1.0), vec3(tx, ty, tz))
    if general:
        m = rotate(m, Y_AXIS, degToRad(35.0))
        m = rotate(m, X_AXIS, degToRad(-20.0))
        m = scale(m, vec3(1.3, 0.8, 1.1))
    return m


def subset_scene(bits, dcam=0.0):
    assert 0 <= bits < 64
    gen = bool(bits & XF_GENERAL)
    refl = 0.5 if bits & REFLECT else 0.0
    objects = []
    if bits & SPHERE:
        objects.append(Object("ballA", initSphere(r=1.2, objectToWorld=_xf(gen, -3.5, 1.6, -11.0)),
                              Material(albedo=vec3(0.9, 0.3, 0.2), reflection=refl)))
        objects.append(Object("ballB", initSphere(r=0.8, objectToWorld=_xf(False, -1.0, 0.8, -8.0)),
                              Material(albedo=vec3(0.6, 0.9, 0.2))))
    if bits & BOX:
        objects.append(Object("box", initBox(objectToWorld=_xf(gen, 3.5, 1.4, -12.0), vmin=vec(-1.0, -1.0, -1.0),
                                             vmax=vec(1.0, 1.0, 1.0)),
                              Material(albedo=vec3(0.2, 0.5, 0.9), reflection=refl)))
    if bits & MESH:
        mesh = scenes.torus_mesh(16, 8, R=1.5, r=0.5)
        mesh.objectToWorld = _xf(gen, 0.5, 1.5 if gen else 1e-4, -11.0)
        mesh.worldToObject = inverse(mesh.objectToWorld)
        objects.append(Object("torus", mesh, Material(albedo=vec3(0.9, 0.5, 0.2), reflection=refl)))
    ground = mat4(1.0)
    if gen and not bits & (SPHERE | BOX | MESH):
        ground = rotate(rotate(ground, X_AXIS, degToRad(4.0)), Y_AXIS, degToRad(20.0))
    objects.append(Object("ground", initPlane(objectToWorld=ground),
                          Material(albedo=vec3(0.4), reflection=0.3 if bits & REFLECT else 0.0)))
    lights = [DistantLight(color=vec3(1.0), intensity=4.0, dir=normalize(vec(-2.0, -0.8, -0.3)))]
    if bits & POINT:
        lights.insert(0, PointLight(color=vec3(1.0, 1.0, 1.0), intensity=3000.0, pos=point(0.5, 12.0, -10.0)))
    cam = np.array(scenes._std_camera(0.0, 5.5, 1.5), np.float64)
    cam[3, :3] += np.asarray(dcam, np.float64) * ((1.0, 1.0, -1.0) if np.ndim(dcam) == 0 else 1.0)
    return Scene(objects=objects, lights=lights, fov=50.0, cameraToWorld=cam, bgColor=vec3(0.01, 0.03, 0.05))


W, H, BIAS = 96, 64, 1e-4
_KINDS = (akJittered, akMultiJittered, akCorrelatedMultiJittered)
# scene subsets whose flags-0 float32 call, at 64 samples per pixel, splits
# into the lean and the general-list kernels: a mesh, no point light, no reflection
LEAN_BITS = tuple(b for b in range(64) if b & MESH and not b & (POINT | REFLECT))

# the recursion limit: sphere + box + reflection, and the same with the mesh
DEPTH_BITS = (SPHERE | BOX | REFLECT, SPHERE | BOX | MESH | REFLECT)
DEPTHS = (0, 1, 2, 7)


def stochastic_kind(bits):
    return _KINDS[bits % 3]


def fp32_samplings(bits):
    """(kind, m) of every float32 comparison of subset `bits` with the oracle
    (test_gpu_subsets.py): akGrid and the subset's stochastic kind at m = 4,
    akGrid at m = 2, and for LEAN_BITS both kinds at m = 8 (one pixel per
    wave, where the two-class launch exists)."""
    s = [(akGrid, 4), (stochastic_kind(bits), 4), (akGrid, 2)]
    if bits in LEAN_BITS:
        s += [(akGrid, 8), (stochastic_kind(bits), 8)]
    return s


@functools.lru_cache(maxsize=48)
def oracle_frame(oracle_mod, bits, kind, m, depth=5, dcam=0.0):
    """The oracle's frame of subset `bits` at W x H and its Stats: computed
    once, shared, read-only."""
    o = Options(width=W, height=H, antialias=Antialias(kind, m), bias=BIAS, maxRayDepth=depth,
                precision=Precision.fp64)
    ref, st, _ = oracle_mod.OracleScene(subset_scene(bits, dcam)).render(o)
    ref.setflags(write=False)
    return ref, st


@functools.lru_cache(maxsize=16)
def oracle_frames(oracle_mod, bits, kind, m, depth=5):
    """oracle_frame, the frames from the cameras moved by +SHIFT and -SHIFT,
    and the smooth-pixel mask those three give."""
    ref, st = oracle_frame(oracle_mod, bits, kind, m, depth)
    shifted = tuple(oracle_frame(oracle_mod, bits, kind, m, depth, d)[0] for d in (SHIFT, -SHIFT))
    mask = smooth_mask(ref, shifted)
    mask.setflags(write=False)
    return ref, st, shifted, mask


def smooth_mask(ref, shifted, contrast=0.05, moves=1e-5):
    """Pixels of the oracle frame `ref` whose colour is decided well inside
    float32 resolution of the inputs: within `contrast` of each of its
    neighbours in every channel (8, fewer on the frame's border), and within
    `moves` of each of the `shifted` oracle frames (the same options from
    cameras moved by +-SHIFT)."""
    ref = ref.astype(np.float64)
    h, w, _ = ref.shape
    pad = np.pad(ref, ((1, 1), (1, 1), (0, 0)), mode="edge")
    ok = np.ones((h, w), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            ok &= (np.abs(pad[dy:dy + h, dx:dx + w] - ref) <= contrast).all(axis=2)
    for s in shifted:
        ok &= (np.abs(s.astype(np.float64) - ref) <= moves).all(axis=2)
    return ok


def pixel_error(got, ref):
    """Per pixel the largest channel error."""
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=2)
