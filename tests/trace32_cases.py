"""The rays of the float32 ray-query tests (DeviceScene.trace_rays_f32 /
pick_f32): shared by test_gpu_trace32.py, which sends them to the device, and
test_trace32_cases_cpu.py, which proves on the oracle alone that rounding
them to float32 leaves the device comparisons room. Nothing here touches a
GPU.

* frame rays: the float64 castPrimaryRay rays of the 96 x 64 akGrid m = 2
  frame every subset scene shares (one camera), 24,576 of them, and their
  image positions;
* small rays: the 165 akNone rays of shade_cases.W1 x H1 (two full waves and
  a 37-lane tail)."""
import functools

import numpy as np

import shade_cases as sc
import subset_scenes as ss

M = 2
GEOMETRY_BITS = tuple(range(16))        # the subsets of {sphere, box, mesh, general transform}
PERTURB = 2.0 ** -20                    # relative, per direction component


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


@functools.lru_cache(maxsize=None)
def frame_rays64(oracle_mod):
    scene = ss.subset_scene(0)
    o, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, ss.W, ss.H, M)
    assert len(o) == ss.W * ss.H * M * M == 24576
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def frame_rays(oracle_mod):
    """frame_rays64 rounded to float32."""
    o, d = (f32(a) for a in frame_rays64(oracle_mod))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def frame_xy():
    """The image positions of frame_rays, exact in float32."""
    xy = np.array(sc.sample_xy(ss.W, ss.H, M), np.float64)
    assert np.array_equal(xy, xy.astype(np.float32).astype(np.float64))
    xy.setflags(write=False)
    return xy


@functools.lru_cache(maxsize=None)
def perturbed_dirs(oracle_mod):
    """frame_rays' directions, each component moved by a seeded relative
    amount of at most PERTURB, rounded to float32 again."""
    _, d = frame_rays(oracle_mod)
    u = np.random.default_rng(3220).uniform(-1.0, 1.0, d.shape)
    p = f32(d.astype(np.float64) * (1.0 + PERTURB * u))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def small_rays(oracle_mod):
    scene = ss.subset_scene(0)
    o, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, sc.W1, sc.H1)
    o, d = f32(o), f32(d)
    assert len(o) == 165
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def oracle_trace(oracle_mod, bits, orig, d):
    """(obj, face, t) of the oracle's trace on subset scene `bits`."""
    osc = oracle_mod.OracleScene(ss.subset_scene(bits))
    n = len(orig)
    obj, face, t = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
    o4 = np.concatenate([np.asarray(orig, np.float64), np.ones((n, 1))], 1)
    d4 = np.concatenate([np.asarray(d, np.float64), np.zeros((n, 1))], 1)
    for i in range(n):
        ob, ti, tri, _ = osc.trace(o4[i], d4[i])
        obj[i], t[i], face[i] = ob, ti, tri if ob >= 0 else -1
    return obj, face, t
