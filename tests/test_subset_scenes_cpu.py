"""The scenes of tests/subset_scenes.py leave test_gpu_subsets.py room: on
the float64 oracle alone (no device), for every feature subset and every
sampling a float32 frame is compared at,

* at least 65 % of the pixels are smooth (subset_scenes.smooth_mask), so the
  1e-4 bound on smooth pixels speaks for most of the frame;
* the oracle itself, from a camera moved by 2^-16 (about 16 float32 ulps of
  the largest coordinate), leaves at most 7 pixels beyond 2e-3 and moves the
  frame's mean by at most 5e-5: a quarter of what the float32 tolerance
  (99.5 % of 6,144 pixels within 2e-3, mean 2e-4) allows a
  kernel whose inputs are rounded to float32;
* reflection rays are traced exactly when the reflect bit is set, and each
  scene has the features of its bits and no others.

The same for the recursion-limit scenes (subsets 35 and 39, maxRayDepth 0,
1, 2 and 7), whose reflection-ray count grows strictly with the depth."""
import numpy as np
import pytest

import subset_scenes as ss
from rtmi import akGrid
from rtmi.scene import Box, Plane, PointLight, Sphere, TriangleMesh

SMOOTH_SHARE = 0.65
BEYOND = 7        # pixels of 6,144 beyond 2e-3: a quarter of the 30 the tolerance allows
MEAN = 5e-5       # a quarter of 2e-4


def _room(oracle_mod, bits, kind, m, depth=5):
    ref, st, shifted, mask = ss.oracle_frames(oracle_mod, bits, kind, m, depth)
    what = (ss.subset_name(bits), int(kind), m, depth)
    share = float(mask.mean())
    moves = [ss.pixel_error(s, ref) for s in shifted]
    beyond = [int(np.count_nonzero(e > 2e-3)) for e in moves]
    mean = [float(e.mean()) for e in moves]
    print("subset", bits, *what, "smooth", round(share, 4), "beyond 2e-3", beyond, "mean", mean,
          "reflection rays", st.numReflectionRays)
    assert st.numPrimaryRays == ss.W * ss.H * m * m
    assert share >= SMOOTH_SHARE, (what, share)
    assert max(beyond) <= BEYOND, (what, beyond)
    assert max(mean) <= MEAN, (what, mean)
    return st


@pytest.mark.parametrize("bits", range(64))
def test_scene_has_exactly_its_features(bits):
    sc = ss.subset_scene(bits)
    geoms = [o.geometry for o in sc.objects]
    assert sum(isinstance(g, Plane) for g in geoms) == 1
    assert any(isinstance(g, Sphere) for g in geoms) == bool(bits & ss.SPHERE)
    assert any(isinstance(g, Box) for g in geoms) == bool(bits & ss.BOX)
    assert any(isinstance(g, TriangleMesh) for g in geoms) == bool(bits & ss.MESH)
    # a general transform: a linear part that is not the identity (csrc/rtmi.cpp classify_xf)
    general = [not np.array_equal(np.asarray(g.objectToWorld)[:3, :3], np.eye(3)) for g in geoms]
    assert any(general) == bool(bits & ss.XF_GENERAL)
    if bits & ss.XF_GENERAL and bits & ss.SPHERE:
        assert not all(g for g, o in zip(general, geoms) if isinstance(o, Sphere))  # both transform classes
    assert any(isinstance(li, PointLight) for li in sc.lights) == bool(bits & ss.POINT)
    assert any(o.material.reflection > 0.0 for o in sc.objects) == bool(bits & ss.REFLECT)
    moved = ss.subset_scene(bits, ss.SHIFT)
    d = np.asarray(moved.cameraToWorld) - np.asarray(sc.cameraToWorld)
    assert np.array_equal(d[3, :3], [ss.SHIFT, ss.SHIFT, -ss.SHIFT]) and not d[:3].any()


@pytest.mark.parametrize("bits", range(64))
def test_oracle_leaves_room(oracle_mod, bits):
    for kind, m in ss.fp32_samplings(bits):
        st = _room(oracle_mod, bits, kind, m)
        assert (st.numReflectionRays > 0) == bool(bits & ss.REFLECT), (bits, st)
        assert st.numShadowRays > 0


@pytest.mark.parametrize("bits", ss.DEPTH_BITS)
def test_recursion_scenes_leave_room(oracle_mod, bits):
    rays = {}
    for depth in range(8):
        if depth in ss.DEPTHS:
            rays[depth] = _room(oracle_mod, bits, akGrid, 4, depth).numReflectionRays
        else:
            rays[depth] = ss.oracle_frame(oracle_mod, bits, akGrid, 4, depth)[1].numReflectionRays
    print("subset", bits, "reflection rays by depth", rays)
    assert rays[0] == 0
    assert all(rays[d] < rays[d + 1] for d in range(7)), rays
