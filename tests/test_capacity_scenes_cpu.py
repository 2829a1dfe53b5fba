"""The scenes of tests/capacity_scenes.py can fail: on the float64 oracle
alone (no device), for every scene of the catalogue,

* every object index is the closest hit of at least 4 pixel-centre camera
  rays (the oracle's trace), so a kernel that loses an object loses pixels;
* without object 15, 16, 63, 64 or the last one (those the scene has) the
  frame differs by more than 1e-3 at pixels whose closest hit is another
  object: the object's shadow, or its reflection, falls where a comparison
  sees it, so a shadow mask that forgets its bit changes the frame;
* every light alone lights ground pixels and leaves others in the shadow of
  the mesh or of an object (shadow rays from the ground's pixel centres, formed
  as shade forms them and traced by the oracle; the frame under that light
  alone is bright at the first and dark at the second), and the frame
  without that light differs from the full one by more than 1e-3 somewhere;
* at least 65 % of the pixels are smooth (subset_scenes.smooth_mask) at
  both samplings a float32 frame is compared at, the share
  test_subset_scenes_cpu.py requires."""
import numpy as np
import pytest

import capacity_scenes as cs
from rtmi import akGrid
from rtmi.scene import DistantLight, Plane, PointLight, TriangleMesh

SMOOTH_SHARE = 0.65
MIN_HITS = 4
EDGE_INDICES = (15, 16, 63, 64)
M = 4   # the sampling of the frames compared here


def _ground_index(sc):
    return next(i for i, o in enumerate(sc.objects) if o.name == "ground")


@pytest.mark.parametrize("name", cs.NAMES)
def test_scene_has_its_counts(name):
    sc = cs.scene(name)
    kind, _, count = name.rpartition("-")
    n_planes = sum(isinstance(o.geometry, Plane) for o in sc.objects)
    n_meshes = sum(isinstance(o.geometry, TriangleMesh) for o in sc.objects)
    assert n_meshes == (1 if cs.has_mesh(name) else 0)
    if kind in ("lights-mesh", "lights-warm"):
        n = int(count.split("p")[0])
        points = tuple(int(p) for p in count.split("p")[1:])
        assert len(sc.lights) == n
        assert tuple(i for i, l in enumerate(sc.lights) if isinstance(l, PointLight)) == points
        assert (name in cs.MIXED) == bool(points)
        # distinct directions, distinct colours, intensities TOTAL / n within 30 %
        d = np.array([cs.light_dir(k, n)[:3] for k in range(n)])
        c = np.array([np.asarray(l.color)[:3] for l in sc.lights])
        for a in (d, c):
            gap = np.abs(a[:, None] - a[None]).max(axis=2) + np.eye(n)
            assert gap.min() > 1e-2
        i = np.array([cs.light_intensity(k, n) for k in range(n)]) * n / cs.TOTAL
        assert i.min() == pytest.approx(0.7) and i.max() == pytest.approx(1.3)
        assert np.allclose(np.linalg.norm(d, axis=1), 1.0) and len({round(x, 6) for x in d[:, 1]}) == 3
    elif kind == "planes":
        assert n_planes == int(count) and len(sc.objects) == int(count) + 1 and len(sc.lights) == 2
    elif name == "mirror-last":
        assert len(sc.objects) == 65 and isinstance(sc.objects[64].geometry, Plane)
        assert sc.objects[64].material.reflection > 0.0
        assert sum(o.material.reflection > 0.0 for o in sc.objects[:64]) == 3 and cs.depth(name) == 3
    else:
        assert len(sc.objects) == int(count) and len(sc.lights) == 2 and n_planes == 1
        if kind == "objects":
            assert isinstance(sc.objects[0].geometry, Plane)
        else:
            at = 0 if kind == "mesh-first" else int(count) - 1
            assert isinstance(sc.objects[at].geometry, TriangleMesh)
    assert all(isinstance(l, (DistantLight, PointLight)) for l in sc.lights)
    w, h = cs.size(name)
    assert w <= 64 and h <= 48 and cs.BIAS == 1e-4
    if len(sc.lights) >= 33:
        assert (w, h) == (48, 32)
    moved = cs.scene(name, cs.SHIFT)
    d = np.asarray(moved.cameraToWorld) - np.asarray(sc.cameraToWorld)
    assert np.array_equal(d[3, :3], [cs.SHIFT, cs.SHIFT, -cs.SHIFT]) and not d[:3].any()


@pytest.mark.parametrize("name", cs.NAMES)
def test_every_object_is_seen(oracle_mod, name):
    sc = cs.scene(name)
    hits = cs.closest_hits(oracle_mod, name)
    seen = np.bincount(hits[hits >= 0], minlength=len(sc.objects))
    print(name, "fewest pixel centres on an object:", int(seen.min()), "object", int(seen.argmin()))
    assert seen.min() >= MIN_HITS, (name, int(seen.argmin()), int(seen.min()))


@pytest.mark.parametrize("name", cs.NAMES)
def test_edge_objects_decide_other_objects_pixels(oracle_mod, name):
    sc = cs.scene(name)
    n = len(sc.objects)
    hits = cs.closest_hits(oracle_mod, name)
    full = cs.oracle_frame(oracle_mod, name, akGrid, M)[0].astype(np.float64)
    for k in sorted({i for i in EDGE_INDICES + (n - 1,) if i < n}):
        less = cs.oracle_variant(oracle_mod, name, M, without_object=k).astype(np.float64)
        others = (hits >= 0) & (hits != k)
        d = np.abs(less - full).max(axis=2)
        print(name, "without object", k, "pixels of other objects that change:",
              int(np.count_nonzero(d[others] > 0)), "most", float(d[others].max()))
        assert d[others].max() > 1e-3, (name, k)


def _shadow_classes(oracle_mod, name):
    """Per light: (ground pixels it lights, ground pixels in another object's shadow)."""
    sc = cs.scene(name)
    w, h = cs.size(name)
    osc = oracle_mod.OracleScene(sc, bvh=cs.has_mesh(name))
    g = _ground_index(sc)
    hits = cs.closest_hits(oracle_mod, name)
    lit = np.zeros((len(sc.lights), h, w), bool)
    dark = np.zeros((len(sc.lights), h, w), bool)
    for y, x in np.argwhere(hits == g):
        o, d = oracle_mod.cast_primary_ray(w, h, x + 0.5, y + 0.5, sc.fov, sc.cameraToWorld)
        ob, t, tri, _ = osc.trace(o, d)
        p = o[:3] + d[:3] * t
        nrm = osc.hit_normal(o, d, ob, t, tri)[:3]
        for k, L in enumerate(sc.lights):
            if isinstance(L, DistantLight):
                to_light, dist = -np.asarray(L.dir, np.float64)[:3], float("inf")
            else:
                v = p - np.asarray(L.pos, np.float64)[:3]
                dist = float(np.linalg.norm(v))
                to_light = -v / dist
            s = osc.trace(np.append(p + nrm * cs.BIAS, 1.0), np.append(to_light, 0.0), dist)[0]
            lit[k, y, x] = s < 0
            dark[k, y, x] = s >= 0 and s != g
    return lit, dark


@pytest.mark.parametrize("name", cs.NAMES)
def test_every_light_lights_and_shadows_the_ground(oracle_mod, name):
    sc = cs.scene(name)
    full = cs.oracle_frame(oracle_mod, name, akGrid, M)[0].astype(np.float64)
    lit, dark = _shadow_classes(oracle_mod, name)
    for k in range(len(sc.lights)):
        assert lit[k].sum() >= MIN_HITS and dark[k].sum() >= MIN_HITS, (name, k, int(lit[k].sum()), int(dark[k].sum()))
        alone = cs.oracle_variant(oracle_mod, name, M, only_light=k).astype(np.float64).sum(axis=2)
        # (pixel centres class the pixels; the frame averages M x M samples a pixel)
        assert np.median(alone[lit[k]]) > np.median(alone[dark[k]]), (name, k)
        less = cs.oracle_variant(oracle_mod, name, M, without_light=k).astype(np.float64)
        assert np.abs(less - full).max() > 1e-3, (name, k)
    if len(sc.lights) > 1:
        # swapping two lights' places changes the frame: each has a colour of its own
        a, b = sc.lights[0], sc.lights[-1]
        assert np.abs(np.asarray(a.color) * a.intensity - np.asarray(b.color) * b.intensity).max() > 1e-2


@pytest.mark.parametrize("name", cs.NAMES)
def test_most_pixels_are_smooth(oracle_mod, name):
    w, h = cs.size(name)
    for m in (4, 8):
        ref, st, shifted, mask = cs.oracle_frames(oracle_mod, name, akGrid, m)
        share = float(mask.mean())
        print(name, "m", m, "smooth", round(share, 4), "brightest", float(ref.max()))
        assert st.numPrimaryRays == w * h * m * m
        assert st.numShadowRays > 0
        assert (st.numReflectionRays > 0) == (name == "mirror-last")
        assert share >= SMOOTH_SHARE, (name, m, share)
