"""Device ray queries (rt_trace_rays* / rt_pick_pixels*, DeviceScene.trace_rays
/ pick): every answer against the oracle's trace (renderer.nim:47-67) and
castPrimaryRay — objects and faces equal, t equal bit for bit, the summed
Stats equal — over seeded incoherent batches, the batch sizes around a wave
and a block, the edges of the rule (signed zeros, the mesh's AABB gate, exact
ties, the plane's 1e-6 threshold, t_near at and just past a hit), any-hit,
the coherence sort, hit normals, picking, and the calls' bookkeeping (no
side effects on the render state, the asynchronous form, released scratch)."""
import ctypes as C
import functools

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, glm, scenes
from rtmi._lib import RtmiError, lib
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH
from rtmi.renderer import DeviceScene
from rtmi.scene import Box, Material, Object, Plane, Scene, Sphere, TriangleMesh, initBox, initPlane, initSphere

from bvh_corpus import coincident as _coincident, flat_grid as _flat_grid
from query_checks import INF, Got, Ref, _dev, check, check_stats, same_bits, trace

pytestmark = pytest.mark.gpu

N_RAYS = 2000
SCALES = (0.01, 1.0, 100.0)


def _torus_scene():
    return scenes._mesh_scene(scenes.torus_mesh(48, 24), "torus", (0.9, 0.5, 0.2))


SCENES = {
    "mesh_mix": scenes.mesh_mix,
    "two_meshes": scenes.two_meshes,
    "spheres_warm3": lambda: scenes.spheres_warm(3),
    "boxes2": scenes.boxes2,
    "boxtest": scenes.boxtest,
    "torus": _torus_scene,
}
HAS_MESH = {"mesh_mix", "two_meshes", "torus"}
# the seeds the hit / miss condition of test 1 was checked with (CPU, oracle only)
SEEDS = {"mesh_mix": 11, "two_meshes": 12, "spheres_warm3": 13, "boxes2": 14, "boxtest": 15, "torus": 16}
PARITY_CASES = [(n, b) for n in SCENES for b in ((RT_BVH_SAH, RT_BVH_PLOC) if n in HAS_MESH else (RT_BVH_SAH,))]


# ---- rays and the oracle's answers (computed once, shared, never modified) ----
def _bounds(scene):
    """World AABB of the scene's bounded objects (everything but planes)."""
    pts = []
    for o in scene.objects:
        g = o.geometry
        if isinstance(g, Plane):
            continue
        if isinstance(g, Sphere):
            c = np.array([0.0, 0.0, 0.0, 1.0]) @ g.objectToWorld
            pts += [c[:3] - g.r, c[:3] + g.r]
        elif isinstance(g, Box):
            for k in range(8):
                p = np.array([(g.vmax if k & 1 else g.vmin)[0], (g.vmax if k & 2 else g.vmin)[1],
                              (g.vmax if k & 4 else g.vmin)[2], 1.0])
                pts.append((p @ g.objectToWorld)[:3])
        elif isinstance(g, TriangleMesh):
            v = np.concatenate([g.vertices, np.ones((len(g.vertices), 1))], 1) @ g.objectToWorld
            pts += [v[:, :3].min(0), v[:, :3].max(0)]
    pts = np.array(pts)
    return pts.min(0), pts.max(0)


def make_rays(name, n=N_RAYS):
    """n seeded rays: origins in a box 3x the scene's extent, unit directions
    towards random points of the scene's bounds for three quarters of them,
    random for the rest."""
    scene = SCENES[name]()
    lo, hi = _bounds(scene)
    rng = np.random.default_rng(SEEDS[name])
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    d = rng.uniform(lo, hi, (n, 3)) - orig
    rnd = rng.normal(0.0, 1.0, (n, 3))
    free = np.arange(n) % 4 == 3
    d[free] = rnd[free]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(orig), np.ascontiguousarray(d)


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    import oracle
    return oracle.OracleScene(SCENES[name]())


@functools.lru_cache(maxsize=None)
def rays(name):
    return make_rays(name)


@functools.lru_cache(maxsize=None)
def ref(name, scale):
    orig, d = rays(name)
    return Ref(_oracle_scene(name), orig, d * scale)


@functools.lru_cache(maxsize=None)
def device_scene(name, builder=RT_BVH_SAH):
    return DeviceScene(SCENES[name](), bvh_builder=builder)


# ---- 1. oracle parity ----------------------------------------------------------
@pytest.mark.parametrize("name,builder", PARITY_CASES)
def test_oracle_parity(gpu, oracle_mod, name, builder):
    orig, d = rays(name)
    ds = device_scene(name, builder)
    for scale in SCALES:
        want = ref(name, scale)
        # from the oracle's answers alone: the batch is neither all hits nor all misses
        hit = float((want.obj >= 0).mean())
        assert hit >= 0.25 and 1.0 - hit >= 0.10, (name, scale, hit)
        got = trace(ds, orig, d * scale)
        check(got, want)
        check_stats(got, want)
    if name in HAS_MESH:
        assert (ref(name, 1.0).face >= 0).sum() >= 50  # mesh faces are among the answers


# ---- 2. wave and block edges ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_batch_sizes(gpu, oracle_mod, n):
    orig, d = rays("mesh_mix")
    want = ref("mesh_mix", 1.0)
    got = trace(device_scene("mesh_mix"), orig[:n], d[:n])
    sel = slice(0, n)
    assert len(got.t) == n
    assert np.array_equal(got.obj, want.obj[sel]) and np.array_equal(got.face, want.face[sel])
    assert same_bits(got.t, want.t[sel])
    check_stats(got, want, sel)


def test_waves_of_misses_next_to_a_wave_of_hits(gpu, oracle_mod):
    """257 rays: after the first 64, every ray starts above the scene and
    points up and away from it."""
    orig, d = rays("mesh_mix")
    orig, d = orig[:257].copy(), d[:257].copy()
    lo, hi = _bounds(SCENES["mesh_mix"]())
    rng = np.random.default_rng(5)
    orig[64:, 1] = hi[1] + 1.0 + rng.uniform(0.0, 5.0, 257 - 64)
    up = rng.normal(0.0, 1.0, (257 - 64, 3))
    up[:, 1] = 1.0 + np.abs(up[:, 1])
    d[64:] = up / np.linalg.norm(up, axis=1, keepdims=True)
    want = Ref(_oracle_scene("mesh_mix"), orig, d)
    assert (want.obj[64:] == -1).all() and (want.obj[:64] >= 0).sum() >= 16
    got = trace(device_scene("mesh_mix"), orig, d)
    check(got, want)
    check_stats(got, want)


def degenerate_batch():
    """257 rays of the mesh_mix set, every other one degenerate: NaN origin,
    an infinite direction component, a zero direction, a NaN t_near, in turn."""
    orig, d = rays("mesh_mix")
    orig, d = orig[:257].copy(), d[:257].copy()
    tnear = np.full(257, INF)
    bad = np.arange(257) % 2 == 1
    for k, i in enumerate(np.flatnonzero(bad)):
        tnear[i] = 7.5 + k
        kind = k % 4
        if kind == 0:
            orig[i, k % 3] = np.nan
        elif kind == 1:
            d[i, k % 3] = -INF if k % 8 == 1 else INF
        elif kind == 2:
            d[i] = [0.0, -0.0, 0.0]
        else:
            tnear[i] = np.nan
    return orig, d, tnear, bad


def test_degenerate_rays_are_masked(gpu, oracle_mod):
    orig, d, tnear, bad = degenerate_batch()
    want = ref("mesh_mix", 1.0)
    ds = device_scene("mesh_mix")
    got = trace(ds, orig, d, tnear, normals=True)
    good = ~bad
    idx = np.flatnonzero(good)
    # the degenerate rays: a miss, their t_near echoed (NaN as NaN), nothing in the Stats
    assert (got.obj[bad] == -1).all() and (got.face[bad] == -1).all()
    assert same_bits(got.t[bad], tnear[bad])
    assert not got.normals[bad].any()
    # their neighbours: the oracle's answers, and what a batch without the others gives
    assert np.array_equal(got.obj[good], want.obj[idx]) and np.array_equal(got.face[good], want.face[idx])
    assert same_bits(got.t[good], want.t[idx])
    assert got.stats.numIntersectionTests == int(want.tests[idx].sum())
    assert got.stats.numIntersectionHits == int(want.hits[idx].sum())
    clean = trace(ds, orig[good], d[good], tnear[good], normals=True)
    assert same_bits(clean.t, got.t[good]) and np.array_equal(clean.obj, got.obj[good])
    assert np.array_equal(clean.face, got.face[good]) and same_bits(clean.normals, got.normals[good])
    assert clean.stats == got.stats


# ---- 3. edges of the rule ------------------------------------------------------
def _axis_rays(points):
    """Every axis direction with every sign of its two zero components, from every point."""
    dirs = []
    for axis in range(3):
        for s in (1.0, -1.0):
            for za in (0.0, -0.0):
                for zb in (0.0, -0.0):
                    v = [za, zb]
                    v.insert(axis, s)
                    dirs.append(v)
    dirs = np.array(dirs)
    o = np.repeat(np.asarray(points, np.float64), len(dirs), axis=0)
    return o, np.tile(dirs, (len(points), 1))


def _against_oracle(scene, orig, d, tnear=None, builders=(RT_BVH_SAH,)):
    import oracle
    want = Ref(oracle.OracleScene(scene), orig, d, tnear)
    for b in builders:
        got = trace(DeviceScene(scene, bvh_builder=b), orig, d, tnear)
        check(got, want)
        check_stats(got, want)
    return want


def test_axis_aligned_signed_zero_boxtest(gpu, oracle_mod):
    # the box is [-1, 1]^3 about (0, 1, -10): points facing it, points in the
    # planes of its faces (0 * inf slabs, the NaN-slab KAT), one inside it
    pts = [(0.3, 1.2, -5.0), (-5.0, 1.2, -10.3), (0.3, 8.0, -10.2), (1.0, 1.0, -5.0), (-1.0, 2.0, -4.0),
           (0.0, 0.0, -10.0), (6.0, 2.0, -11.0), (0.2, 1.1, -10.1), (0.5, -3.0, -9.5), (-1.0, 5.0, -9.0)]
    o, d = _axis_rays(pts)
    want = _against_oracle(scenes.boxtest(), o, d)
    assert (want.obj == 1).sum() >= 20 and (want.obj == 0).sum() >= 20 and (want.obj == -1).sum() >= 20


def test_axis_aligned_signed_zero_flat_grid(gpu, oracle_mod):
    # the grid spans x in [-3, 3], z in [-14, -10] at y = 1.5001: points above
    # it on vertex columns (shared edges: equal t, lowest face), between them,
    # beside it in its own plane, and below it (back faces: culled)
    xs = np.linspace(-3.0, 3.0, 33)
    pts = [(xs[4], 5.0, -12.0), (xs[9], 5.0, -10.0 - 4.0 * 5 / 32), (0.1, 6.0, -11.3), (-2.95, 4.0, -13.9),
           (3.0, 5.0, -14.0), (-6.0, 1.5001, -12.0), (0.0, 1.5001, -3.0), (0.3, 0.5, -12.2), (4.0, 7.0, -12.0)]
    o, d = _axis_rays(pts)
    want = _against_oracle(scenes._mesh_scene(_flat_grid(), "m", (0.7, 0.6, 0.5)), o, d,
                           builders=(RT_BVH_SAH, RT_BVH_PLOC))
    assert (want.face >= 0).sum() >= 12


def test_rays_starting_inside_a_mesh_box_miss_it(gpu, oracle_mod):
    scene = _torus_scene()
    lo, hi = _bounds(scene)  # the torus is the only bounded object
    rng = np.random.default_rng(21)
    o = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (300, 3))
    d = rng.normal(0.0, 1.0, (300, 3))
    want = _against_oracle(scene, o, d, builders=(RT_BVH_SAH, RT_BVH_PLOC))
    assert (want.obj != 0).all() and (want.face == -1).all()  # TriangleMesh.intersect's gate (geom.nim:340)
    assert (want.obj == 1).sum() >= 50


def test_coincident_faces_lowest_index_wins(gpu, oracle_mod):
    rng = np.random.default_rng(22)
    n = 200
    # towards the 64 copies (z = -12 in world space, facing +z) from in front,
    # mostly below the face that stands before them (y >= 1.5 at z = -11)
    tgt = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(1.05, 1.6, n), np.full(n, -12.0)], 1)
    o = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(0.8, 1.3, n), rng.uniform(-6.0, -2.0, n)], 1)
    want = _against_oracle(scenes._mesh_scene(_coincident(), "m", (0.7, 0.6, 0.5)), o, tgt - o,
                           builders=(RT_BVH_SAH, RT_BVH_PLOC))
    on_copies = (want.obj == 0) & (want.face < 64)
    assert on_copies.sum() >= 100 and (want.face[on_copies] == 0).all()


def test_plane_threshold(gpu, oracle_mod):
    """Plane.intersect answers only when |dot(n, dir)| > 1e-6 (geom.nim:243)."""
    ys = [1e-6, -1e-6, 9.9e-7, -9.9e-7, 1.0000000000000002e-6, -1.0000000000000002e-6, 2e-6, -2e-6, 0.0, -0.0,
          5e-7, 1e-3, -1e-3]
    o = np.array([[-20.0, 0.5, -3.0]] * len(ys) + [[3.0, -0.25, 4.0]] * len(ys))
    d = np.array([[1.0, y, 0.0] for y in ys] + [[0.0, y, -1.0] for y in ys])
    want = _against_oracle(scenes.boxtest(), o, d)
    assert (want.obj == 0).sum() >= 4 and (want.obj == -1).sum() >= 8


def test_t_near_at_and_just_past_the_hit(gpu, oracle_mod):
    orig, d = rays("mesh_mix")
    free = ref("mesh_mix", 1.0)
    sel = np.flatnonzero(free.obj >= 0)[:400]
    o, dd, t0 = orig[sel], d[sel], free.t[sel]
    osc, ds = _oracle_scene("mesh_mix"), device_scene("mesh_mix")
    # strict <: with t_near equal to the closest t nothing is hit
    at = trace(ds, o, dd, t0)
    want = Ref(osc, o, dd, t0)
    check(at, want)
    check_stats(at, want)
    assert (at.obj == -1).all() and same_bits(at.t, t0)
    # one ulp further it is hit again, the same answer as without a t_near
    past = np.nextafter(t0, INF)
    nx = trace(ds, o, dd, past)
    want = Ref(osc, o, dd, past)
    check(nx, want)
    check_stats(nx, want)
    assert np.array_equal(nx.obj, free.obj[sel]) and np.array_equal(nx.face, free.face[sel]) and same_bits(nx.t, t0)


# ---- 4. any-hit ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anyhit_tnear(name):
    t = ref(name, 1.0).t
    f = np.random.default_rng(SEEDS[name] + 100).uniform(0.5, 2.0, len(t))
    return f * t  # +inf where the unrestricted ray misses


@pytest.mark.parametrize("name", list(SCENES))
def test_any_hit(gpu, oracle_mod, name):
    orig, d = rays(name)
    tn = anyhit_tnear(name)
    want = Ref(_oracle_scene(name), orig, d, tn)
    assert 0.05 <= float((want.obj >= 0).mean()) <= 0.95
    got = trace(device_scene(name), orig, d, tn, any_hit=True)
    assert np.array_equal(got.obj >= 0, want.obj >= 0)
    check_stats(got, want)
    with pytest.raises(RtmiError) as e:
        device_scene(name).trace_rays(_dev(orig[:8]), _dev(d[:8]), any_hit=True, normals=True)
    assert e.value.code == abi.RT_E_INVALID


# ---- 5. sort -------------------------------------------------------------------
def _sorted_equals_unsorted(ds, orig, d, tnear=None):
    a = trace(ds, orig, d, tnear, normals=True)
    b = trace(ds, orig, d, tnear, normals=True, sort=True)
    assert a.raw() == b.raw()
    assert a.stats == b.stats
    return a


@pytest.mark.parametrize("name", ["mesh_mix", "torus"])
def test_sort_same_bytes(gpu, oracle_mod, name):
    orig, d = rays(name)
    got = _sorted_equals_unsorted(device_scene(name), orig, d)
    check(got, ref(name, 1.0))
    for n in (1, 65):
        _sorted_equals_unsorted(device_scene(name), orig[:n], d[:n])
    # one shared origin: the key falls back to the directions
    o1 = np.repeat(orig[:1], 500, axis=0)
    _sorted_equals_unsorted(device_scene(name), o1, d[:500])


def test_sort_degenerate_batch(gpu, oracle_mod):
    orig, d, tnear, bad = degenerate_batch()
    got = _sorted_equals_unsorted(device_scene("mesh_mix"), orig, d, tnear)
    assert (got.obj[bad] == -1).all() and same_bits(got.t[bad], tnear[bad])


# ---- 6. normals ----------------------------------------------------------------
def _normals_scene():
    """A plane (identity), a translated box, a translated mesh with explicit
    (not unit) face normals, a translated sphere, a rotated and scaled mesh
    with explicit normals."""
    tri = np.array([[-2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 3.0, 0.0],
                    [0.0, 3.0, 0.0], [2.0, 0.0, 0.0], [3.0, 3.5, -0.5]])
    fn = np.array([[0.3, 0.4, 1.2], [-0.25, 0.5, 2.0]])
    m1 = TriangleMesh(tri, np.arange(6, dtype=np.int32).reshape(2, 3), fn,
                      glm.translate(glm.mat4(1.0), glm.vec3(-6.0, 0.5, -10.0)))
    xf = glm.scale(glm.rotate(glm.translate(glm.mat4(1.0), glm.vec3(6.0, 1.0, -11.0)), glm.Y_AXIS, glm.degToRad(25.0)),
                   glm.vec3(1.5, 0.75, 1.25))
    m2 = TriangleMesh(tri, np.arange(6, dtype=np.int32).reshape(2, 3), fn, xf)
    objects = [
        Object("ground", initPlane(objectToWorld=glm.mat4(1.0)), Material(albedo=glm.vec3(0.4))),
        Object("box", initBox(objectToWorld=glm.translate(glm.mat4(1.0), glm.vec3(0.0, 1.0, -10.0)),
                              vmin=glm.vec(-1.0, -1.0, -1.0), vmax=glm.vec(1.0, 1.0, 1.0)),
               Material(albedo=glm.vec3(1.0))),
        Object("m1", m1, Material(albedo=glm.vec3(0.5))),
        Object("ball", initSphere(r=1.25, objectToWorld=glm.translate(glm.mat4(1.0), glm.vec3(0.5, 4.0, -9.0))),
               Material(albedo=glm.vec3(0.5))),
        Object("m2", m2, Material(albedo=glm.vec3(0.5))),
    ]
    return Scene(objects=objects, lights=scenes._warm_lights(), fov=50.0,
                 cameraToWorld=scenes._std_camera(0.0, 5.5, 1.5), bgColor=glm.vec3(0.01, 0.03, 0.05)), fn


def test_normals(gpu, oracle_mod):
    import oracle
    scene, fn = _normals_scene()
    rng = np.random.default_rng(31)
    n = 1500
    centres = np.array([[0.0, 0.0, -10.0], [0.0, 1.0, -10.0], [-6.0, 1.8, -10.0], [0.5, 4.0, -9.0], [6.5, 2.0, -11.0]])
    tgt = centres[np.arange(n) % 5] + rng.uniform(-0.8, 0.8, (n, 3))
    o = np.stack([rng.uniform(-8.0, 8.0, n), rng.uniform(1.0, 9.0, n), rng.uniform(-4.0, 2.0, n)], 1)
    d = tgt - o
    got = trace(DeviceScene(scene), o, d, normals=True)
    want = Ref(oracle.OracleScene(scene), o, d)
    check(got, want)
    N = got.normals
    hw = o + d * got.t[:, None]
    counts = [(got.obj == k).sum() for k in range(5)]
    assert min(counts) >= 30, counts
    assert not N[got.obj < 0].any()
    # plane under the identity: (0, 1, 0) exactly
    assert (N[got.obj == 0] == [0.0, 1.0, 0.0]).all()
    # translated box: geom.nim:370-379 restated (the same IEEE operations)
    k = got.obj == 1
    g = scene.objects[1].geometry
    ho = (0.0 + hw[k]) + g.worldToObject[3][:3]
    c = (g.vmin + g.vmax) * 0.5
    dd = (g.vmin - g.vmax) * 0.5
    q = np.trunc((ho - c) / np.abs(dd) * 1.000001)
    ln = np.sqrt(((0.0 + q[:, 0] * q[:, 0]) + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2] + 0.0)
    assert same_bits(N[k], 0.0 + q / ln[:, None])
    assert (np.abs(N[k]).sum(1) == 1.0).mean() > 0.9  # face interiors: an axis
    # translated mesh, explicit normals: the face's normal exactly
    k = got.obj == 2
    assert same_bits(N[k], fn[got.face[k]])
    # sphere: objectToWorld * normalize(hitO), within 1e-14 of the restatement
    k = got.obj == 3
    ho = hw[k] + scene.objects[3].geometry.worldToObject[3][:3]
    e = ho / np.linalg.norm(ho, axis=1, keepdims=True)
    assert np.abs(N[k] - e).max() <= 1e-14 * 1.0
    # rotated and scaled mesh: objectToWorld's 3x3 times the face's normal
    k = got.obj == 4
    e = fn[got.face[k]] @ scene.objects[4].geometry.objectToWorld[:3, :3]
    assert (np.abs(N[k] - e) <= 1e-14 * np.linalg.norm(e, axis=1, keepdims=True)).all()


# ---- 7. picking ----------------------------------------------------------------
def _pick_points(w, h):
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    grid = np.stack([X.ravel(), Y.ravel()], 1)
    rng = np.random.default_rng(41)
    extra = np.stack([rng.uniform(-0.5 * w, 1.5 * w, 200), rng.uniform(-0.5 * h, 1.5 * h, 200)], 1)
    return np.concatenate([grid, extra])


def _oracle_pick(oracle, osc, scene, w, h, xy, c2w=None, fov=None):
    c2w = scene.cameraToWorld if c2w is None else c2w
    fov = scene.fov if fov is None else fov
    o = np.empty((len(xy), 3))
    d = np.empty((len(xy), 3))
    for i, (x, y) in enumerate(xy):
        ro, rd = oracle.cast_primary_ray(w, h, float(x), float(y), fov, glm.flat(c2w))
        assert ro[3] == 1.0 and rd[3] == 0.0
        o[i], d[i] = ro[:3], rd[:3]
    return Ref(osc, o, d)


def test_picking(gpu, oracle_mod):
    import torch
    scene = scenes.mesh_mix()
    w, h = 48, 32
    opts = Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64)
    ds = DeviceScene(scene)
    osc = _oracle_scene("mesh_mix")
    xy = _pick_points(w, h)
    want = _oracle_pick(oracle_mod, osc, scene, w, h, xy)
    got = Got(ds.pick(opts, _dev(xy), stats=True))
    check(got, want)
    assert got.stats.numPrimaryRays == len(xy)
    assert got.stats.numIntersectionTests == int(want.tests.sum())
    assert got.stats.numIntersectionHits == int(want.hits.sum())
    assert 0.2 <= float((want.obj[:w * h] >= 0).mean()) <= 0.98
    # where a pick misses, the akNone float64 frame shows the background
    fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ds.render_device(opts, fb)
    frame = fb.view(h * w, 3).cpu().numpy()
    miss = got.obj[:w * h] < 0
    assert miss.any() and (frame[miss] == np.asarray(scene.bgColor, np.float32)).all()
    # degenerate points are answered as misses and not counted
    bad = np.concatenate([xy[:100], [[np.nan, 3.0], [2.0, np.inf], [-np.inf, np.nan]]])
    g2 = Got(ds.pick(opts, _dev(bad), stats=True))
    assert g2.stats.numPrimaryRays == 100
    assert (g2.obj[100:] == -1).all() and (g2.t[100:] == INF).all()
    assert np.array_equal(g2.obj[:100], got.obj[:100]) and same_bits(g2.t[:100], got.t[:100])
    # the answers follow the scene's camera
    cam = glm.translate(glm.rotate(glm.mat4(1.0), glm.X_AXIS, glm.degToRad(-20.0)), glm.vec3(1.5, 7.0, 3.0))
    ds.set_camera(cam, 35.0)
    sub = xy[::7]
    want2 = _oracle_pick(oracle_mod, osc, scene, w, h, sub, cam, 35.0)
    got2 = Got(ds.pick(opts, _dev(sub), stats=True))
    check(got2, want2)
    assert not (np.array_equal(want2.obj, want.obj[::7]) and same_bits(want2.t, want.t[::7]))
    # float64 only
    o32 = Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp32)
    with pytest.raises(RtmiError) as e:
        ds.pick(o32, _dev(xy[:4]))
    assert e.value.code == abi.RT_E_UNSUPPORTED


# ---- 8. no side effects, host forms ---------------------------------------------
def _last_stats(ds):
    st = abi.rt_stats()
    assert lib().rt_scene_last_stats(ds.h, C.byref(st)) == abi.RT_OK
    return st.as_dict()


def test_queries_leave_the_render_state_alone(gpu, oracle_mod):
    import torch
    scene = _torus_scene()
    ds = DeviceScene(scene)
    opts = Options(width=64, height=48, antialias=Antialias(akGrid, 4), bias=1e-4, precision=Precision.fp32)
    fb = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    before = (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds))
    assert before[3]["num_primary_rays"] == st.numPrimaryRays == 64 * 48 * 16
    orig, d = rays("torus")
    want = ref("torus", 1.0)
    o64 = Options(width=64, height=48, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64)
    xy = _pick_points(64, 48)[::5]
    dev = trace(ds, orig, d, normals=True, sort=True)
    pk = Got(ds.pick(o64, _dev(xy), normals=True, stats=True), True)
    assert (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds)) == before
    check(dev, want)
    fb2 = torch.zeros_like(fb)
    assert ds.render_device(opts, fb2) == st
    assert torch.equal(fb, fb2)
    # the host forms give the device forms' answers
    t, obj, face, nrm, hst = ds.trace_rays(orig, d, normals=True, stats=True)
    assert same_bits(t, dev.t) and np.array_equal(obj, dev.obj) and np.array_equal(face, dev.face)
    assert same_bits(nrm, dev.normals) and hst == dev.stats
    t, obj, face, nrm, hst = ds.pick(o64, xy, normals=True, stats=True, sort=True)
    assert same_bits(t, pk.t) and np.array_equal(obj, pk.obj) and np.array_equal(face, pk.face)
    assert same_bits(nrm, pk.normals) and hst == pk.stats
    # validation that needs a scene
    assert ds.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)[-1].numIntersectionTests == 0
    L = lib()
    hits = (abi.rt_hit * 4)()
    z = np.zeros(12)
    zp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert L.rt_trace_rays(ds.h, -1, zp, zp, None, 0, hits, None, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays(ds.h, 4, zp, zp, None, 0x4, hits, None, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays(ds.h, 4, None, zp, None, 0, hits, None, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays(ds.h, 4, zp, zp, None, 0, None, None, None) == abi.RT_E_INVALID
    assert L.rt_pick_pixels(ds.h, None, 4, zp, 0, hits, None, None) == abi.RT_E_INVALID
    assert L.rt_trace_rays(ds.h, 0, None, None, None, 0, None, None, None) == abi.RT_OK
    assert (ds.last_split(), ds.last_lean_kernel(), ds.last_batch()) == before[:3]


# ---- 9. the asynchronous form ----------------------------------------------------
def test_async_on_a_side_stream(gpu, oracle_mod):
    import torch
    orig, d = rays("mesh_mix")
    want = ref("mesh_mix", 1.0)
    ds = device_scene("mesh_mix")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o, dd = _dev(orig), _dev(d)
        t, obj, face = ds.trace_rays(o, dd, stream=s)  # out == NULL: enqueued only
        t2, obj2, face2 = ds.trace_rays(o, dd, sort=True, stream=s)
    s.synchronize()
    for res in ((t, obj, face), (t2, obj2, face2)):
        got = Got(list(res) + [None])
        check(got, want)


# ---- 10. scratch buffers are released ---------------------------------------------
def test_create_query_destroy_releases_memory(gpu, oracle_mod):
    import torch
    orig, d = rays("torus")
    o, dd = _dev(orig), _dev(d)
    scene = _torus_scene()

    def cycle():
        ds = DeviceScene(scene)
        ds.trace_rays(o, dd, sort=True, normals=True, stats=True)
        ds.trace_rays(orig[:300], d[:300], sort=True, stats=True)  # the host form's staging buffer too
        ds.close()

    cycle()  # first use: the runtime's own one-time allocations (code objects, queues)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(5):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print("free bytes before / after:", free0, free1)
    assert free1 == free0
