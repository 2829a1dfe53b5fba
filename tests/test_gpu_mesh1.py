"""Mesh pixels of one-plane launches (rt_fast.h gen1_batch): a sample slot whose
lit shadow origins all lie strictly inside the call's inset box skips the
mesh's box gate of every light (rt_bins_geom.h lemma 1, tests/test_mesh1_cpu.py),
and a batch whose samples all hit the mesh, every one inside, is shaded on a
straight path without the hit-kind selects.

Every comparison is for bit-identical frames and equal Stats between flags 0,
RT_FLAG_NO_MESH1 (the same kernels, every gate evaluated and every batch on
the general path), RT_FLAG_NO_GEN1 (gen_batch, which shares none of this
code) and RT_FLAG_NO_BINNING (the BVH for every ray: the anchor, itself
anchored on the oracle below). The flags-0 call's counters say which kernel
ran and how many batches took the straight path (last_mesh1)."""
import math

import numpy as np
import pytest

import cameras
from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.abi import (RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING, RT_FLAG_NO_GEN1, RT_FLAG_NO_MESH1, RT_FLAG_NO_MIX,
                      RT_FLAG_NO_REORDER)
from rtmi.glm import inverse, mat4, normalize, translate, vec, vec3
from rtmi.renderer import DeviceScene, band_rows
from rtmi.scene import DistantLight, Material, Object, Scene, TriangleMesh, initPlane
from test_gpu_oneplane import _through_scene

pytestmark = pytest.mark.gpu

W, H = 96, 64  # a wave is one pixel; m = 16 and 32: iters = 4 and 16 (iters % 4 == 0)
BIAS = 1e-4
MIX1 = 15      # last_lean_kernel: k_render_mix1


def _outward(v, f):
    """The faces wound so that their normals point away from the vertices' centre."""
    c = v.mean(axis=0)
    a, b, d = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, d - a), (a + b + d) / 3 - c) < 0
    f = f.copy()
    f[flip] = f[flip][:, ::-1]
    return f.astype(np.int32)


def sphere_mesh(radius=2.0, nlat=10, nlon=16, centre=(0.0, 0.0, 0.0), squash=1.0):
    """A latitude / longitude sphere about `centre` (object space); squash < 1 flattens it in y."""
    v = [(0.0, radius, 0.0)]
    for i in range(1, nlat):
        th = math.pi * i / nlat
        for j in range(nlon):
            ph = 2 * math.pi * j / nlon
            v.append((radius * math.sin(th) * math.cos(ph), radius * math.cos(th), radius * math.sin(th) * math.sin(ph)))
    v.append((0.0, -radius, 0.0))
    f = []
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon  # noqa: E731
    for j in range(nlon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(nlat - 1, j), ring(nlat - 1, j + 1)))
        for i in range(1, nlat - 1):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    v = np.array(v, np.float64) * np.array([1.0, squash, 1.0])
    f = _outward(v, np.array(f))
    return TriangleMesh(v + np.array(centre, np.float64), f, None, mat4(1.0))


def cube_mesh(half=1.5):
    """An axis-aligned cube: every face lies on the mesh's box."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])
    return TriangleMesh(v, _outward(v, f), None, mat4(1.0))


def lights(*dirs, raw=False):
    return [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=3.0 - k, dir=vec(*d) if raw else normalize(vec(*d)))
            for k, d in enumerate(dirs)]


WARM2 = ((-2.0, -0.8, -0.3), (1.5, -2.0, -1.0))


def scene(mesh, at=(0.0, 2.5, -12.0), plane_first=False, dirs=WARM2, raw=False, c2w=None):
    """`mesh` with its object-space origin at `at`, over the ground y = 0,
    from the standard camera (or c2w)."""
    mesh.objectToWorld = translate(mat4(1.0), vec3(*at))
    mesh.worldToObject = inverse(mesh.objectToWorld)
    objects = [Object("mesh", mesh, Material(albedo=vec3(0.9, 0.5, 0.2))),
               Object("ground", initPlane(mat4(1.0)), Material(albedo=vec3(0.4)))]
    return Scene(objects=objects[::-1] if plane_first else objects, lights=lights(*dirs, raw=raw), fov=50.0,
                 cameraToWorld=scenes._std_camera(0.0, 5.5, 1.5) if c2w is None else c2w,
                 bgColor=vec3(0.01, 0.03, 0.05))


def _opts(w, h, m, flags=0, bias=BIAS):
    # NO_REORDER as in test_gpu_split.py: small frames keep the two-class launch
    return Options(width=w, height=h, antialias=Antialias(akGrid, m), bias=bias, precision=Precision.fp32,
                   flags=flags | RT_FLAG_NO_REORDER)


def _whole(ds, o, fb):
    yield ds.render_device(o, fb)


class Counts:
    def __init__(self):
        self.general = self.batched = self.fallback = self.straight = 0
        self.kernels = set()

    def read(self, ds):
        self.general += ds.last_split()[1]
        b = ds.last_batch()
        self.batched += b[0]
        self.fallback += b[1]
        self.straight += ds.last_mesh1()
        self.kernels.add(ds.last_lean_kernel())

    def __repr__(self):
        return (f"general {self.general} batched {self.batched} fallback {self.fallback} straight {self.straight} "
                f"kernels {sorted(self.kernels)}")


def compare(sc, m, bias=BIAS, calls=_whole, rows=None, extra=0, what="", w=W, h=H):
    """Renders with flags `extra`, + NO_MESH1, + NO_GEN1 and NO_BINNING;
    asserts frames and Stats equal to the anchor's, that NO_MESH1 counts no
    straight batch and leaves the lists and the batched count alone. Returns
    the flags-`extra` calls' counters, summed."""
    import torch
    ds = DeviceScene(sc)
    res, cnts = [], []
    for flags in (extra, extra | RT_FLAG_NO_MESH1, extra | RT_FLAG_NO_GEN1, RT_FLAG_NO_BINNING):
        o = _opts(w, h, m, flags, bias)
        fb = torch.full(((rows or h) * w * 3,), -7.0, dtype=torch.float32, device="cuda")
        sts, cnt = [], Counts()
        for st in calls(ds, o, fb):  # a generator: the counters are read after each call
            sts.append(st)
            cnt.read(ds)
        res.append((fb, sts))
        cnts.append(cnt)
    print(what, m, cnts)
    ref, rsts = res[-1]
    for k, (fb, sts) in enumerate(res[:-1]):
        assert sts == rsts, (what, m, k, sts, rsts)
        assert torch.equal(fb, ref), (what, m, k, float((fb - ref).abs().max()),
                                      int(((fb != ref).view(-1, 3).any(dim=1)).sum()))
    assert cnts[1].straight == 0 and cnts[2].straight == 0 and cnts[3].straight == 0, (what, cnts)
    assert (cnts[0].general, cnts[0].batched, cnts[0].fallback, cnts[0].kernels) == \
           (cnts[1].general, cnts[1].batched, cnts[1].fallback, cnts[1].kernels), (what, cnts)
    return cnts[0]


def _mix1(cnt, what):
    assert cnt.kernels == {MIX1} and cnt.general > 0 and cnt.batched == cnt.general, (what, cnt)


ORDERS = [False, True]
NLIGHTS = [1, 2]


@pytest.mark.parametrize("nl", NLIGHTS)
@pytest.mark.parametrize("plane_first", ORDERS)
def test_torus(gpu, plane_first, nl):
    """Interior pixels of the ring: whole batches hit the mesh well inside its
    box and take the straight path; the silhouette's batches do not."""
    for m in (16, 32):
        sc = scene(scenes.torus_mesh(24, 12), at=(0.0, 0.0001, -12.0), plane_first=plane_first, dirs=WARM2[:nl])
        cnt = compare(sc, m, what=("torus", plane_first, nl))
        _mix1(cnt, "torus")
        # fewer than one batch per sample iteration of every general pixel
        assert 0 < cnt.straight < cnt.general * (m * m // 64), cnt


@pytest.mark.parametrize("nl", NLIGHTS)
@pytest.mark.parametrize("plane_first", ORDERS)
def test_sphere(gpu, plane_first, nl):
    for m in (16, 32):
        cnt = compare(scene(sphere_mesh(), plane_first=plane_first, dirs=WARM2[:nl]), m, what=("sphere", plane_first, nl))
        _mix1(cnt, "sphere")
        assert cnt.straight > 0, cnt


@pytest.mark.parametrize("nl", NLIGHTS)
@pytest.mark.parametrize("plane_first", ORDERS)
def test_cube(gpu, plane_first, nl):
    """Every face lies on the box, so every hit is outside the inset box:
    no slot skips its gates and no batch is straight."""
    for m in (16, 32):
        cnt = compare(scene(cube_mesh(), at=(0.6, 1.5001, -11.0), plane_first=plane_first, dirs=WARM2[:nl]), m,
                      what=("cube", plane_first, nl))
        _mix1(cnt, "cube")
        assert cnt.straight == 0, cnt


@pytest.mark.parametrize("plane_first", ORDERS)
def test_bias_pushes_origins_out_of_the_box_top(gpu, plane_first):
    """A flattened sphere with the bias at 1e-2 of its size: the shadow origins
    near its top leave the box (inside the mesh's frame they are above hi.y),
    those further down stay inside the inset box."""
    mesh = sphere_mesh(radius=2.0, squash=0.5)
    for m in (16, 32):
        cnt = compare(scene(mesh, at=(0.0, 1.2, -11.0), plane_first=plane_first), m, bias=4e-2,
                      what=("bias 1e-2 of the size", plane_first))
        _mix1(cnt, "bias")
        assert cnt.straight > 0, cnt


@pytest.mark.parametrize("plane_first", ORDERS)
@pytest.mark.parametrize("dirs", [((0.0, -1.0, 0.0),), ((1.0, 0.0, 0.0),), ((0.0, -1.0, 0.0), (1.0, 0.0, 0.0))])
def test_axis_lights(gpu, dirs, plane_first):
    """A light straight down and a light along +x: two components of the
    shadow direction are zero, their reciprocals +-1e20. (A light along the
    plane has no grid for the batched kernel to search: whatever kernel the
    call takes, the frames agree.)"""
    for m in (16, 32):
        cnt = compare(scene(sphere_mesh(), plane_first=plane_first, dirs=dirs, raw=True), m,
                      what=("axis lights", dirs, plane_first))
        assert cnt.general > 0, cnt
        if dirs == ((0.0, -1.0, 0.0),):
            _mix1(cnt, "down")
            assert cnt.straight > 0, cnt


@pytest.mark.parametrize("plane_first", ORDERS)
def test_mesh_translated_by_1e3_sizes(gpu, plane_first):
    """The sphere's vertices 1e3 of its size away from the object-space origin
    (and the object's translation back): the margin 2^-12 |coordinates| is as
    large as the sphere, the inset box holds none of its surface."""
    off = np.array([4e3, -2e3, 1e3])
    mesh = sphere_mesh(centre=off)
    at = np.array([0.0, 2.5, -12.0]) - off
    for m in (16, 32):
        cnt = compare(scene(mesh, at=tuple(at), plane_first=plane_first), m, what=("1e3 sizes", plane_first))
        assert cnt.general > 0 and cnt.straight == 0, cnt


@pytest.mark.parametrize("where", ["inside", "a hair outside"])
def test_camera_at_the_mesh_box(gpu, where):
    """The camera inside the mesh's box (every camera ray starts inside it
    and misses the mesh) and 1e-3 in front of the box's near face. Neither
    camera has the whole box in front of its plane, so the call builds no
    pixel lists and is a one-kernel launch: no batch, nothing straight, and
    the frames still agree."""
    mesh = sphere_mesh(radius=2.0)
    z = 0.0 if where == "inside" else 2.0 + 1e-3
    c2w = cameras.lookat([0.0, 2.5, -12.0 + z], [0.0, 2.2, -20.0])
    for m in (16, 32):
        cnt = compare(scene(mesh, c2w=c2w), m, what=("camera", where))
        assert cnt.straight == 0 and cnt.batched == 0 and cnt.general == W * H, cnt


@pytest.mark.parametrize("cam", ["std", "below"])
def test_box_straddles_the_plane(gpu, cam):
    """test_gpu_oneplane's "through" scene: plane hits inside the mesh's box
    start their shadow rays inside it, and may lie inside the inset box."""
    for m in (16, 32):
        cnt = compare(_through_scene(cam), m, what=("through", cam))
        _mix1(cnt, "through")


def test_scanlines(gpu):
    sc = scene(sphere_mesh())

    def lines(ds, o, fb):
        for y in range(H):
            yield ds.render_device(o, fb, y0=y, y1=y + 1)

    cnt = compare(sc, 16, calls=lines, what="scanlines")
    assert cnt.straight > 0 and cnt.batched == cnt.general > 0, cnt


def test_bands(gpu):
    """A rank's round-robin 4-row bands (world 3)."""
    sc = scene(sphere_mesh())
    world, total = 3, 0
    for r in range(world):
        def bands(ds, o, fb, r=r):
            yield ds.render_bands_device(o, fb, 4, r, world)
        total += compare(sc, 16, calls=bands, rows=band_rows(H, 4, world), what=("bands", r)).straight
    assert total > 0


def test_progressive(gpu):
    sc = scene(sphere_mesh())
    for step, mx in ((4, 4), (2, 4), (1, 2)):
        def one(ds, o, fb, step=step, mx=mx):
            yield ds.render_device(o, fb, step=step, maxStep=mx)
        cnt = compare(sc, 16, calls=one, what=("progressive", step, mx))
        assert cnt.straight > 0, (step, mx, cnt)


def test_no_mix(gpu):
    """k_render_gen1 on its own (two kernels): the same general-pixel loop."""
    cnt = compare(scene(sphere_mesh()), 16, extra=RT_FLAG_NO_MIX, what="no mix")
    assert cnt.straight > 0 and cnt.batched == cnt.general > 0 and MIX1 not in cnt.kernels, cnt


def test_anchor_fp64_equals_oracle(gpu, oracle_mod):
    """The anchor's anchor: the sphere scene in float64, one pixel per wave
    (k_render_px64), one lane per pixel and the BVH only, bit for bit against
    the oracle."""
    import torch
    sc = scene(sphere_mesh())
    ds = DeviceScene(sc)
    w, h = 48, 32
    o = Options(width=w, height=h, antialias=Antialias(akGrid, 8), bias=BIAS, precision=Precision.fp64)
    ref, rst, _ = oracle_mod.OracleScene(sc, bvh=True).render(o)
    for flags in (0, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING):
        o.flags = flags
        fb = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        st = ds.render_device(o, fb)
        got = fb.view(h, w, 3).cpu().numpy()
        assert np.array_equal(got, ref), (flags, int(np.count_nonzero((got != ref).any(axis=2))))
        assert st == rst, (flags, st, rst)
