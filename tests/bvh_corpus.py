"""Meshes chosen to stress the BVH builders (csrc/rt_bvh.cpp, rt_bvh_gpu.hip),
the tree checker's hooks and the ray set the answers are compared over: shared
by test_bvh_corpus_cpu.py (the host builder and the oracle alone: the proof
that the corpus and the checker are sound) and test_gpu_bvh.py.

Every mesh is seeded and built in numpy; every triangle has its own three
vertices, except the tori and the flat grid.

* sizes: random soups of n faces around the leaf size (1 - 5, 8, 9), the
  clustering's +-16 radius (31 - 33, 64), one block of k_nearest (255 - 257),
  one block plus its 32-position halo (288, 289), two blocks (511 - 513), 1025;
* chains: log-spaced geometry, whose boxes nest around a shared corner, so a
  bottom-up clustering merges only the innermost pair in each round;
* one Morton cell, zero Morton axes, degenerate faces;
* large: 540,000 faces, past the 2048 x 256 faces at which k_bounds' threads
  start to stride (structure checks only).
"""
import ctypes as C
import functools

import numpy as np

from rtmi import abi, scenes
from rtmi._lib import lib
from rtmi.scene import TriangleMesh

SOUP_SIZES = (1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 255, 256, 257, 288, 289, 511, 512, 513, 1025)
N_RAYS = 512
MAX_DEPTH = 60  # rt_common.h kMaxBvhDepth: the kernels' traversal stack
LEAF_MAX = 4    # rt_common.h kLeafMax


def _own(tris):
    """(n, 3, 3) triangles -> a mesh in which each face has its own vertices."""
    tris = np.ascontiguousarray(tris, np.float64)
    return TriangleMesh(tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3))


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2.0, 2.0, (n, 1, 3)) + np.array([0.0, 2.0, 0.0])
    v = (c + rng.normal(0.0, 0.6, (n, 3, 3))).reshape(-1, 3)
    return TriangleMesh(v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3))


def coincident():
    """64 copies of one face (equal Morton codes, exact t ties) plus 3 others."""
    base = np.array([[-1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 3.0, 0.0]])
    v = np.concatenate([np.tile(base, (64, 1)), base + [2.5, 0.0, 0.5], base + [-2.5, 0.0, -0.5],
                        base + [0.0, 0.5, 1.0]])
    return TriangleMesh(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3))


def flat_grid(k=32):
    """A k x k quad grid in the plane y = 1.5, facing the camera's side
    (zero-thickness boxes: zero half-areas in the SAH collapse)."""
    xs = np.linspace(-3.0, 3.0, k + 1)
    zs = np.linspace(-2.0, 2.0, k + 1)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    v = np.stack([X.ravel(), np.full(X.size, 1.5), Z.ravel()], 1)
    f = []
    for i in range(k):
        for j in range(k):
            a, b, c, d = i * (k + 1) + j, (i + 1) * (k + 1) + j, (i + 1) * (k + 1) + j + 1, i * (k + 1) + j + 1
            f += [[a, d, b], [b, d, c]]
    return TriangleMesh(v, np.array(f, np.int32))


# ---- chains: spokes that grow geometrically from a shared corner -----------------
def fan():
    L = 1.3 ** (np.arange(120) - 60.0)
    z = np.zeros_like(L)
    return _own(np.stack([np.stack([z, z, z], 1), np.stack([L, z, z], 1), np.stack([L, 1e-3 * L, z], 1)], 1))


def fan3d():
    L = 1.25 ** (np.arange(150) - 75.0)
    z = np.zeros_like(L)
    return _own(np.stack([np.stack([z, z, z], 1), np.stack([L, 0.3 * L, 0.1 * L], 1),
                          np.stack([L, 0.31 * L, 0.2 * L], 1)], 1))


def spiral_fan():
    i = np.arange(300)
    L, a = 1.1 ** (i - 150.0), 0.02 * i
    z = np.zeros_like(L)
    return _own(np.stack([np.stack([z, z, z], 1), np.stack([L * np.cos(a), z, L * np.sin(a)], 1),
                          np.stack([L * np.cos(a + 0.02), z, L * np.sin(a + 0.02)], 1)], 1))


def disc_log():
    """80 rings of 16 faces, ring r between the radii 1.25^(r-40) and 1.25^(r-39)."""
    r, k = np.meshgrid(np.arange(80), np.arange(16), indexing="ij")
    R0, R1 = 1.25 ** (r.ravel() - 40.0), 1.25 ** (r.ravel() - 39.0)
    a0, a1 = k.ravel() * (2.0 * np.pi / 16), (k.ravel() + 1) * (2.0 * np.pi / 16)
    z = np.zeros_like(R0)
    return _own(np.stack([np.stack([R0 * np.cos(a0), z, R0 * np.sin(a0)], 1),
                          np.stack([R1 * np.cos(a0), z, R1 * np.sin(a0)], 1),
                          np.stack([R0 * np.cos(a1), z, R0 * np.sin(a1)], 1)], 1))


def flipped(mesh):
    """The same triangles wound the other way: the same boxes and tree, but the
    single-sided face test (geom.nim:306) now sees the side that, for the two
    flat meshes above, does not face the ground they lie on."""
    return TriangleMesh(mesh.vertices, np.ascontiguousarray(mesh.faces[:, [0, 2, 1]]))


def line_pow2(nested):
    """100 faces at x = 2^(i-50): from the origin to x (nested boxes), or
    from x to 1.5 x (boxes apart)."""
    x = 2.0 ** (np.arange(100) - 50.0)
    x0 = np.zeros_like(x) if nested else x
    x1 = x if nested else 1.5 * x
    w = x1 - x0
    z = np.zeros_like(x)
    return _own(np.stack([np.stack([x0, z, z], 1), np.stack([x1, z, 0.5 * w], 1), np.stack([x1, 0.5 * w, z], 1)], 1))


# ---- one Morton cell ---------------------------------------------------------------
def coincident_1000():
    base = np.array([[-1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 3.0, 0.5]])
    return _own(np.tile(base, (1000, 1, 1)))


def cluster_outlier():
    """500 faces of size 1e-5 within 1e-4 of the origin and one unit face at (1e4, 1e4, 1e4)."""
    rng = np.random.default_rng(41)
    c = rng.uniform(-1e-4, 1e-4, (500, 1, 3))
    small = c + rng.uniform(-0.5e-5, 0.5e-5, (500, 3, 3))
    big = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]]) + 1e4
    return _own(np.concatenate([small, big]))


def far_soup():
    """300 faces of extent 1e-3 centred at (1e4, 0, 0): the margin exceeds the mesh."""
    rng = np.random.default_rng(42)
    c = rng.uniform(-0.4e-3, 0.4e-3, (300, 1, 3))
    return _own(c + rng.uniform(-1e-4, 1e-4, (300, 3, 3)) + np.array([1e4, 0.0, 0.0]))


# ---- zero Morton axes --------------------------------------------------------------
def planar_soup():
    """A 500-face soup with every y equal."""
    rng = np.random.default_rng(43)
    c = rng.uniform(-2.0, 2.0, (500, 1, 3))
    t = c + rng.normal(0.0, 0.3, (500, 3, 3))
    t[:, :, 1] = 1.25
    return _own(t)


def axis_line():
    """500 faces whose centres lie on the x axis (each symmetric about it in y and z)."""
    rng = np.random.default_rng(44)
    x = rng.uniform(-3.0, 3.0, 500)
    h = rng.uniform(0.05, 0.4, 500)
    z = np.zeros(500)
    return _own(np.stack([np.stack([x - h, -h, -h], 1), np.stack([x + h, h, -h], 1), np.stack([x - h, z, h], 1)], 1))


# ---- degenerate faces --------------------------------------------------------------
N_POINT_FACES, N_LINE_FACES, N_PROPER = 300, 50, 10


def degenerate_mix():
    """300 faces with three equal vertices, then 50 with collinear vertices,
    then 10 proper faces, all in one box of side 4."""
    rng = np.random.default_rng(45)
    p = rng.uniform(-2.0, 2.0, (N_POINT_FACES, 1, 3)) + np.array([0.0, 2.5, 0.0])
    points = np.repeat(p, 3, axis=1)
    a = rng.uniform(-2.0, 2.0, (N_LINE_FACES, 3)) + np.array([0.0, 2.5, 0.0])
    d = rng.normal(0.0, 0.5, (N_LINE_FACES, 3))
    lines = np.stack([a, a + d, a + 2.0 * d], 1)  # a + 2 d is exact: the three are collinear
    c = rng.uniform(-1.5, 1.5, (N_PROPER, 1, 3)) + np.array([0.0, 2.5, 0.0])
    proper = c + rng.normal(0.0, 0.8, (N_PROPER, 3, 3))
    return _own(np.concatenate([points, lines, proper]))


MESHES = {f"soup_{n}": functools.partial(soup, n, 100 + n) for n in SOUP_SIZES}
CHAINS = ("fan", "fan3d", "spiral_fan", "disc_log", "line_pow2_nested", "line_pow2_apart")
MESHES.update({
    "fan": fan,
    "fan3d": fan3d,
    "spiral_fan": spiral_fan,
    "disc_log": disc_log,
    "spiral_fan_up": lambda: flipped(spiral_fan()),
    "disc_log_up": lambda: flipped(disc_log()),
    "line_pow2_nested": lambda: line_pow2(True),
    "line_pow2_apart": lambda: line_pow2(False),
    "coincident_1000": coincident_1000,
    "cluster_outlier": cluster_outlier,
    "far_soup": far_soup,
    "planar_soup": planar_soup,
    "axis_line": axis_line,
    "flat_grid": flat_grid,
    "coincident": coincident,
    "degenerate_mix": degenerate_mix,
    "torus_2304": lambda: scenes.torus_mesh(48, 24),
    "torus_540k": lambda: scenes.torus_mesh(600, 450),
})
LARGE = ("torus_540k",)
SMALL = tuple(n for n in MESHES if n not in LARGE)


def mesh_scene(name):
    return scenes._mesh_scene(MESHES[name](), "m", (0.7, 0.6, 0.5))


# ---- the ray set -------------------------------------------------------------------
def make_rays(scene, seed, n=N_RAYS):
    """n rays at the scene's mesh (object 0), in world space: towards a
    uniform point of a uniformly chosen face, from a sphere of twice the
    mesh's extent (its box's longest side) around its box's centre; one ray in
    four has a random direction instead. Unit directions."""
    mesh = scene.objects[0].geometry
    v = (np.concatenate([mesh.vertices, np.ones((len(mesh.vertices), 1))], 1) @ mesh.objectToWorld)[:, :3]
    lo, hi = v.min(0), v.max(0)
    centre, radius = 0.5 * (lo + hi), 2.0 * float((hi - lo).max())
    rng = np.random.default_rng(seed)
    tri = v[mesh.faces[rng.integers(0, len(mesh.faces), n)]]
    b = rng.uniform(0.0, 1.0, (n, 2))
    flip = b.sum(1) > 1.0
    b[flip] = 1.0 - b[flip]
    target = tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0])
    on_sphere = rng.normal(0.0, 1.0, (n, 3))
    orig = centre + radius * on_sphere / np.linalg.norm(on_sphere, axis=1, keepdims=True)
    d = target - orig
    rnd = rng.normal(0.0, 1.0, (n, 3))
    free = np.arange(n) % 4 == 3
    d[free] = rnd[free]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(orig), np.ascontiguousarray(d)


RAY_SEED = 7  # the seed the hit / miss condition of test_bvh_corpus_cpu.py was checked with


@functools.lru_cache(maxsize=None)
def rays(name):
    orig, d = make_rays(mesh_scene(name), RAY_SEED)
    orig.setflags(write=False)
    d.setflags(write=False)
    return orig, d


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's brute-force answers for rays(name): computed once, shared."""
    import oracle
    from query_checks import Ref
    return Ref(oracle.OracleScene(mesh_scene(name)), *rays(name))


# ---- the checker's hooks (csrc/rt_hooks.cpp) ---------------------------------------
COUNTERS = ("invalid", "uncontained", "big_leaves", "layout", "host_boxes", "boxes64", "boxes32", "children")
WORDS = COUNTERS + ("leaf_max", "depth", "reported_depth", "nodes")


def _report(out, cost):
    r = dict(zip(WORDS, (int(x) for x in out)))
    r["cost"] = float(cost[0])
    return r


BOX_DEFECT, ORDER_DEFECT, DEPTH_DEFECT = 1, 2, 4  # rtmi_test_bvh_check_host's `defect`


def check_host(mesh, defect=0):
    """build_bvh on the mesh's arrays through the checker; (rc, report)."""
    f = lib().rtmi_test_bvh_check_host
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int32,
                  C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    v = np.ascontiguousarray(mesh.vertices, np.float64)
    faces = np.ascontiguousarray(mesh.faces, np.int32)
    out, cost = (C.c_int64 * len(WORDS))(), (C.c_double * 1)()
    rc = f(v.ctypes.data_as(C.POINTER(C.c_double)), len(v), faces.ctypes.data_as(C.POINTER(C.c_int32)), len(faces),
           defect, out, cost)
    return rc, _report(out, cost)


def check_scene(ds, mesh=0):
    """One mesh of a live DeviceScene through the checker."""
    f = lib().rtmi_test_bvh_check
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    out, cost = (C.c_int64 * len(WORDS))(), (C.c_double * 1)()
    assert f(ds.h, mesh, out, cost) == abi.RT_OK, lib().rt_last_error()
    return _report(out, cost)


def ploc_raw(mesh):
    """The device builder alone on the mesh's arrays: (accepted, depth, nodes)."""
    f = lib().rtmi_test_ploc_raw
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
    v = np.ascontiguousarray(mesh.vertices, np.float64)
    faces = np.ascontiguousarray(mesh.faces, np.int32)
    out = (C.c_int64 * 3)()
    assert f(v.ctypes.data_as(C.POINTER(C.c_double)), len(v), faces.ctypes.data_as(C.POINTER(C.c_int32)), len(faces),
             out) == abi.RT_OK, lib().rt_last_error()
    return bool(out[0]), int(out[1]), int(out[2])


def counters(report):
    return {k: report[k] for k in COUNTERS}


ZERO = dict.fromkeys(COUNTERS, 0)
