"""The cases the multiprecision truth (truth.py) is recorded for: shared by
the generator tests/golden/make_truth.py, test_truth_cpu.py (which recomputes
them, whole or in part) and test_gpu_truth.py (which only reads the scenes
and the recorded answers). Nothing here imports the oracle or anything native.

* ray batches: two of rays at thresholds (edge_rays_15, edge_rays_4), and
  N_RAYS seeded rays per scene, origins above the ground (in
  boxes2 the platform's underside lies in the ground plane: from below, a
  quarter of the rays would be exact ties), three quarters aimed at the
  scene's bounds; every fifth ray has a finite t_near around its distance to
  the scene's centre, so that both sides of `t < t_near` occur;
* picks: integer, fractional and out-of-image positions of a PICK_W x PICK_H
  image through the scene's camera;
* frames: FRAME_W x FRAME_H at akNone (m = 0), akGrid 2 and akGrid 8 (64
  samples: one pixel per wave, the smallest at which k_render_px64 runs);
* the output quantiser's inputs."""
import numpy as np

from rtmi import scenes
from rtmi.scene import Box, Plane, Sphere, TriangleMesh

import truth
from subset_scenes import subset_scene

N_RAYS = 500
BATCHES = {
    "s3": lambda: subset_scene(3), "s11": lambda: subset_scene(11),      # sphere + box, plain and general
    "s4": lambda: subset_scene(4), "s12": lambda: subset_scene(12),      # mesh, plain and general
    "s15": lambda: subset_scene(15),
    "boxes2": scenes.boxes2,                                             # thirteen Y rotations
    "two_meshes": scenes.two_meshes,
    "edge15": lambda: subset_scene(15),     # edge_rays_15
    "edge4": lambda: subset_scene(4),       # edge_rays_4
}
SEEDED = ("s3", "s11", "s4", "s12", "s15", "boxes2", "two_meshes")
SEEDS = {"s3": 103, "s11": 111, "s4": 104, "s12": 112, "s15": 115, "boxes2": 7, "two_meshes": 8}
HAS_MESH = ("s4", "s12", "s15", "two_meshes", "edge15", "edge4")

PICK_SCENES = ("s15", "boxes2")
PICK_W, PICK_H = 96, 64

FRAME_BITS = (12, 19, 35, 63)
FRAME_M = (0, 2, 8)
FRAME_W, FRAME_H, BIAS, DEPTH = 16, 12, 1e-4, 5

QUANT_CASES = [(bits, srgb) for bits in (5, 8, 16) for srgb in (True, False)]

UNDECIDED_CAP = 0.02
QUANT_CAP = 0.01


def bounds(scene):
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


def edge_rays_15():
    """320 rays at subset 15 whose directions are not unit vectors: 100 of its
    seeded rays scaled by 0.01 and 100 by 100 (a = d.d far from 1: the
    sphere's `/2*a`; t_near scaled the other way), and 120 nearly parallel
    to the ground, d.y = -k * 1e-6 for k either side of the plane's
    |n.d| > 1e-6."""
    orig, d, tnear = make_rays("s15")
    orig, d, tnear = orig[:320].copy(), d[:320].copy(), tnear[:320].copy()
    d[:100] *= 0.01
    tnear[:100] *= 100.0
    d[100:200] *= 100.0
    tnear[100:200] *= 0.01
    rng = np.random.default_rng(515)
    az = rng.uniform(0.0, 2.0 * np.pi, 120)
    k = np.tile([0.5, 0.9, 0.999, 1.001, 1.1, 2.0], 20)
    d[200:] = np.stack([np.cos(az), -k * 1e-6, np.sin(az)], 1)
    orig[200:, 1] = rng.uniform(0.05, 4.0, 120)
    tnear[200:] = np.inf
    return orig, d, tnear


def edge_rays_4():
    """128 rays at subset 4's torus, one straight down the normal of every
    second face from 5 units away, so short that the face's det is k * 1e-6
    for k either side of the absolute `det < 1e-6` cull."""
    g = subset_scene(4).objects[0].geometry
    v = g.vertices[g.faces[::2]] + np.asarray(g.objectToWorld)[3, :3]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    area2 = np.linalg.norm(n, axis=1)
    n /= area2[:, None]
    k = np.tile([0.5, 0.9, 0.999, 1.001, 1.1, 2.0, 10.0, 1000.0], len(v) // 8 + 1)[:len(v)]
    orig = v.mean(1) + 5.0 * n
    d = -n * (k * 1e-6 / area2)[:, None]
    return np.ascontiguousarray(orig), np.ascontiguousarray(d), np.full(len(v), np.inf)


def make_rays(name, n=N_RAYS):
    """(orig (n, 3), dir (n, 3), t_near (n,)) of batch `name`."""
    if name in ("edge15", "edge4"):
        return edge_rays_15() if name == "edge15" else edge_rays_4()
    lo, hi = bounds(BATCHES[name]())
    rng = np.random.default_rng(SEEDS[name])
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    orig[:, 1] = 0.25 + np.abs(orig[:, 1])          # above the ground
    d = rng.uniform(lo, hi, (n, 3)) - orig
    rnd = rng.normal(0.0, 1.0, (n, 3))
    free = np.arange(n) % 4 == 3
    d[free] = rnd[free]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tnear = np.full(n, np.inf)
    near = np.arange(n) % 5 == 4
    tnear[near] = (np.linalg.norm(c - orig, axis=1) * rng.uniform(0.5, 1.5, n))[near]
    return np.ascontiguousarray(orig), np.ascontiguousarray(d), tnear


def _answers(rows):
    obj, face, t, nrm, tests, hits, margin = zip(*rows)
    return {"obj": np.array(obj, np.int32), "face": np.array(face, np.int32), "t": np.array(t, np.float64),
            "normal": np.array(nrm, np.float64).reshape(-1, 3), "tests": np.array(tests, np.int64),
            "hits": np.array(hits, np.int64), "margin": np.array(margin, np.float64)}


def batch(name, idx=None):
    """The truth of batch `name` (of its rays idx): what truth_<name>.npz holds."""
    orig, d, tnear = make_rays(name)
    idx = np.arange(len(orig)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(BATCHES[name]())
    out = _answers([truth.query(ts, orig[i], d[i], tnear[i]) for i in idx])
    out.update(orig=orig[idx], dir=d[idx], tnear=tnear[idx])
    return out


def oracle_answers(osc, b):
    """An OracleScene's answers for the rays of a batch or pick set `b`, in
    the fixtures' form (obj, face, t, normal, tests, hits)."""
    n = len(b["orig"])
    out = {"obj": np.empty(n, np.int32), "face": np.empty(n, np.int32), "t": np.empty(n), "normal": np.zeros((n, 3)),
           "tests": np.empty(n, np.int64), "hits": np.empty(n, np.int64)}
    for i in range(n):
        o, d = np.append(b["orig"][i], 1.0), np.append(b["dir"][i], 0.0)
        ob, t, tri, st = osc.trace(o, d, float(b["tnear"][i]) if "tnear" in b else float("inf"))
        out["obj"][i], out["t"][i], out["face"][i] = ob, t, tri if ob >= 0 else -1
        out["tests"][i], out["hits"][i] = st.numIntersectionTests, st.numIntersectionHits
        if ob >= 0:
            out["normal"][i] = osc.hit_normal(o, d, ob, t, tri)
    return out


def compare(want, got, tol_t, tol_n, counts=True):
    """The comparison of answers with a recorded truth, on its decided rays:
    objects and faces equal, t within tol_t ulps (a miss: t_near itself),
    normals within tol_n (truth.vec_ulps), per-ray tests and hits equal where
    `got` has them. Returns the largest errors seen (t, normal) in ulps."""
    ok = want["margin"] >= truth.EPS
    assert np.array_equal(got["obj"][ok], want["obj"][ok])
    assert np.array_equal(got["face"][ok], want["face"][ok])
    hit, miss = ok & (want["obj"] >= 0), ok & (want["obj"] < 0)
    assert np.array_equal(got["t"][miss], want["t"][miss])
    e_t = truth.ulps(got["t"][hit], want["t"][hit]).max(initial=0.0)
    e_n = truth.vec_ulps(got["normal"][hit], want["normal"][hit]).max(initial=0.0) if hit.any() else 0.0
    assert e_t <= tol_t, (e_t, tol_t)
    assert e_n <= tol_n, (e_n, tol_n)
    assert not np.asarray(got["normal"])[miss].any()
    if counts and "tests" in got:
        assert np.array_equal(got["tests"][ok], want["tests"][ok])
        assert np.array_equal(got["hits"][ok], want["hits"][ok])
    return float(e_t), float(e_n)


def pick_xy(name):
    """120 positions: 40 integer, 60 fractional, 20 outside the image."""
    rng = np.random.default_rng(SEEDS[name] + 1000)
    whole = np.stack([rng.integers(0, PICK_W, 40), rng.integers(0, PICK_H, 40)], 1).astype(np.float64)
    frac = rng.uniform((0.0, 0.0), (PICK_W, PICK_H), (60, 2))
    out = rng.uniform((-24.0, -16.0), (0.0, 0.0), (20, 2))
    out[::2] += (PICK_W + 24.0, PICK_H + 16.0)
    return np.ascontiguousarray(np.concatenate([whole, frac, out]))


def picks(name, idx=None):
    """truth_pick_<name>.npz: the camera rays and their answers."""
    xy = pick_xy(name)
    idx = np.arange(len(xy)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(BATCHES[name]())
    rows = [truth.pick(ts, PICK_W, PICK_H, float(xy[i, 0]), float(xy[i, 1])) for i in idx]
    out = _answers([r[2:] for r in rows])
    out.update(xy=xy[idx], orig=np.array([r[0] for r in rows]), dir=np.array([r[1] for r in rows]))
    return out


def frame(bits, m, rows=None):
    """truth_frame_<bits>_m<m>.npz (its rows `rows`): rgb (float64), the Stats
    of each pixel (primary, tests, hits, shadow, reflection), both margins."""
    rows = range(FRAME_H) if rows is None else rows
    ts = truth.TruthScene(subset_scene(bits))
    px = [[truth.pixel(ts, FRAME_W, FRAME_H, x, y, m, BIAS, DEPTH) for x in range(FRAME_W)] for y in rows]
    return {"rgb": np.array([[p[0] for p in r] for r in px], np.float64),
            "stats": np.array([[p[1] for p in r] for r in px], np.int64),
            "margin": np.array([[p[2] for p in r] for r in px], np.float64),
            "margin32": np.array([[p[3] for p in r] for r in px], np.float64)}


PRIMITIVES = ("camera", "sphere", "aabb", "triangle")
N_PRIMITIVE = 1000


def primitive_inputs(kind, n=N_PRIMITIVE):
    """n seeded argument tuples for one of the oracle's primitives. Rays are
    not normalised (the sphere's `/2*a` shows only where a != 1); most are
    aimed at the shape or just beside it; one box ray in eight has a zero
    direction component."""
    from rtmi import glm
    rng = np.random.default_rng(900 + PRIMITIVES.index(kind))
    out = []
    for i in range(n):
        o = rng.uniform(-10.0, 10.0, 3)
        scale = rng.uniform(0.5, 2.0)
        if kind == "camera":
            w, h = int(rng.integers(1, 2000)), int(rng.integers(1, 2000))
            m = glm.rotate(glm.mat4(1.0), rng.normal(size=3), rng.uniform(-3.0, 3.0))
            m = glm.translate(m, rng.uniform(-20.0, 20.0, 3))
            out.append((w, h, float(rng.uniform(-8.0, w + 8.0)), float(rng.uniform(-8.0, h + 8.0)),
                        float(rng.uniform(5.0, 150.0)), m))
        elif kind == "sphere":
            r = float(rng.uniform(0.1, 3.0))
            aim = rng.normal(size=3)
            aim *= r * rng.uniform(0.0, 1.5) / np.linalg.norm(aim)
            d = (aim - o) / np.linalg.norm(aim - o) * scale
            out.append((r, np.append(o, 1.0), np.append(d if i % 8 else -d, 0.0)))
        elif kind == "aabb":
            vmin = rng.uniform(-3.0, 0.0, 3)
            vmax = vmin + rng.uniform(0.1, 4.0, 3)
            aim = rng.uniform(vmin - 0.25 * (vmax - vmin), vmax + 0.25 * (vmax - vmin))
            d = (aim - o) / np.linalg.norm(aim - o) * scale
            if i % 8 == 7:
                d[int(rng.integers(0, 3))] = 0.0 if i % 16 == 7 else -0.0
            if i % 32 == 5:
                o = rng.uniform(vmin, vmax)         # starts inside: tmin < 0 is returned
            out.append((vmin, vmax, np.append(o, 1.0), np.append(d, 0.0)))
        else:
            v = rng.uniform(-3.0, 3.0, (3, 3))
            a, b = rng.uniform(-0.3, 1.0, 2)
            aim = v[0] + a * (v[1] - v[0]) + b * (v[2] - v[0])
            d = (aim - o) / np.linalg.norm(aim - o) * scale
            if i % 4 and np.dot(np.cross(v[1] - v[0], v[2] - v[0]), d) > 0:
                v = v[[0, 2, 1]]                    # three quarters face the ray (the test is single-sided)
            out.append((np.append(o, 1.0), np.append(d, 0.0), v[0], v[1], v[2]))
    return out


def primitive_truth(kind, args):
    """(values (n, k) float64 with -inf for the reference's -inf, margins (n,))."""
    vals, margins = [], []
    for a in args:
        mg = truth.Margin()
        if kind == "camera":
            o, d = truth.cast_primary_ray(*a)
            v = [float(x) for x in o + d]
        else:
            if kind == "sphere":
                t = truth.sphere_intersect(truth.mpf(a[0]), truth._vec(a[1]), truth._vec(a[2]), mg)
            elif kind == "aabb":
                t = truth.aabb_intersect(truth._vec(a[0]), truth._vec(a[1]), truth._vec(a[2]), truth._vec(a[3]), mg)
            else:
                t, m = truth.ray_triangle(*(truth._vec(x) for x in a))
                mg.add(m)
            v = [-np.inf if t is None else float(t)]
        vals.append(v)
        margins.append(mg.m)
    return np.array(vals, np.float64), np.array(margins)


def primitive_oracle(oracle_mod, kind, args):
    f = {"camera": lambda *a: np.concatenate([x[:3] for x in oracle_mod.cast_primary_ray(*a)]),
         "sphere": oracle_mod.sphere_intersect, "aabb": oracle_mod.aabb_intersect,
         "triangle": oracle_mod.ray_triangle}[kind]
    return np.array([np.atleast_1d(f(*a)) for a in args], np.float64)


def compare_primitive(kind, want, margins, got, tol):
    """hit / miss equal and the value within tol ulps, on decided inputs;
    returns the largest error in ulps."""
    ok = margins >= truth.EPS
    assert (~ok).mean() <= UNDECIDED_CAP
    if kind == "camera":
        e = max(truth.vec_ulps(got[:, :3], want[:, :3]).max(), truth.vec_ulps(got[:, 3:], want[:, 3:]).max())
    else:
        w, g = want[ok, 0], got[ok, 0]
        assert np.array_equal(np.isfinite(w), np.isfinite(g))
        assert np.array_equal(w[~np.isfinite(w)], g[~np.isfinite(g)])
        assert 0.2 <= np.isfinite(w).mean() <= 0.9   # hits and misses both occur
        e = truth.ulps(g[np.isfinite(w)], w[np.isfinite(w)]).max()
    assert e <= tol, (kind, e, tol)
    return float(e)


def matrices():
    """The matrices the inverses are checked on: every object and camera
    matrix of boxes2, mesh_mix and subset_scene(15), and 200 seeded affine
    matrices of condition number <= 1e3 (rotation * scales in [0.1, 10] *
    rotation, a translation in [-20, 20])."""
    out = []
    for sc in (scenes.boxes2(), scenes.mesh_mix(), subset_scene(15)):
        out += [np.asarray(o.geometry.objectToWorld, np.float64) for o in sc.objects]
        out.append(np.asarray(sc.cameraToWorld, np.float64))
    rng = np.random.default_rng(77)
    n_scene = len(out)
    while len(out) < n_scene + 200:
        q1, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q2, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q1 @ np.diag(10.0 ** rng.uniform(-1.0, 1.0, 3)) @ q2
        m = np.eye(4)
        m[:3, :3] = a.T                    # glm's m[col][row]
        m[3, :3] = rng.uniform(-20.0, 20.0, 3)
        if np.linalg.cond(a) <= 1e3:
            out.append(m)
    return out


def quant_inputs():
    """4,096 seeded float32 in [-0.2, 1.2], 0.0031308, every k / 255, the
    extremes: 4,365 values, a multiple of 3 (one RGB row of 1,455 pixels)."""
    rng = np.random.default_rng(55)
    one = np.float32(1.0)
    extremes = [-0.2, 1.2, 0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                1e-45, 1e-30, -1e30, 1e30, 0.5]
    v = np.concatenate([rng.uniform(-0.2, 1.2, 4096), [0.0031308], np.arange(256) / 255.0, extremes])
    assert len(v) % 3 == 0
    return v.astype(np.float32)


def quant():
    """truth_quant.npz: the inputs and, per (bits, srgb), q and the undecided flags."""
    v = quant_inputs()
    out = {"v": v}
    for bits, srgb in QUANT_CASES:
        q, und = truth.quantise(v, bits, srgb)
        out[f"q_{bits}_{int(srgb)}"] = q.astype(np.uint16)
        out[f"und_{bits}_{int(srgb)}"] = und
    return out
