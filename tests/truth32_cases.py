"""The cases the float32 ray, pick and radiance queries are judged on against
the multiprecision truth (truth.py): shared by the generator
tests/golden/make_truth32.py, test_truth32_cpu.py and test_gpu_truth32.py
(which reads the scenes and the recorded answers only). Nothing here imports
the oracle or anything native.

Every origin, direction, t_near and pick position is a float32 value, and the
truth is evaluated on exactly those values (the scenes keep their doubles: a
float32 kernel's rounding of them is part of its error, which EPS32 covers).

* ray batches (RAY_SCENES, N_RAYS rays, make_rays): incoherent rays, the
  quotas of QUOTAS asserted per batch: origins inside a bounded object's
  box, origins below the ground, directions with one or two components +0.0
  or -0.0, every fifth ray a finite t_near, a quarter unaimed;
* corpus batches (CORPUS): bvh_corpus.rays on the hostile meshes whose faces
  float32 coordinates still resolve; on the PLACED three, where those rays
  decide too little, placed_rays;
* picks (truth_cases.pick_xy, positions in 1/64ths);
* radiance (SHADE_SCENES, N_SHADE rays of make_rays, bias 1e-4, depth 5).

An answer is decided for a float32 kernel where the truth's float32 query
margins (truth.Margin.h32 / n32) reach EPS32 (or a batch's raised threshold,
truth32_meta.json "exclude"): `decided`.

brute_force is the specification in plain numpy float32, every object and
every face against every ray, with no tree, list or clamp: the proof that the
thresholds leave honest float32 arithmetic room (test_truth32_cpu.py).
compare is the comparison the GPU tests and that proof share."""
import functools
import json
import os

import numpy as np

from rtmi import scenes
from rtmi.scene import Box, Plane, Sphere, TriangleMesh

import bvh_corpus as bc
import truth
import truth_cases as tc
from subset_scenes import subset_scene

# test_gpu_trace32.py's bounds on a float32 query (4 x the largest error measured there)
T_BOUND = 2e-4
N_BOUND = 2e-3
RGB_BOUND = 1e-4        # test_float32_frame's and test_gpu_shade32.py's
F32 = np.float32

N_RAYS = 512            # eight waves
RAY_SCENES = {
    "s3": lambda: subset_scene(3), "s11": lambda: subset_scene(11),
    "s4": lambda: subset_scene(4), "s12": lambda: subset_scene(12),
    "s15": lambda: subset_scene(15),
    "boxes2": scenes.boxes2, "two_meshes": scenes.two_meshes, "mesh_mix": scenes.mesh_mix,
}
SEEDS = {"s3": 3203, "s11": 3211, "s4": 3204, "s12": 3212, "s15": 3215, "boxes2": 3207, "two_meshes": 3208,
         "mesh_mix": 3209, "s19": 3219, "s35": 3235, "s63": 3263}
# below the ground boxes2's platform underside lies in the ground plane (truth_cases)
NO_BELOW = ("boxes2",)
CORPUS = ("soup_33", "soup_257", "soup_1025", "torus_2304", "spiral_fan_up", "disc_log_up", "flat_grid",
          "planar_soup", "degenerate_mix")
# Meshes on which bvh_corpus.rays decide too little for a float32 kernel (measured: 36 % on spiral_fan, 63 %
# on planar_soup, and on disc_log a brute force that fails at every threshold):
# * spiral_fan and disc_log lie 1e-4 above the ground plane and face it, so whatever ray meets a face has
#   crossed the ground just before it: no ray has a face as its answer, from any side. Their flipped twins
#   (bvh_corpus.flipped: the same vertices, boxes and tree, faces wound to look up) stand in for them.
# * From a distance a face's t and the plane's still differ by ~1e-5 relative. disc_log's radius is
#   1.25^40 = 7.5e3, so bvh_corpus's origins are some 3e4 units away, from where float32 cannot place a ray
#   on a ring of any size.
# * planar_soup's faces are coplanar and overlap, so most face hits tie.
# They get placed_rays instead: origins 0.05 - 0.2 from a face float32 resolves, answers unique by
# construction.
# (fan3d stays out: its faces are nested coplanar copies, so every point of every face but the outer strip
# of the largest, 1.5e7 units out, is covered by two faces or more: an exact tie, test_gpu_ties.py's.)
PLACED = ("spiral_fan_up", "disc_log_up", "planar_soup")
SLACK = 1e-3
PLACED_SEEDS = {"spiral_fan_up": 3301, "disc_log_up": 3302, "planar_soup": 3303}
PICK_SCENES = ("s15", "boxes2")
PICK_W, PICK_H = tc.PICK_W, tc.PICK_H
N_SHADE = 256
SHADE_SCENES = {"s19": lambda: subset_scene(19), "s35": lambda: subset_scene(35), "s63": lambda: subset_scene(63),
                "boxes2": scenes.boxes2}
BIAS, DEPTH = 1e-4, 5

QUOTAS = {"inside": 0.05, "below": 0.05, "zero": 0.10}
HIT_SHARE, NORMAL_SHARE, SHADE_SHARE, BOX_HITS = 0.80, 0.70, 0.50, 30


def scene_of(name):
    if name in RAY_SCENES:
        return RAY_SCENES[name]()
    if name in SHADE_SCENES:
        return SHADE_SCENES[name]()
    return bc.mesh_scene(name)


def has_mesh(scene):
    return any(isinstance(o.geometry, TriangleMesh) for o in scene.objects)


def kinds(scene):
    return np.array([{Sphere: 0, Plane: 1, Box: 2, TriangleMesh: 3}[type(o.geometry)] for o in scene.objects])


# ---- the rays -------------------------------------------------------------------------
def _object_box(g):
    """Object-space box of a bounded object (a sphere: the cube inscribed in it)."""
    if isinstance(g, Sphere):
        h = g.r / np.sqrt(3.0)
        return np.full(3, -h), np.full(3, h)
    if isinstance(g, Box):
        return np.asarray(g.vmin, np.float64)[:3], np.asarray(g.vmax, np.float64)[:3]
    return g.vertices.min(0), g.vertices.max(0)


def _to_world(g, p):
    return (np.append(p, 1.0) @ np.asarray(g.objectToWorld, np.float64))[:3]


def inside_some_box(scene, orig):
    """Per origin: strictly inside a bounded object's box (a mesh's box, a
    box, the cube inscribed in a sphere), tested in the object's frame."""
    out = np.zeros(len(orig), bool)
    for ob in scene.objects:
        g = ob.geometry
        if isinstance(g, Plane):
            continue
        lo, hi = _object_box(g)
        p = np.concatenate([np.asarray(orig, np.float64), np.ones((len(orig), 1))], 1) @ np.linalg.inv(
            np.asarray(g.objectToWorld, np.float64))
        out |= ((p[:, :3] > lo) & (p[:, :3] < hi)).all(1)
    return out


def on_slab_plane(scene, orig, d):
    """Per ray: a zero direction component whose origin lies on a slab plane
    of an axis-aligned (untransformed or translated) box or mesh box."""
    out = np.zeros(len(orig), bool)
    for ob in scene.objects:
        g = ob.geometry
        m = np.asarray(g.objectToWorld, np.float64)
        if isinstance(g, (Plane, Sphere)) or not np.array_equal(m[:3, :3], np.eye(3)):
            continue
        lo, hi = _object_box(g)
        p = np.asarray(orig, np.float64) - m[3, :3]
        out |= ((np.asarray(d) == 0) & ((p == lo) | (p == hi))).any(1)
    return out


def make_rays(name, n=N_RAYS):
    """(orig (n, 3), dir (n, 3), t_near (n,)) float32 of batch `name`, built
    as truth_cases.make_rays builds its rays, with by index i:
      i % 16 == 6   the origin below the ground (not in NO_BELOW);
      i % 16 == 2   the origin inside a bounded object's box, the objects in turn;
      i %  8 == 0   one (i // 16 even) or two direction components set to
                    +0.0 (i // 8 even) or -0.0;
      i %  5 == 4   a finite t_near around the distance to the scene's centre;
      i %  4 == 3   a random direction instead of an aimed one;
      i %  4 == 1   aimed at a point of a bounded object's box, the objects in
                    turn (the others: at a point of the scene's bounds).
    Each ray draws its own origin and target: consecutive rays are unrelated."""
    scene = scene_of(name)
    lo, hi = tc.bounds(scene)
    rng = np.random.default_rng(SEEDS[name])
    i = np.arange(n)
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    orig[:, 1] = 0.25 + np.abs(orig[:, 1])
    below = (i % 16 == 6) & (name not in NO_BELOW)
    orig[below, 1] = -orig[below, 1]
    bounded = [o.geometry for o in scene.objects if not isinstance(o.geometry, Plane)]
    u = rng.uniform(0.1, 0.9, (n, 3))
    for k in np.flatnonzero(i % 16 == 2):
        g = bounded[(k // 16) % len(bounded)]
        blo, bhi = _object_box(g)
        orig[k] = _to_world(g, blo + u[k] * (bhi - blo))
    target = rng.uniform(lo, hi, (n, 3))
    v = rng.uniform(0.0, 1.0, (n, 3))
    boxes = [g for g in bounded if isinstance(g, Box)]
    aimed = bounded + 2 * boxes if len(boxes) == 1 else bounded     # a lone box among other objects: three turns
    for k in np.flatnonzero(i % 4 == 1):
        g = aimed[(k // 4) % len(aimed)]
        blo, bhi = _object_box(g)
        target[k] = _to_world(g, blo + v[k] * (bhi - blo))
    d = target - orig
    rnd = rng.normal(0.0, 1.0, (n, 3))
    free = i % 4 == 3
    d[free] = rnd[free]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axis = rng.integers(0, 3, n)
    for k in np.flatnonzero(i % 8 == 0):
        z = -0.0 if (k // 8) % 2 else 0.0
        d[k, axis[k]] = z
        if (k // 16) % 2:
            d[k, (axis[k] + 1) % 3] = z
    tnear = np.full(n, np.inf)
    near = i % 5 == 4
    tnear[near] = (np.linalg.norm(c - orig, axis=1) * rng.uniform(0.5, 1.5, n))[near]
    orig, d, tnear = (np.ascontiguousarray(a.astype(F32)) for a in (orig, d, tnear))
    # the quotas
    assert inside_some_box(scene, orig).mean() >= QUOTAS["inside"], name
    assert name in NO_BELOW or (orig[:, 1] < 0).mean() >= QUOTAS["below"], name
    nz = (d == 0).sum(1)
    zero = (nz >= 1) & (nz <= 2)
    neg = zero & (np.signbit(d) & (d == 0)).any(1)
    assert zero.mean() >= QUOTAS["zero"] and abs(int(neg.sum()) * 2 - int(zero.sum())) <= 1, name
    assert not on_slab_plane(scene, orig, d).any(), name
    assert np.isfinite(tnear[4::5]).all() and free.mean() == 0.25
    return orig, d, tnear


def _faces_hit(V, F, o, d, slack):
    """Per ray and face (float64): the face is hit with every test of
    ray_triangle passed by `slack` or more (negative: missed by less than
    -slack), and t (inf where not)."""
    v0, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    with np.errstate(all="ignore"):
        p = np.cross(d[:, None, :], e2[None])
        det = (e1[None] * p).sum(2)
        tv = o[:, None, :] - v0[None]
        u = (tv * p).sum(2) / det
        q = np.cross(tv, e1[None])
        v = (d[:, None, :] * q).sum(2) / det
        t = (e2[None] * q).sum(2) / det
        ok = (det >= 1e-6 * (1.0 + 500.0 * slack)) & (u >= slack) & (v >= slack) & (u + v <= 1.0 - slack) & (t >= 10.0 * slack)
    return ok, np.where(ok, t, np.inf)


def placed_rays(name, n=N_RAYS):
    """n rays at a PLACED mesh that float32 can place and whose answer is
    unique, in world space as float32. Three in four start 0.05 - 0.2 above
    a point well inside a face (on the side it faces; the face drawn
    uniformly from those of size 0.03 or more within 100 units of the mesh's
    origin, so that a float32 world coordinate resolves it and t stays clear
    of 0), moved sideways by up to that height; every fourth has a random
    direction from such an origin (every eighth: one that leaves the face's
    side). Candidates are drawn in order and kept
    when, in float64, every face is either hit with SLACK (ten times EPS32)
    to spare on every barycentric test or missed by as much (no face in
    between; a huge face whose apex is near the ray is such a face), and the
    closest hit is the only one within 1 % of its t. Consecutive rays are unrelated."""
    mesh = bc.mesh_scene(name).objects[0].geometry
    V, F = np.asarray(mesh.vertices, np.float64), np.asarray(mesh.faces, np.int64)
    shift = np.asarray(mesh.objectToWorld, np.float64)[3, :3]
    assert np.array_equal(np.asarray(mesh.objectToWorld)[:3, :3], np.eye(3))
    nrm = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    area2 = np.linalg.norm(nrm, axis=1)
    good = np.flatnonzero((np.sqrt(area2) >= 0.03) & (np.abs(V[F]).max(axis=(1, 2)) <= 100.0))
    assert len(good) >= 32, (name, len(good))
    rng = np.random.default_rng(PLACED_SEEDS[name])
    m = 32 * n
    f = good[rng.integers(0, len(good), m)]
    b = rng.uniform(0.1, 0.4, (m, 2))
    tri = V[F[f]]
    target = tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0])
    up = nrm[f] / area2[f][:, None]
    h = rng.uniform(0.05, 0.2, m)
    side = rng.normal(0.0, 1.0, (m, 3))
    side -= (side * up).sum(1, keepdims=True) * up
    side *= (rng.uniform(0.0, 1.0, m) * h / np.linalg.norm(side, axis=1))[:, None]
    orig = target + up * h[:, None] + side
    d = target - orig
    rnd = rng.normal(0.0, 1.0, (m, 3))
    free = np.arange(m) % 4 == 3
    away = free & (np.arange(m) % 8 == 7) & ((rnd * up).sum(1) < 0)       # every second of them leaves its face's side
    rnd[away] = -rnd[away]
    d[free] = rnd[free]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    orig32, d32 = (orig + shift).astype(F32), d.astype(F32)
    o64, d64 = orig32.astype(np.float64) - shift, d32.astype(np.float64)      # what the rounded ray is, in the mesh's frame
    keep = np.zeros(m, bool)
    for a in range(0, m, 256):
        sl = slice(a, a + 256)
        sure, t = _faces_hit(V, F, o64[sl], d64[sl], SLACK)
        maybe, _ = _faces_hit(V, F, o64[sl], d64[sl], -SLACK)
        ts = np.sort(t, axis=1)
        alone = ~np.isfinite(ts[:, 0]) | (ts[:, 1] > 1.01 * ts[:, 0])
        keep[sl] = (sure == maybe).all(1) & alone
    aimed, unaimed = list(np.flatnonzero(keep & ~free)), list(np.flatnonzero(keep & free))
    assert len(aimed) >= n - n // 4 and len(unaimed) >= n // 4, (name, len(aimed), len(unaimed))
    idx = np.array([unaimed.pop(0) if i % 4 == 3 else aimed.pop(0) for i in range(n)])
    return np.ascontiguousarray(orig32[idx]), np.ascontiguousarray(d32[idx]), np.full(n, np.inf, F32)


def corpus_rays(name):
    """bvh_corpus.rays rounded to float32; placed_rays on the PLACED meshes."""
    if name in PLACED:
        return placed_rays(name)
    orig, d = bc.rays(name)
    return (np.ascontiguousarray(orig.astype(F32)), np.ascontiguousarray(d.astype(F32)),
            np.full(len(orig), np.inf, F32))


def rays_of(name):
    return corpus_rays(name) if name in CORPUS else make_rays(name)


def pick_xy(name):
    """truth_cases.pick_xy with the fractional positions rounded to 1/64ths: exact in float32."""
    xy = np.round(tc.pick_xy(name) * 64.0) / 64.0
    xy32 = xy.astype(F32)
    assert np.array_equal(xy32.astype(np.float64), xy)
    return np.ascontiguousarray(xy32)


# ---- the truth of the cases ---------------------------------------------------------------
def _answers(rows):
    obj, face, t, nrm, tests, hits, margin, hit32, normal32 = zip(*rows)
    return {"obj": np.array(obj, np.int32), "face": np.array(face, np.int32), "t": np.array(t, np.float64),
            "normal": np.array(nrm, np.float64).reshape(-1, 3), "tests": np.array(tests, np.int32),
            "hits": np.array(hits, np.int32), "margin": np.array(margin, np.float64),
            "hit32": np.array(hit32, np.float64), "normal32": np.array(normal32, np.float64)}


def batch(name, idx=None):
    """truth32_<name>.npz (its rays idx)."""
    orig, d, tnear = rays_of(name)
    idx = np.arange(len(orig)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(scene_of(name))
    out = _answers([truth.query(ts, orig[i].astype(np.float64), d[i].astype(np.float64), float(tnear[i]), f32=True)
                    for i in idx])
    out.update(orig=orig[idx], dir=d[idx], tnear=tnear[idx])
    return out


def picks(name, idx=None):
    """truth32_pick_<name>.npz: the positions, the truth's camera rays and answers."""
    xy = pick_xy(name)
    idx = np.arange(len(xy)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(scene_of(name))
    rows = [truth.pick(ts, PICK_W, PICK_H, float(xy[i, 0]), float(xy[i, 1]), f32=True) for i in idx]
    out = _answers([r[2:] for r in rows])
    out.update(xy=xy[idx], orig=np.array([r[0] for r in rows]), dir=np.array([r[1] for r in rows]))
    return out


def shade(name, idx=None):
    """truth32_shade_<name>.npz: truth._trace + truth.shade along make_rays'
    first N_SHADE rays (t_near unused), as shade_cases.truth_shade: colour,
    Counts, the primary hit's object, the margins."""
    mp = truth._mp()
    orig, d, _ = make_rays(name, N_SHADE)
    idx = np.arange(len(orig)) if idx is None else np.asarray(idx)
    ts = truth.TruthScene(scene_of(name))
    rgb, counts, obj, margin, hit32, normal32 = [], [], [], [], [], []
    for i in idx:
        st, mg = truth.Counts(), truth.Margin()
        o, dd = truth._vec(orig[i]), truth._vec(d[i])
        st.primary += 1
        ob, face, t, tests, hits = truth._trace(ts, o, dd, mp.inf, mg)
        st.tests += tests
        st.hits += hits
        col = truth.shade(ts, o, dd, ob, face, t, 1, mp.mpf(float(BIAS)), DEPTH, st, mg)
        rgb.append([float(x) for x in col])
        counts.append(st.tuple())
        obj.append(ob)
        margin.append(mg.m)
        hit32.append(mg.h32)
        normal32.append(mg.n32)
    return {"orig": orig[idx], "dir": d[idx], "rgb": np.array(rgb, np.float64),
            "counts": np.array(counts, np.int32), "obj": np.array(obj, np.int32),
            "margin": np.array(margin, np.float64), "hit32": np.array(hit32, np.float64),
            "normal32": np.array(normal32, np.float64)}


# ---- fixtures (no mpmath) -----------------------------------------------------------------------
def load(name):
    """tests/golden/truth32_<name>.npz as a dict of arrays."""
    with np.load(os.path.join(truth.GOLDEN, f"truth32_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def meta():
    with open(os.path.join(truth.GOLDEN, "truth32_meta.json")) as f:
        return json.load(f)


def threshold(name, m=None):
    """The exclusion threshold of a batch or pick set: EPS32, or the raised
    one truth32_meta.json records for it."""
    m = meta() if m is None else m
    return max(truth.EPS32, float(m.get("exclude", {}).get(name, 0.0)))


def decided(b, thr=truth.EPS32):
    """(hit decided, normal decided) per ray."""
    return b["hit32"] >= thr, b["normal32"] >= thr


# ---- the comparison ---------------------------------------------------------------------------
def compare(want, got, thr=truth.EPS32, t_bound=T_BOUND, n_bound=N_BOUND):
    """Answers `got` (t float32, obj, face, normal float32 or None) for the
    rays of `want` (a fixture, or rows of one) against the truth: on every
    ray whose hit margin reaches thr the object and the face equal; a miss
    echoes t_near bit for bit with face -1 and a zero normal; a hit's
    |t32 - t| / max(1, t) within t_bound; where the normal margin reaches thr
    as well the normal's largest component error within n_bound. Returns the
    largest (t, normal) errors."""
    ok, okn = decided(want, thr)
    obj, face = np.asarray(got["obj"]), np.asarray(got["face"])
    bad = np.flatnonzero(ok & ((obj != want["obj"]) | (face != want["face"])))
    assert bad.size == 0, [(int(i), int(obj[i]), int(face[i]), int(want["obj"][i]), int(want["face"][i]),
                            float(want["hit32"][i])) for i in bad[:8]]
    hit, miss = ok & (want["obj"] >= 0), ok & (want["obj"] < 0)
    t = np.asarray(got["t"])
    assert t.dtype == F32
    tn = want["tnear"] if "tnear" in want else np.full(len(t), np.inf, F32)
    assert t[miss].tobytes() == np.asarray(tn, F32)[miss].tobytes()
    assert (face[miss] == -1).all()
    t64 = t.astype(np.float64)
    e_t = np.abs(t64[hit] - want["t"][hit]) / np.maximum(1.0, want["t"][hit])
    assert e_t.max(initial=0.0) <= t_bound, (int(np.flatnonzero(hit)[e_t.argmax()]), float(e_t.max()))
    e_n = np.zeros(0)
    if got.get("normal") is not None:
        nrm = np.asarray(got["normal"], np.float64)
        assert not nrm[miss].any()
        hn = hit & okn
        e_n = np.abs(nrm[hn] - want["normal"][hn]).max(axis=1) if hn.any() else e_n
        assert e_n.max(initial=0.0) <= n_bound, (int(np.flatnonzero(hn)[e_n.argmax()]), float(e_n.max()))
    return float(e_t.max(initial=0.0)), float(e_n.max(initial=0.0))


# ---- the specification in numpy float32 ----------------------------------------------------------
def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(F32))


def scene32(scene):
    """The scene's inputs rounded to float32, per object: kind, o2w and w2o
    as (3, 3) matrices M[row][col] and a translation, and the shape."""
    recs = []
    for ob in scene.objects:
        g = ob.geometry
        m = np.asarray(g.objectToWorld, np.float64)
        w = np.linalg.inv(m)
        rec = {"o2w": _f(m[:3, :3].T), "w2o": _f(w[:3, :3].T), "w2o_t": _f(w[3, :3])}
        if isinstance(g, Sphere):
            rec.update(kind=0, r=_f(g.r))
        elif isinstance(g, Plane):
            rec.update(kind=1)
        elif isinstance(g, Box):
            rec.update(kind=2, vmin=_f(np.asarray(g.vmin)[:3]), vmax=_f(np.asarray(g.vmax)[:3]))
        else:
            rec.update(kind=3, V=_f(g.vertices), F=np.asarray(g.faces, np.int64))
        recs.append(rec)
    return recs


def camera32(scene):
    m = np.asarray(scene.cameraToWorld, np.float64)
    return {"c2w": _f(m[:3, :3].T), "pos": _f(m[3, :3]), "fov": _f(scene.fov)}


def perturb(a, rng):
    """Every non-zero finite entry of a float32 array moved to a neighbouring
    float32 number, up or down by the seeded rng (zeros stay exact zeros: a
    subnormal in their place is another input, not a rounding of this one)."""
    a = np.asarray(a, F32)
    up = rng.integers(0, 2, a.shape).astype(bool)
    moved = np.nextafter(a, np.where(up, F32(np.inf), F32(-np.inf)).astype(F32))
    return np.where((a != 0) & np.isfinite(a), moved, a).astype(F32)


def perturb_scene(recs, rng):
    out = []
    for rec in recs:
        out.append({k: (perturb(v, rng) if isinstance(v, np.ndarray) and v.dtype == F32 else v)
                    for k, v in rec.items()})
    return out


def _mul(M, v):
    """(3, 3) float32 matrix times (n, 3) float32 vectors, in float32."""
    return (v[:, 0:1] * M[:, 0] + v[:, 1:2] * M[:, 1]) + v[:, 2:3] * M[:, 2]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _slabs(vmin, vmax, o, d):
    """AABB.intersect: tmin per ray, -inf on a miss."""
    inv = F32(1.0) / d
    t0, t1 = (vmin - o) * inv, (vmax - o) * inv
    lo, hi = np.where(inv < 0, t1, t0), np.where(inv < 0, t0, t1)
    tmin, tmax = lo.max(1), hi.min(1)
    return np.where(tmin <= tmax, tmin, F32(-np.inf)).astype(F32)


def _mesh(rec, o, d):
    """TriangleMesh.intersect: (t, face); a ray that misses the mesh's box or
    starts inside it (entry t < 0) misses the mesh."""
    V, F = rec["V"], rec["F"]
    tb = _slabs(V.min(0), V.max(0), o, d)
    v0, v1, v2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    D, O = d[:, None, :], o[:, None, :]
    p = _cross(D, e2[None])
    det = _dot(e1[None], p)
    tv = O - v0[None]
    u = _dot(tv, p) / det
    q = _cross(tv, e1[None])
    v = _dot(D, q) / det
    t = _dot(e2[None], q) / det
    ok = (det >= F32(1e-6)) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0)
    t = np.where(ok, t, F32(np.inf))
    face = t.argmin(1)                          # the first of equal t: the lowest face index
    best = t[np.arange(len(o)), face]
    found = np.isfinite(best) & (tb >= 0)
    return np.where(found, best, F32(-np.inf)).astype(F32), np.where(found, face, -1)


def brute_force(recs, orig, d, tnear):
    """The written specification on float32 numbers, every
    operation rounded to float32: trace's loop over the objects in order, and
    the hit's normal with the 1.000001 truncation and, where every axis
    truncates to 0, the dominant axis. Returns a dict as compare takes it,
    with the per-ray accepted-hit count `hits`."""
    orig, d = np.asarray(orig, F32), np.asarray(d, F32)
    n = len(orig)
    best = np.array(tnear, F32)
    obj, face, hits = np.full(n, -1), np.full(n, -1), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for i, rec in enumerate(recs):
            o = _mul(rec["w2o"], orig) + rec["w2o_t"]
            dd = _mul(rec["w2o"], d)
            f = np.full(n, -1)
            if rec["kind"] == 0:
                a, b = _dot(dd, dd), F32(2.0) * _dot(dd, o)
                c = _dot(o, o) - rec["r"] * rec["r"]
                delta = b * b - F32(4.0) * a * c
                # (b == 0: sign(0) = 0, t1 = 0, t2 = c / 0; the truth gives such a ray margin 0, so it is never judged)
                t1 = ((-b - np.sign(b) * np.sqrt(delta)) / F32(2.0)) * a
                t2 = c / (a * t1)
                t = np.where(delta >= 0, np.minimum(t1, t2), F32(-np.inf))
            elif rec["kind"] == 1:
                t = np.where(np.abs(dd[:, 1]) > F32(1e-6), -o[:, 1] / dd[:, 1], F32(-np.inf))
            elif rec["kind"] == 2:
                t = _slabs(rec["vmin"], rec["vmax"], o, dd)
            else:
                t, f = _mesh(rec, o, dd)
            acc = (t >= 0) & (t < best)
            hits += acc
            best = np.where(acc, t, best).astype(F32)
            obj, face = np.where(acc, i, obj), np.where(acc, f, face)
        nrm = np.zeros((n, 3), F32)
        hw = orig + d * np.where(obj >= 0, best, F32(0.0))[:, None]
        for i, rec in enumerate(recs):
            sel = obj == i
            if not sel.any():
                continue
            h = _mul(rec["w2o"], hw[sel]) + rec["w2o_t"]
            if rec["kind"] == 0:
                k = h / np.sqrt(_dot(h, h))[:, None]
            elif rec["kind"] == 1:
                k = np.tile(np.array([0.0, 1.0, 0.0], F32), (len(h), 1))
            elif rec["kind"] == 2:
                c = (rec["vmin"] + rec["vmax"]) / F32(2.0)
                half = np.abs((rec["vmin"] - rec["vmax"]) / F32(2.0))
                q = (h - c) / half
                k = np.trunc(q * F32(1.000001))
                none = ~k.any(1)
                dom = np.abs(q).argmax(1)
                k[none, dom[none]] = np.where(q[none, dom[none]] < 0, F32(-1.0), F32(1.0))
                k = k / np.sqrt(_dot(k, k))[:, None]
            else:
                V, F = rec["V"], rec["F"][face[sel]]
                k = _cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
                k = k / np.sqrt(_dot(k, k))[:, None]
            nrm[sel] = _mul(rec["o2w"], k.astype(F32))
    return {"t": best, "obj": obj.astype(np.int32), "face": face.astype(np.int32), "normal": nrm, "hits": hits}


def camera_rays32(cam, w, h, xy):
    """castPrimaryRay (row a1) on float32 numbers."""
    x, y = np.asarray(xy, F32)[:, 0], np.asarray(xy, F32)[:, 1]
    r = F32(w) / F32(h)
    f = np.tan(cam["fov"] * F32(np.pi) / F32(180.0) / F32(2.0)).astype(F32)
    cx = ((F32(2.0) * x * r) / F32(w) - r) * f
    cy = (F32(1.0) - F32(2.0) * y / F32(h)) * f
    v = np.stack([cx, cy, np.full(len(x), -1.0, F32)], 1).astype(F32)
    v = v / np.sqrt(_dot(v, v))[:, None]
    return np.tile(cam["pos"], (len(x), 1)).astype(F32), _mul(cam["c2w"], v.astype(F32)).astype(F32)


PERTURB_SEED = 3232


def room(b, scene, thr=truth.EPS32, pick=False):
    """brute_force on the rays of fixture `b` (a pick set: on the float32
    camera rays of its positions), on the float32 inputs as they are and with
    every scene input and ray moved by one seeded float32 ulp (perturb):
    compare at a quarter of the bounds, and the per-ray hit counts equal on
    the decided rays. Returns the largest errors of both runs."""
    out = {}
    rng = np.random.default_rng(PERTURB_SEED)
    for moved in (False, True):
        recs, cam = scene32(scene), camera32(scene)
        if moved:
            recs = perturb_scene(recs, rng)
            cam = {k: perturb(v, rng) for k, v in cam.items()}
        if pick:
            orig, d = camera_rays32(cam, PICK_W, PICK_H, b["xy"])
            tn = np.full(len(orig), np.inf, F32)
        else:
            orig, d, tn = b["orig"], b["dir"], b["tnear"]
        if moved:
            orig, d, tn = perturb(orig, rng), perturb(d, rng), perturb(tn, rng)
        got = brute_force(recs, orig, d, tn)
        want = dict(b, tnear=tn)
        e_t, e_n = compare(want, got, thr, T_BOUND / 4, N_BOUND / 4)
        ok = decided(b, thr)[0]
        assert np.array_equal(got["hits"][ok], b["hits"][ok]), np.flatnonzero(ok & (got["hits"] != b["hits"]))[:8]
        out["t_moved" if moved else "t"] = e_t
        out["normal_moved" if moved else "normal"] = e_n
    return out
