"""Multiprecision truth: the reference's trace / shade path evaluated from its
written specification (the quirks list above that
table, the ray-query rules of include/rtmi.h) in 200-bit mpmath arithmetic.

It is neither the oracle nor a kernel and imports neither: from a Scene it
reads the double-precision inputs only (objectToWorld, radii, box bounds,
vertices and faces, materials, lights, camera, fov, bgColor), inverts the
matrices itself and forms the face normals itself. The one float64 shortcut
is the mesh prefilter (PREFILTER): a numpy Moeller-Trumbore with every bound
loosened picks the faces that get the multiprecision test.

Every answer carries its `margin`: the smallest relative distance from its
threshold of any decision the answer depends on. An answer with margin < EPS
is undecided: arithmetic in float64 may honestly decide it the other way, so
comparisons leave it out (the tests cap how many). The decisions:

  delta against 0 (sphere)                |delta| / max(b^2, |4ac|)
  |n.d| against 1e-6 (plane)              relative
  tmin against tmax (slabs)               relative (a box of no thickness on
                                          one axis, that slab binding both
                                          ends: its t against the other slabs'
                                          entries and exits; of no thickness
                                          on two axes: 0, a hit needs the two
                                          slabs' t equal)
  tmin against 0, t against 0             |t| |d| / (1 + |o|), object space
  det against 1e-6                        relative
  u against 0 and 1, v against 0,
  u + v against 1                         absolute (they are barycentric)
  t against t_near, closest t against
  every other accepted t (objects), the
  closest face's t against the runner-up  relative
  box normal p/|d| * 1.000001 against +-1 absolute
  a zero direction component with the
  origin on that slab's plane (NaN slab)  0

A face that misses contributes the largest distance among the tests it fails
(it stays a miss while one of them holds); a face that hits the smallest of
all its tests. Faces the prefilter drops fail a test by PREFILTER or more.
The float32 margin (frames only, judged against EPS32) leaves out one
decision: t against 0 of a shadow or reflection ray for the sphere, plane or
box it has just left. That distance is the caller's `bias` itself (1e-4 in
every float32 comparison of the suite: the offset SURVEY.md's "hard parts"
choose because float32 resolves it, some hundred float32 roundings of a
coordinate of 10); against EPS32 it would call every lit pixel undecided.
The AABB's tmax *= 1.0000000000000004 is a float64 rounding guard: left out
here, covered by EPS.

The float32 QUERY margins (Margin.h32, n32; query(f32=True), pick(f32=True),
and shade through the Margin it is handed) judge a float32 kernel on single
rays. They are the float32 margin with the box normal's truncation taken
apart. On the axis a box is hit on, v is 1.000001 by construction, a
distance of 1e-6 that would call every box hit undecided against EPS32; a
float32 kernel settles that axis by taking the dominant one when every axis
truncates to 0, so the axis with the largest |v| is left out. The other two
axes' distances to +-1 (a hit near an edge) decide the normal but not the
hit: the hit margin h32 covers object, face, t and the Stats, the normal
margin n32 is h32 and those two axes. A radiance is decided at n32 of its
whole path.

The fixture readers at the end (load, meta) need no mpmath."""
import json
import os

import numpy as np

EPS = 1e-9          # float64 comparisons: exclusion threshold, not a tolerance
EPS32 = 1e-4        # float32 frames
PREC = 200
PREFILTER = 1e-3    # loosening of the float64 face prefilter (at least 1e-6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SPHERE, PLANE, BOX, MESH = "sphere", "plane", "box", "mesh"
INF = float("inf")


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath.mp


def mpf(x):
    return _mp().mpf(float(x))


# ---- matrices: glm's m[col][row] arrays <-> rows of mpf -------------------------
def rows(m):
    """glm matrix (numpy, m[col][row]) -> M[row][col] of mpf (exact)."""
    mp = _mp()
    m = np.asarray(m, np.float64).reshape(4, 4)
    return [[mp.mpf(float(m[c][r])) for c in range(4)] for r in range(4)]


def to_glm(M):
    """M[row][col] -> numpy m[col][row], each entry rounded to float64."""
    return np.array([[float(M[r][c]) for r in range(4)] for c in range(4)], np.float64)


def mat_mul(A, B):
    return [[sum((A[r][k] * B[k][c] for k in range(4)), _mp().mpf(0)) for c in range(4)] for r in range(4)]


def mat_inverse(M):
    """Multiprecision inverse (LU); ZeroDivisionError if singular."""
    mp = _mp()
    inv = mp.inverse(mp.matrix(M))
    return [[inv[r, c] for c in range(4)] for r in range(4)]


def translation(v):
    mp = _mp()
    M = [[mp.mpf(int(r == c)) for c in range(4)] for r in range(4)]
    for r in range(3):
        M[r][3] = mp.mpf(float(v[r]))
    return M


def scaling(v):
    mp = _mp()
    return [[mp.mpf(float(v[r])) if r == c and r < 3 else mp.mpf(int(r == c)) for c in range(4)] for r in range(4)]


def rotation(axis, angle):
    """The right-handed rotation by `angle` (radians, a double) about `axis`:
    Rodrigues, R = cos I + sin [k]x + (1 - cos) k k^T, k the unit axis."""
    mp = _mp()
    k = [mp.mpf(float(a)) for a in axis[:3]]
    ln = mp.sqrt(sum(a * a for a in k))
    k = [a / ln for a in k]
    th = mp.mpf(float(angle))
    c, s = mp.cos(th), mp.sin(th)
    K = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    M = [[mp.mpf(int(r == c_)) for c_ in range(4)] for r in range(4)]
    for r in range(3):
        for q in range(3):
            M[r][q] = c * int(r == q) + s * K[r][q] + (1 - c) * k[r] * k[q]
    return M


def xf_point(M, p):
    return tuple(M[r][0] * p[0] + M[r][1] * p[1] + M[r][2] * p[2] + M[r][3] for r in range(3))


def xf_dir(M, d):
    return tuple(M[r][0] * d[0] + M[r][1] * d[1] + M[r][2] * d[2] for r in range(3))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return _mp().sqrt(_dot(a, a))


def _normalize(a):
    n = _norm(a)
    return (a[0] / n, a[1] / n, a[2] / n)


def _vec(a):
    mp = _mp()
    return tuple(mp.mpf(float(x)) for x in np.asarray(a, np.float64).reshape(-1)[:3])


def _rel(a, b):
    """Relative distance of two numbers, as a float."""
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    if abs(a) == INF or abs(b) == INF:
        return 1.0
    return abs(a - b) / max(abs(a), abs(b))


class Margin:
    """Running minimum of the decisions' distances: m of all of them, m32 of
    all but those add() is told to leave out of the float32 margin. h32 and
    n32 are the float32 QUERY margins (module docstring): h32 of what m32
    holds less the box normal's truncation (q32 = False), n32 of h32 and the
    truncation's edge axes (add_edge)."""
    __slots__ = ("m", "m32", "h32", "_e32")

    def __init__(self):
        self.m = self.m32 = self.h32 = self._e32 = 1.0

    def add(self, d, f32=True, q32=True):
        d = float(d)
        if d < self.m:
            self.m = d
        if f32 and d < self.m32:
            self.m32 = d
        if f32 and q32 and d < self.h32:
            self.h32 = d

    def add_edge(self, d):
        """A decision of the normal alone: in n32, in no other minimum."""
        self._e32 = min(self._e32, float(d))

    @property
    def n32(self):
        return min(self.h32, self._e32)


def _t_margin(t, o, d):
    """t against 0: |t| |d| against the scale of the origin."""
    return float(abs(t) * _norm(d) / (1 + _norm(o)))


# ---- a1: castPrimaryRay ---------------------------------------------------------
def cast_primary_ray(w, h, x, y, fov, c2w):
    """Row a1. c2w: rows of mpf (rows()) or a glm array. x, y: numbers or mpf.
    Returns (orig, dir), triples of mpf."""
    mp = _mp()
    C = c2w if isinstance(c2w, list) else rows(c2w)
    x, y = mp.mpf(x), mp.mpf(y)
    r = mp.mpf(int(w)) / int(h)
    f = mp.tan(mp.mpf(float(fov)) * mp.pi / 180 / 2)
    cx = ((2 * x * r) / int(w) - r) * f
    cy = (1 - 2 * y / int(h)) * f
    d = _normalize((cx, cy, mp.mpf(-1)))
    return (C[0][3], C[1][3], C[2][3]), xf_dir(C, d)


# ---- a4-a10: intersections (object space) -----------------------------------------
def sphere_intersect(r, o, d, mg):
    """Row a5; None for -inf."""
    mp = _mp()
    a = _dot(d, d)
    b = 2 * _dot(d, o)
    c = _dot(o, o) - r * r
    ac4 = 4 * a * c
    delta = b * b - ac4
    scale = max(b * b, abs(ac4))
    mg.add(abs(delta) / scale if scale else 0.0)
    if delta < 0:
        return None
    if b == 0:          # sign(0) = 0: t1 = 0, t2 = c / 0
        mg.add(0.0)
        return mp.mpf(0) if c >= 0 else mp.mpf("-inf")
    sgn = 1 if b > 0 else -1
    t1 = ((-b - sgn * mp.sqrt(delta)) / 2) * a      # the precedence quirk
    t2 = c / (a * t1)
    return min(t1, t2)


def plane_intersect(o, d, mg):
    """Row a6; None for -inf."""
    thr = _mp().mpf(1e-6)
    denom = d[1]
    mg.add(_rel(abs(denom), thr))
    if abs(denom) > thr:
        return -o[1] / denom
    return None


def aabb_intersect(vmin, vmax, o, d, mg):
    """Row a4: tmin, or None where the reference returns -inf."""
    tmin = tmax = None
    slabs = []
    for i in range(3):
        if d[i] == 0:                       # invDir = +-inf
            if o[i] == vmin[i] or o[i] == vmax[i]:
                mg.add(0.0)                 # 0 * inf: the NaN slab
                continue
            if vmin[i] < o[i] < vmax[i]:
                continue                    # (-inf, +inf)
            mg.add(min(abs(o[i] - vmin[i]), abs(o[i] - vmax[i])) / (1 + abs(o[i])))
            return None
        inv = 1 / d[i]
        t0, t1 = (vmin[i] - o[i]) * inv, (vmax[i] - o[i]) * inv
        if inv < 0:
            t0, t1 = t1, t0
        tmin = t0 if tmin is None or t0 > tmin else tmin
        tmax = t1 if tmax is None or t1 < tmax else tmax
        slabs.append((i, t0, t1))
    flat = [s for s in slabs if vmin[s[0]] == vmax[s[0]] and s[1] == tmin and s[2] == tmax]
    if flat:
        # a slab of no thickness binds both ends: its entry and its exit are
        # one number in any arithmetic, so tmin <= tmax rests on the other
        # slabs' entries staying below it and their exits above it
        # (tmin == tmax here, so the box is hit; a second flat slab binds at
        # the same t and adds _rel(tk, tk) = 0)
        k, tk = flat[0][0], flat[0][1]
        for i, t0, t1 in slabs:
            if i != k:
                mg.add(min(_rel(t0, tk), _rel(tk, t1)))
        return tmin
    mg.add(_rel(tmin, tmax))
    return tmin if tmin <= tmax else None


def ray_triangle(o, d, v0, v1, v2):
    """Row a8, single-sided. Returns (t or None, the face's margin)."""
    thr = _mp().mpf(1e-6)
    e1 = (v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2])
    e2 = (v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2])
    p = (d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0])
    det = _dot(e1, p)
    m_det = _rel(det, thr)
    if det < thr and m_det >= PREFILTER:
        return None, m_det                  # far below: u, v would not be meaningful
    tv = (o[0] - v0[0], o[1] - v0[1], o[2] - v0[2])
    u = _dot(tv, p) / det
    q = (tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0])
    v = _dot(d, q) / det
    tests = ((det >= thr, m_det), (u >= 0, abs(float(u))), (u <= 1, abs(float(1 - u))),
             (v >= 0, abs(float(v))), (u + v <= 1, abs(float(1 - u - v))))
    failed = [m for ok, m in tests if not ok]
    if failed:
        return None, max(failed)
    return _dot(e2, q) / det, min(m for _, m in tests)


def _prefilter(V, F, o, d):
    """float64 candidates: the faces that pass every test loosened by PREFILTER."""
    o = np.array([float(x) for x in o])
    d = np.array([float(x) for x in d])
    v0, v1, v2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    p = np.cross(d, e2)
    det = (e1 * p).sum(1)
    with np.errstate(all="ignore"):
        tv = o - v0
        u = (tv * p).sum(1) / det
        q = np.cross(tv, e1)
        v = (q * d).sum(1) / det
        L = 2 * PREFILTER
        keep = (det >= 1e-6 * (1 - L)) & (u >= -L) & (u <= 1 + L) & (v >= -L) & (u + v <= 1 + L)
    return np.flatnonzero(keep)


class _Mesh:
    def __init__(self, g):
        self.V = np.ascontiguousarray(g.vertices, np.float64)
        self.F = np.ascontiguousarray(g.faces, np.int64)
        self.vmin, self.vmax = _vec(self.V.min(0)), _vec(self.V.max(0))
        self._v, self._n = {}, {}

    def vert(self, i):
        if i not in self._v:
            self._v[i] = _vec(self.V[i])
        return self._v[i]

    def normal(self, f):
        """normalize(cross(v1 - v0, v2 - v0))."""
        if f not in self._n:
            v0, v1, v2 = (self.vert(int(i)) for i in self.F[f])
            a = tuple(v1[k] - v0[k] for k in range(3))
            b = tuple(v2[k] - v0[k] for k in range(3))
            self._n[f] = _normalize((a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]))
        return self._n[f]

    def intersect(self, o, d, mg):
        """Row a10: (t or None, face)."""
        tb = aabb_intersect(self.vmin, self.vmax, o, d, mg)
        if tb is None:
            return None, -1
        mg.add(_t_margin(tb, o, d))
        if tb < 0:
            return None, -1
        cand = _prefilter(self.V, self.F, o, d)
        if len(cand) < len(self.F):
            mg.add(PREFILTER)
        hits = []
        for f in cand:
            t, m = ray_triangle(o, d, *(self.vert(int(i)) for i in self.F[f]))
            mg.add(m)
            if t is None:
                continue
            mg.add(_t_margin(t, o, d))
            if t >= 0:
                hits.append((t, int(f)))
        if not hits:
            return None, -1
        hits.sort()                         # lowest t, then lowest face index
        if len(hits) > 1:
            mg.add(_rel(hits[0][0], hits[1][0]))
        return hits[0]


# ---- the scene ---------------------------------------------------------------------
class TruthScene:
    """The double-precision inputs of a Scene, lifted to mpf; worldToObject by
    a multiprecision inverse."""

    def __init__(self, scene):
        from rtmi.scene import Box, DistantLight, Plane, PointLight, Sphere, TriangleMesh
        mp = _mp()
        self.objects = []
        for ob in scene.objects:
            g = ob.geometry
            o2w = rows(g.objectToWorld)
            rec = {"o2w": o2w, "w2o": mat_inverse(o2w), "albedo": _vec(ob.material.albedo),
                   "refl": mp.mpf(float(ob.material.reflection))}
            if isinstance(g, Sphere):
                rec.update(kind=SPHERE, r=mp.mpf(float(g.r)))
            elif isinstance(g, Plane):
                rec.update(kind=PLANE)
            elif isinstance(g, Box):
                rec.update(kind=BOX, vmin=_vec(g.vmin), vmax=_vec(g.vmax))
            elif isinstance(g, TriangleMesh):
                rec.update(kind=MESH, mesh=_Mesh(g))
            else:
                raise TypeError(type(g).__name__)
            self.objects.append(rec)
        self.lights = []
        for l in scene.lights:
            if isinstance(l, DistantLight):
                self.lights.append(("distant", _vec(l.color), mp.mpf(float(l.intensity)), _vec(l.dir)))
            elif isinstance(l, PointLight):
                self.lights.append(("point", _vec(l.color), mp.mpf(float(l.intensity)), _vec(l.pos)))
            else:
                raise TypeError(type(l).__name__)
        self.c2w = rows(scene.cameraToWorld)
        self.fov = float(scene.fov)
        self.bg = _vec(scene.bgColor)


def _scene(scene):
    """A TruthScene as it is, a Scene lifted (and remembered by identity)."""
    if isinstance(scene, TruthScene):
        return scene
    if _scene.last[0] is not scene:
        _scene.last = (scene, TruthScene(scene))
    return _scene.last[1]


_scene.last = (None, None)


def _intersect(rec, o, d, mg):
    """(t or None, face) of one object for the object-space ray."""
    k = rec["kind"]
    if k == SPHERE:
        return sphere_intersect(rec["r"], o, d, mg), -1
    if k == PLANE:
        return plane_intersect(o, d, mg), -1
    if k == BOX:
        return aabb_intersect(rec["vmin"], rec["vmax"], o, d, mg), -1
    return rec["mesh"].intersect(o, d, mg)


def _trace(ts, orig, d, t_near, mg, src=-1):
    """Row a3 on mpf rays: (obj, face, t, tests, hits). src: the object a
    shadow or reflection ray leaves."""
    best, best_obj, best_face, hits = t_near, -1, -1, 0
    accepted = []
    for i, rec in enumerate(ts.objects):
        o_o, d_o = xf_point(rec["w2o"], orig), xf_dir(rec["w2o"], d)
        t, face = _intersect(rec, o_o, d_o, mg)
        if t is None:
            continue
        if rec["kind"] != MESH:             # the mesh has judged its own t against 0
            mg.add(_t_margin(t, o_o, d_o), f32=i != src)
        if t < 0:
            continue
        mg.add(_rel(t, t_near))
        if not t < t_near:
            continue
        accepted.append(t)
        if t < best:
            best, best_obj, best_face = t, i, face
            hits += 1
    accepted.sort()
    for a, b in zip(accepted, accepted[1:]):  # the order of any two decides the Stats' hits
        mg.add(_rel(a, b))
    return best_obj, best_face, best, len(ts.objects), hits


def trace(scene, orig, d, t_near=INF):
    """Row a3 for a world-space ray given in doubles, of a Scene or a
    TruthScene: (obj, face, t, tests, hits, margin); on a miss obj = face = -1
    and t = t_near."""
    mp = _mp()
    ts = _scene(scene)
    mg = Margin()
    tn = mp.mpf(float(t_near))
    obj, face, t, tests, hits = _trace(ts, _vec(orig), _vec(d), tn, mg)
    return obj, face, t, tests, hits, mg.m


# ---- a11: hit normal -----------------------------------------------------------------
def hit_normal(ts, obj, face, hit_w, mg=None):
    """Row a11: objectToWorld * n, not renormalised."""
    mp = _mp()
    mg = mg or Margin()
    rec = ts.objects[obj]
    k = rec["kind"]
    if k == MESH:
        n = rec["mesh"].normal(face)
    elif k == PLANE:
        n = (mp.mpf(0), mp.mpf(1), mp.mpf(0))
    else:
        h = xf_point(rec["w2o"], hit_w)
        if k == SPHERE:
            n = _normalize(h)
        else:
            bias = mp.mpf(1.000001)
            n, vs = [], []
            for i in range(3):
                c = (rec["vmin"][i] + rec["vmax"][i]) / 2
                half = abs((rec["vmin"][i] - rec["vmax"][i]) / 2)
                v = (h[i] - c) / half * bias
                mg.add(abs(float(abs(v) - 1)), q32=False)
                vs.append(v)
                n.append(mp.mpf(int(v)))    # truncation
            hit_axis = max(range(3), key=lambda i: abs(vs[i]))
            for i in range(3):              # the query margin: the hit axis is the dominant one
                if i != hit_axis:
                    mg.add_edge(abs(float(abs(vs[i]) - 1)))
            if not any(n):
                mg.add(0.0, q32=False)
                mg.add_edge(0.0)
                return (mp.nan, mp.nan, mp.nan)
            n = _normalize(tuple(n))
    return xf_dir(rec["o2w"], n)


def query(ts, orig, d, t_near=INF, f32=False):
    """What rt_trace_rays answers for one ray given in doubles (mpf triples
    are taken as they are): (obj, face, t, normal (3,), tests, hits, margin),
    t and the normal rounded to float64; a miss has t = t_near, normal 0.
    f32: the float32 query margins (hit, normal) follow the margin."""
    mp = _mp()
    ts = _scene(ts)
    mg = Margin()
    o = orig if isinstance(orig, tuple) else _vec(orig)
    dd = d if isinstance(d, tuple) else _vec(d)
    obj, face, t, tests, hits = _trace(ts, o, dd, mp.mpf(float(t_near)), mg)
    n = np.zeros(3)
    if obj >= 0:
        hit_w = tuple(o[i] + dd[i] * t for i in range(3))
        n = np.array([float(x) for x in hit_normal(ts, obj, face, hit_w, mg)])
    return (obj, face, float(t), n, tests, hits, mg.m) + ((mg.h32, mg.n32) if f32 else ())


def pick(ts, w, h, x, y, f32=False):
    """rt_pick_pixels: castPrimaryRay through the scene's camera (unrounded),
    traced with t_near = +inf. Returns (orig (3,), dir (3,)) + query()'s tuple."""
    ts = _scene(ts)
    o, d = cast_primary_ray(w, h, x, y, ts.fov, ts.c2w)
    f = lambda v: np.array([float(c) for c in v])
    return (f(o), f(d)) + query(ts, o, d, f32=f32)


# ---- a12-a15: shade, pixel -------------------------------------------------------------
class Counts:
    """Row a19, and the two ray counters the C-ABI adds."""
    FIELDS = ("primary", "tests", "hits", "shadow", "reflection")

    def __init__(self):
        self.primary = self.tests = self.hits = self.shadow = self.reflection = 0

    def tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


def shade(ts, orig, d, obj, face, t, depth, bias, max_depth, st, mg):
    """Row a13 (with a12 and a14): the colour of a traced ray, a triple of mpf."""
    mp = _mp()
    if obj < 0:
        return ts.bg
    rec = ts.objects[obj]
    hit_w = tuple(orig[i] + d[i] * t for i in range(3))
    n = hit_normal(ts, obj, face, hit_w, mg)
    col = [mp.mpf(0)] * 3
    s_orig = tuple(hit_w[i] + n[i] * bias for i in range(3))
    for kind, color, intensity, v in ts.lights:
        if kind == "distant":
            ldir, dist = v, mp.inf
            inten = tuple(c * intensity for c in color)
        else:
            L = tuple(hit_w[i] - v[i] for i in range(3))
            r2 = _dot(L, L)
            dist = mp.sqrt(r2)
            ldir = tuple(x / dist for x in L)
            inten = tuple(c * intensity / (4 * mp.pi * r2) for c in color)
        to_light = tuple(-x for x in ldir)
        st.shadow += 1
        s_obj, _, _, tests, hits = _trace(ts, s_orig, to_light, dist, mg, obj)
        st.tests += tests
        st.hits += hits
        if s_obj < 0:
            lam = max(mp.mpf(0), _dot(n, to_light))
            col = [col[i] + rec["albedo"][i] / mp.pi * inten[i] * lam for i in range(3)]
    refl = rec["refl"]
    if refl > 0 and depth <= max_depth:
        k = 2 * _dot(n, d)
        r = tuple(d[i] - k * n[i] for i in range(3))
        r_orig = tuple(hit_w[i] + r[i] * bias for i in range(3))
        st.reflection += 1
        r_obj, r_face, r_t, tests, hits = _trace(ts, r_orig, r, mp.inf, mg, obj)
        st.tests += tests
        st.hits += hits
        rc = shade(ts, r_orig, r, r_obj, r_face, r_t, depth + 1, bias, max_depth, st, mg) if r_obj >= 0 else ts.bg
        col = [(1 - refl) * col[i] + refl * rc[i] for i in range(3)]
    return tuple(col)


def grid(m):
    """Row a16's grid for an m x m table: ((i + 1/2) / m, (j + 1/2) / m), j outer."""
    mp = _mp()
    return [((mp.mpf(i) + mp.mpf(1) / 2) / m, (mp.mpf(j) + mp.mpf(1) / 2) / m) for j in range(m) for i in range(m)]


def sample(ts, w, h, x, y, bias, max_depth, st, mg):
    """One primary sample at image position (x, y): its colour."""
    mp = _mp()
    orig, d = cast_primary_ray(w, h, x, y, ts.fov, ts.c2w)
    st.primary += 1
    obj, face, t, tests, hits = _trace(ts, orig, d, mp.inf, mg)
    st.tests += tests
    st.hits += hits
    return shade(ts, orig, d, obj, face, t, 1, mp.mpf(float(bias)), int(max_depth), st, mg)


def pixel(ts, w, h, x, y, m=0, bias=1e-4, max_depth=5):
    """Row a15: akNone (m = 0: one sample at the pixel's corner) or akGrid m.
    Returns (rgb as float64 (3,), Counts tuple, margin, float32 margin)."""
    mp = _mp()
    ts = _scene(ts)
    st, mg = Counts(), Margin()
    if m == 0:
        col = sample(ts, w, h, x, y, bias, max_depth, st, mg)
    else:
        col = [mp.mpf(0)] * 3
        pts = grid(m)
        for sx, sy in pts:
            c = sample(ts, w, h, x + sx, y + sy, bias, max_depth, st, mg)
            col = [col[i] + c[i] for i in range(3)]
        col = [c * (mp.mpf(1) / len(pts)) for c in col]
    return np.array([float(c) for c in col]), st.tuple(), mg.m, mg.m32


# ---- the output quantiser (framebuf.nim writePpm's outvalue) ---------------------------
def _f32(x):
    """An mpf rounded to the nearest float32 (ties to even), as an exact mpf."""
    mp = _mp()
    return mp.mpf(float(np.float32(float(x)))) if abs(x) < 1e30 else x


def quantise(values, bits, srgb):
    """clamp to [0, 1] -> optional linearToSRGB -> round(c * (2^bits - 1)),
    half away from zero, with the reference's types: the transfer's result and
    the product are float32. Returns (q int64, undecided bool): undecided where
    the exactly scaled value lies within 1e-6 of a half, or the transfer's
    exact value within 1e-13 (relative: a thousand float64 roundings of the
    reference's pow) of the middle of two float32 numbers.
    NaN is left to the callers (the reference's clamp does not define it)."""
    mp = _mp()
    maxval = 2 ** int(bits) - 1
    q = np.zeros(len(values), np.int64)
    und = np.zeros(len(values), bool)
    for i, v in enumerate(np.asarray(values, np.float32)):
        c = mp.mpf(float(min(max(v, np.float32(0.0)), np.float32(1.0))))
        if srgb:
            if c <= mp.mpf(0.0031308):
                e = mp.mpf(12.92) * c
            else:
                e = (1 + mp.mpf(0.055)) * mp.power(c, 1 / mp.mpf(2.4)) - mp.mpf(0.055)
            c32 = _f32(e)
            f = np.float32(float(c32))
            lo, hi = np.nextafter(f, np.float32(-1)), np.nextafter(f, np.float32(2))
            for nb in (lo, hi):
                mid = (c32 + mp.mpf(float(nb))) / 2
                if e != 0 and abs(e - mid) / abs(e) < 1e-13:
                    und[i] = True
            s = e * maxval
        else:
            c32, s = c, c * maxval
        if abs((s - mp.floor(s)) - mp.mpf(1) / 2) < 1e-6:
            und[i] = True
        x = _f32(c32 * maxval)
        fl = mp.floor(x)
        q[i] = int(fl) + (1 if x - fl >= mp.mpf(1) / 2 else 0)
    return q, und


# ---- fixtures (no mpmath) -----------------------------------------------------------------
def load(name):
    """tests/golden/truth_<name>.npz as a dict of arrays."""
    with np.load(os.path.join(GOLDEN, f"truth_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def meta():
    with open(os.path.join(GOLDEN, "truth_meta.json")) as f:
        return json.load(f)


def vec_ulps(a, b):
    """Error of vectors or matrices (last axes flattened per item of axis 0)
    in units of the float64 spacing at b's largest entry: an entry that is 0
    up to rounding has no spacing of its own to be measured in."""
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    big = np.abs(b).max(1)
    return np.abs(a - b).max(1) / np.spacing(np.where(big > 0, big, 1.0))


def ulps(a, b):
    """|a - b| in units of the float64 spacing at b (elementwise)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.abs(b)))


def within_f32_ulp(got, truth64, n=1):
    """got (float32 or float64 colour) within n float32 ulps of truth rounded to float32."""
    t32 = np.asarray(truth64, np.float64).astype(np.float32)
    g = np.asarray(got, np.float64)
    return np.abs(g - t32.astype(np.float64)) <= n * np.spacing(np.abs(t32)).astype(np.float64)
