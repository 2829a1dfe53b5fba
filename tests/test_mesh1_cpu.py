"""The mesh pixels' inset box (rt_bins_geom.h inset_box and lemma 1, rt_common.h
inset_inside, rt_fast.h gen1_batch) on the host: a shadow origin strictly
inside the inset box fails the mesh's box gate for every light, so the kernel
skips the gate there.

The hook (rt_hooks.cpp rtmi_test_mesh1) forms the box through the function a
render call forms it with, applies the kernel's inside test, and evaluates a
float32 restatement of mesh_gate with fmaf where the kernel has an FMA. The
reciprocals ni are an input, so every case is also tried with each of them one
ulp either side of the correctly rounded value (v_rcp is not correctly
rounded)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from rtmi._lib import lib

_P = C.c_void_p
F32 = np.float32
INF = F32(np.inf)


def mesh1(lo, hi, lights, ro=None, ni=None):
    """(box6, inside, gate) of rtmi_test_mesh1."""
    f = lib().rtmi_test_mesh1
    f.restype = C.c_int
    f.argtypes = [_P, _P, _P, C.c_int32, _P, C.c_int64, _P, _P, _P, _P]
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    li = np.ascontiguousarray(np.asarray(lights, F32).reshape(-1, 3))
    ro = np.zeros((0, 3), F32) if ro is None else np.ascontiguousarray(ro, F32)
    ni = np.zeros((0, 3), F32) if ni is None else np.ascontiguousarray(ni, F32)
    assert ro.shape == ni.shape and ro.shape[1] == 3
    n = len(ro)
    box = np.zeros(6, F32)
    inside, gate = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    rc = f(lo.ctypes.data, hi.ctypes.data, li.ctypes.data, len(li), box.ctypes.data, n, ro.ctypes.data, ni.ctypes.data,
           inside.ctypes.data, gate.ctypes.data)
    assert rc == 0, rc
    return box, inside[:n], gate[:n]


def slab_ni(d):
    """slab_ray's reciprocals of the directions d (n, 3), correctly rounded:
    components under 1e-20 in magnitude become +-1e-20 (the sign of a zero too)."""
    d = np.asarray(d, F32)
    e = F32(1e-20)
    c = np.where(np.abs(d) < e, np.copysign(e, d), d).astype(F32)
    return (1.0 / c.astype(np.float64)).astype(F32)


def ulps(x, k):
    """x moved by k float32 steps (away from zero for k > 0)."""
    return (x.view(np.int32) + np.int32(k)).view(F32)


def expected_box(lo, hi):
    lo64, hi64 = np.asarray(lo, F32).astype(np.float64), np.asarray(hi, F32).astype(np.float64)
    m = 2.0 ** -12 * max(np.abs(lo64).max(), np.abs(hi64).max())
    return np.concatenate([np.nextafter((lo64 + m).astype(F32), INF), np.nextafter((hi64 - m).astype(F32), -INF)]), m


WARM = [(-0.5, -0.8, -0.3), (0.6, -0.7, 0.2)]

# scale 1e-3, 1 and 1e6, centred and off-centre by 1e3 times the size
BOXES = []
for scale in (1e-3, 1.0, 1e6):
    for off in (0.0, 1e3):
        c = np.array([off, -0.7 * off, 0.3 * off]) * scale
        BOXES.append((c + scale * np.array([-0.5, -0.31, -0.77]), c + scale * np.array([0.5, 0.43, 0.6])))

COMPONENTS = (0.0, -0.0, 1e-21, -1e-21, 1e-6, -1e-6, 1e6, -1e6, 0.37, -1.0)


def _assert_lemma1(lo, hi, ro, d, what):
    """Every origin is inside and no gate is true, for ni and ni +- 1 ulp."""
    ni0 = slab_ni(d)
    assert np.all(np.abs(ni0) >= F32(0.99e-6)) and np.all(np.abs(ni0) <= F32(1.01e20))
    for k in (-1, 0, 1):
        box, inside, gate = mesh1(lo, hi, WARM, ro, ulps(ni0, k))
        assert inside.all(), (what, k, int((inside == 0).sum()))
        bad = np.flatnonzero(gate)
        assert len(bad) == 0, (what, k, len(bad), ro[bad[:3]], d[bad[:3]], box)


@pytest.mark.parametrize("b", range(len(BOXES)))
def test_lemma1_adversarial(b):
    """Origins exactly one float inside each inset bound (the 8 corners, and
    each bound with the other axes anywhere inside), light components 0,
    +-1e-21, +-1e-6 and +-1e6 on every axis in every combination."""
    lo, hi = BOXES[b]
    box, _, _ = mesh1(lo, hi, WARM)
    want, m = expected_box(lo, hi)
    assert np.array_equal(box, want), (box, want)
    assert np.all(box[:3] < box[3:])
    near_lo, near_hi = np.nextafter(box[:3], INF), np.nextafter(box[3:], -INF)
    mid = ((box[:3].astype(np.float64) + box[3:]) / 2).astype(F32)
    origins = [np.where(np.array(c, bool), near_hi, near_lo) for c in itertools.product((0, 1), repeat=3)]
    for ax in range(3):
        for edge in (near_lo, near_hi):
            o = mid.copy()
            o[ax] = edge[ax]
            origins.append(o)
    origins = np.array(origins, F32)
    dirs = np.array(list(itertools.product(COMPONENTS, repeat=3)), F32)
    ro = np.repeat(origins, len(dirs), axis=0)
    d = np.tile(dirs, (len(origins), 1))
    _assert_lemma1(lo, hi, ro, d, ("box", b))


def test_lemma1_random():
    """Seeded: boxes of scale 1e-3 .. 1e6 up to 1e3 sizes off centre, origins
    anywhere strictly inside the inset box (its bounds' neighbours included),
    direction components of magnitude 1e-25 .. 1e6, some exactly zero."""
    rng = np.random.default_rng(20261020)
    total = 0
    for _ in range(100):
        scale = 10.0 ** rng.uniform(-3, 6)
        c = rng.uniform(-1, 1, 3) * scale * 10.0 ** rng.uniform(-2, 3)
        half = scale * rng.uniform(0.2, 1.0, 3)
        lo, hi = (c - half).astype(F32), (c + half).astype(F32)
        box, _, _ = mesh1(lo, hi, WARM)
        if not np.all(box[:3] < box[3:]):  # (a box thinner than its margin: nothing to prove)
            continue
        n = 20000
        u = rng.uniform(0, 1, (n, 3))
        u[rng.uniform(size=(n, 3)) < 0.1] = 0.0
        u[rng.uniform(size=(n, 3)) < 0.1] = 1.0
        near_lo, near_hi = np.nextafter(box[:3], INF), np.nextafter(box[3:], -INF)
        ro = (near_lo.astype(np.float64) * (1 - u) + near_hi.astype(np.float64) * u).astype(F32)
        ro = np.clip(ro, near_lo, near_hi)
        d = (10.0 ** rng.uniform(-25, 6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F32)
        d[rng.uniform(size=(n, 3)) < 0.05] = 0.0
        _assert_lemma1(lo, hi, ro, d, ("random", float(scale)))
        total += n
    assert total >= 1_000_000, total


def test_the_restated_gate_is_the_reference_gate():
    """Not vacuous: from outside, towards the box, the gate is true; from
    inside the box but outside the inset box the lemma says nothing and the
    inside test says no; a ray that points away misses."""
    lo, hi = np.array([-1, -1, -1], F32), np.array([1, 1, 1], F32)
    ro = np.array([[0, 5, 0], [0, 5, 0], [0.99999, 0, 0], [0, 0, 0]], F32)
    d = np.array([[0, -1, 0], [0, 1, 0], [0.3, -0.5, 0.1], [0.3, -0.5, 0.1]], F32)
    box, inside, gate = mesh1(lo, hi, WARM, ro, slab_ni(d))
    assert list(gate) == [1, 0, 0, 0] and list(inside) == [0, 0, 0, 1], (gate, inside, box)


EMPTY = np.array([np.inf] * 3 + [-np.inf] * 3, F32)


def _passes_nobody(lo, hi, lights):
    box, _, _ = mesh1(lo, hi, lights)
    assert np.array_equal(box, EMPTY), box
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ro = np.array([(lo64 + hi64) / 2, lo64, hi64, [0, 0, 0], [np.nan] * 3, [np.inf] * 3], F32)
    _, inside, _ = mesh1(lo, hi, lights, ro, np.ones_like(ro))
    assert not inside.any(), inside


def test_flat_mesh_passes_no_lane():
    """in_lo >= in_hi on one axis: a flat mesh, and a slab thinner than twice
    the margin."""
    _passes_nobody([-1, 0.25, -1], [1, 0.25, 1], WARM)
    _passes_nobody([-1, 0.25, -1], [1, 0.25 + 2.0 ** -12, 1], WARM)
    _passes_nobody([100, 100, 100], [100.01, 100.01, 100.01], WARM)  # margin 0.024 of |coordinates| 100


def test_light_beyond_1e6_empties_the_box():
    lo, hi = BOXES[2]
    assert np.array_equal(mesh1(lo, hi, [(0.1, -1e6, 0.2)])[0], expected_box(lo, hi)[0])
    _passes_nobody(lo, hi, [(0.1, -2e6, 0.2)])
    _passes_nobody(lo, hi, WARM + [(2e6, -0.5, 0.0)])
    _passes_nobody(lo, hi, [(float(np.nextafter(F32(1e6), INF)), -0.5, 0.0)])
    _passes_nobody(lo, hi, [(np.nan, -0.5, 0.0)])


def test_scale_limits():
    """m >= 1e-25 and |coordinates| <= 1e15, either side."""
    for s, ok in ((5e-22, True), (3e-22, False), (1e15, True), (1.1e15, False)):
        lo, hi = np.array([-s, -s, -s], F32), np.array([s, s, s], F32)
        if ok:
            box, _, _ = mesh1(lo, hi, WARM)
            assert np.array_equal(box, expected_box(lo, hi)[0]) and np.all(box[:3] < box[3:]), (s, box)
        else:
            _passes_nobody(lo, hi, WARM)
    _passes_nobody([-1, np.nan, -1], [1, 1, 1], WARM)
    _passes_nobody([-1, -1, -1], [1, np.inf, 1], WARM)
