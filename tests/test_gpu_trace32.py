"""Float32 ray queries and picks (DeviceScene.trace_rays_f32 / pick_f32,
rt_trace_rays_f32* / rt_pick_pixels_f32*) on the device.

1. Picks agree with the picture, exactly: on the coverage scenes (black
   objects under a sky of 1: a float32 frame encodes per pixel how many
   samples hit) the picks at a pixel's sample positions hit as many times as
   the RT_FP32 frame shows, with the default flags and with
   RT_FLAG_NO_BINNING, on every pixel, before and after set_camera.
2. Against the reference: all 16 specialisations of k_trace_rays_f32 on the
   float32-rounded rays of the 96 x 64 akGrid m = 2 frame, against the float64
   query (bit-exact against the oracle, test_gpu_query.py) on the same values:
   (obj, face) equal on 99.9 % of the rays, t and the normal within T_BOUND /
   N_BOUND on the agreeing hits, any-hit under the same cap, the Stats, and
   pick_f32 against the float64 pick likewise.
3. Any-hit hits exactly where the closest-hit query hits.
4. The independence rule, bit for bit.
5. The contract: t_near, degenerate rays, unnormalised directions, scene
   edits, the render state, the error codes.

RTMI_PARITY_LOG=<file> appends the measured distances of test 2
(profiles/trace32/parity_fp32.jsonl).

T_BOUND and N_BOUND are 4 times the largest value measured on the MI355X over
the 16 scenes, rays and picks (profiles/trace32/parity_fp32.jsonl), rounded up
to one significant digit (the margin covers compiler-version differences in
contraction):
  relative error of t, |t32 - t64| / max(1, t64): largest 3.4e-5, on picks of
    scenes with spheres (rays: 1.5e-5; without spheres 4.1e-6 and 1.5e-6; the
    99th percentile is at most 2.3e-6)                        -> T_BOUND 2e-4
  largest component error of the normal: largest 3.3e-4, again on the
    spheres (without them 1.0e-7; the 99th percentile is at most 1.2e-5, the
    99.9th 5.0e-5; no hit of these frames took a neighbouring box face's
    normal)                                                   -> N_BOUND 2e-3
(obj, face) agreed on every ray of every scene, and the float32 hit counts
equalled the float64 ones.
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

import coverage_scenes as cs
import shade_cases as sc
import subset_scenes as ss
import trace32_cases as t32
from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi import abi
from rtmi._lib import RtmiError, lib
from rtmi.glm import point, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import PointLight, Stats, TriangleMesh

pytestmark = pytest.mark.gpu

T_BOUND = 2e-4
N_BOUND = 2e-3
CAP = 0.999
INF32 = np.float32(np.inf)
_fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731


def _np(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Got:
    """One call's answers as numpy arrays, and its Stats."""

    def __init__(self, res, normals):
        res = list(res)
        self.t, self.obj, self.face = (_np(x) for x in res[:3])
        self.normals = _np(res[3]) if normals else None
        self.stats = res[-1]
        assert self.t.dtype == np.float32 and self.obj.dtype == np.int32 and self.face.dtype == np.int32
        assert self.normals is None or self.normals.dtype == np.float32

    def raw(self):
        n = b"" if self.normals is None else self.normals.tobytes()
        return self.t.tobytes() + self.obj.tobytes() + self.face.tobytes() + n

    def take(self, idx):
        g = object.__new__(Got)
        g.t, g.obj, g.face = self.t[idx], self.obj[idx], self.face[idx]
        g.normals = None if self.normals is None else self.normals[idx]
        g.stats = None
        return g


def trace32(ds, orig, d, tn=None, device=False, normals=True, **kw):
    if device:
        orig, d, tn = _dev(orig), _dev(d), _dev(tn)
    return Got(ds.trace_rays_f32(orig, d, tn, normals=normals, stats=True, **kw), normals)


def pick32(ds, o, xy, device=False, normals=True, **kw):
    return Got(ds.pick_f32(o, _dev(xy) if device else xy, normals=normals, stats=True, **kw), normals)


def same(got, want, stats=True):
    assert got.raw() == want.raw(), np.flatnonzero((got.obj != want.obj) | (got.t != want.t))[:8]
    if stats:
        assert got.stats == want.stats, (got.stats, want.stats)


def pick_opts(w, h, precision=Precision.fp32):
    return Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=precision)


@functools.lru_cache(maxsize=None)
def device_scene(bits):
    return DeviceScene(ss.subset_scene(bits))


# ---- 1. picks agree with the picture ---------------------------------------------------------
SAMPLINGS = ((akNone, 1), (akGrid, 2), (akGrid, 4))


def _render(ds, o):
    import torch
    fb = torch.zeros(o.height * o.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb)
    return fb.view(o.height, o.width, 3).cpu().numpy(), st


def _sample_xy(kind, m):
    """(H, W, spp, 2) float32: the image positions of every sample, exact in float32."""
    rows = [cs.row_positions(kind, m, 0, y) for y in range(cs.H)]
    xy = np.stack([np.stack([px, py], -1) for px, py in rows])
    xy32 = xy.astype(np.float32)
    assert np.array_equal(xy32.astype(np.float64), xy)
    return xy32


@pytest.mark.parametrize("kind,m", SAMPLINGS, ids=["none", "grid2", "grid4"])
@pytest.mark.parametrize("name", cs.SCENES)
def test_picks_agree_with_the_picture(gpu, name, kind, m):
    scene = cs.scene(name)
    ds = DeviceScene(scene)
    spp = cs.spp_of(kind, m)
    xy = _sample_xy(kind, m)
    moved = np.array(scene.cameraToWorld, np.float64)
    moved[3, 2] += 0.1
    for cam in (None, moved):
        if cam is not None:
            ds.set_camera(cam, scene.fov)
        got = pick32(ds, pick_opts(cs.W, cs.H), xy.reshape(-1, 2), device=cam is not None)
        assert got.stats.numPrimaryRays == cs.W * cs.H * spp
        picked = (got.obj.reshape(cs.H, cs.W, spp) >= 0).sum(axis=2)
        assert 0 < picked.sum() < cs.W * cs.H * spp
        for flags in (0, abi.RT_FLAG_NO_BINNING):
            frame, st = _render(ds, cs.options(kind, m, 0, Precision.fp32, flags))
            assert st.numPrimaryRays == cs.W * cs.H * spp
            hits, off = cs.hit_counts(name, frame, spp)
            assert off.max() <= 0.05
            bad = np.argwhere(picked != hits)
            assert bad.size == 0, (name, int(kind), m, flags, cam is not None,
                                   [(int(x), int(y), int(picked[y, x]), int(hits[y, x])) for y, x in bad[:8]])
    ds.close()


# ---- 2. against the reference ------------------------------------------------------------------
def _log(row):
    print(json.dumps(row))
    path = os.environ.get("RTMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _quantile(err, q):
    """The smallest value that at least the share q of err does not exceed."""
    s = np.sort(err)
    return float(s[max(0, math.ceil(q * len(s)) - 1)]) if len(s) else 0.0


def _judge(what, got, ref64, n, nobj, primary):
    """got (float32 query) against ref64 = (t, obj, face, normals, Stats) of the float64 query."""
    t64, obj64, face64, n64, st64 = ref64
    agree = (got.obj == obj64) & (got.face == face64)
    k = agree & (obj64 >= 0)
    t_err = np.abs(got.t[k].astype(np.float64) - t64[k]) / np.maximum(1.0, t64[k])
    n_err = np.abs(got.normals[k].astype(np.float64) - n64[k]).max(axis=1)
    row = {"what": what, "rays": int(n), "agree": float(agree.mean()), "agreeing_hits": int(k.sum()),
           "t_rel_max": float(t_err.max()), "t_rel_p99": _quantile(t_err, 0.99),
           "normal_max": float(n_err.max()), "normal_p99": _quantile(n_err, 0.99),
           "normal_p999": _quantile(n_err, CAP),
           "hits32": int(got.stats.numIntersectionHits), "hits64": int(st64.numIntersectionHits)}
    _log(row)
    assert k.sum() >= n // 10, row
    assert row["agree"] >= CAP, row
    assert row["t_rel_max"] <= T_BOUND, row
    assert row["normal_p999"] <= N_BOUND, row
    # a miss: t_near echoed, no face, a zero normal
    miss = got.obj < 0
    assert miss.any() and (got.t[miss] == INF32).all() and (got.face[miss] == -1).all()
    assert not got.normals[miss].any()
    assert got.stats.numIntersectionTests == n * nobj, (what, got.stats)
    assert got.stats.numIntersectionHits == pytest.approx(st64.numIntersectionHits, rel=1e-2), (what, got.stats, st64)
    assert got.stats.numPrimaryRays == (n if primary else 0)
    assert got.stats.numShadowRays == 0 and got.stats.numReflectionRays == 0


@pytest.mark.parametrize("bits", t32.GEOMETRY_BITS)
def test_every_specialisation_against_the_float64_query(gpu, oracle_mod, bits):
    orig, d = t32.frame_rays(oracle_mod)
    n = len(orig)
    scene = ss.subset_scene(bits)
    nobj = len(scene.objects)
    ds = DeviceScene(scene)
    assert ds.trace32_subset() == bits
    name = f"subset {bits} {ss.subset_name(bits)}"
    o64, d64 = orig.astype(np.float64), d.astype(np.float64)
    ref64 = ds.trace_rays(o64, d64, normals=True, stats=True)
    got = trace32(ds, orig, d)
    _judge(name + " trace_rays_f32", got, ref64, n, nobj, False)
    # any-hit: hit or no hit, under the same cap
    any64 = ds.trace_rays(o64, d64, any_hit=True, stats=True)
    anyhit = trace32(ds, orig, d, any_hit=True, normals=False)
    assert float(((anyhit.obj >= 0) == (any64[1] >= 0)).mean()) >= CAP
    assert (anyhit.face == -1).all() and (anyhit.t == INF32).all()
    assert anyhit.stats.numIntersectionTests == n * nobj
    assert anyhit.stats.numIntersectionHits == pytest.approx(any64[-1].numIntersectionHits, rel=1e-2)
    # picks at the same image positions against the float64 pick
    xy = t32.frame_xy()
    p64 = ds.pick(pick_opts(ss.W, ss.H, Precision.fp64), xy, normals=True, stats=True)
    picked = pick32(ds, pick_opts(ss.W, ss.H), xy.astype(np.float32))
    _judge(name + " pick_f32", picked, p64, n, nobj, True)
    ds.close()


# ---- 3. any-hit hits exactly where the closest-hit query hits ----------------------------------
@pytest.mark.parametrize("bits", t32.GEOMETRY_BITS)
def test_any_hit_equals_closest_hit(gpu, oracle_mod, bits):
    orig, d = t32.frame_rays(oracle_mod)
    ds = device_scene(bits)
    free = trace32(ds, orig, d, device=True, normals=False)
    anyhit = trace32(ds, orig, d, device=True, normals=False, any_hit=True)
    assert np.array_equal(anyhit.obj >= 0, free.obj >= 0)
    assert (free.obj >= 0).any() and (free.obj < 0).any()
    # a finite t_near either side of the hit (20 where the unrestricted ray misses)
    f = np.random.default_rng(300 + bits).uniform(0.5, 2.0, len(orig)).astype(np.float32)
    tn = np.where(free.obj >= 0, f * free.t, np.float32(20.0)).astype(np.float32)
    near = trace32(ds, orig, d, tn, device=True, normals=False)
    anynear = trace32(ds, orig, d, tn, device=True, normals=False, any_hit=True)
    assert np.array_equal(anynear.obj >= 0, near.obj >= 0)
    share = float((near.obj >= 0).mean())
    assert 0.05 <= share <= 0.95, share
    assert sc.same_bits(anynear.t, tn) and (anynear.face == -1).all()
    assert sc.same_bits(near.t[near.obj < 0], tn[near.obj < 0])


# ---- 4. independence, bit for bit --------------------------------------------------------------
def _sum_stats(a, b):
    total = Stats()
    total += a
    total += b
    return total


def _concat(a, b, normals=True):
    g = object.__new__(Got)
    g.t, g.obj, g.face = (np.concatenate([getattr(a, k), getattr(b, k)]) for k in ("t", "obj", "face"))
    g.normals = np.concatenate([a.normals, b.normals]) if normals else None
    g.stats = _sum_stats(a.stats, b.stats)
    return g


@pytest.mark.parametrize("bits", [15, 7])
def test_independence(gpu, oracle_mod, bits):
    orig, d = t32.small_rays(oracle_mod)
    n = len(orig)
    ds = device_scene(bits)
    free = trace32(ds, orig, d)
    assert (free.obj >= 0).any() and (free.obj < 0).any()
    f = np.random.default_rng(40 + bits).uniform(0.5, 2.0, n).astype(np.float32)
    near = np.where(free.obj >= 0, f * free.t, np.float32(15.0)).astype(np.float32)
    for tn in (None, near):
        cut_tn = (lambda a, b: None) if tn is None else (lambda a, b: tn[a:b].copy())
        base = trace32(ds, orig, d, tn)
        assert base.stats.numIntersectionTests == n * len(ss.subset_scene(bits).objects)
        for kw in ({"sort": True}, {"device": True}, {"device": True, "sort": True}):
            same(trace32(ds, orig, d, tn, **kw), base)
        # without normals: the same hits
        plain = trace32(ds, orig, d, tn, normals=False)
        assert plain.raw() == base.raw()[:len(plain.raw())] and plain.stats == base.stats   # (raw: the normals last)
        base_any = trace32(ds, orig, d, tn, normals=False, any_hit=True)
        for kw in ({"sort": True}, {"device": True, "sort": True}):
            same(trace32(ds, orig, d, tn, normals=False, any_hit=True, **kw), base_any)
        # a seeded permutation of the batch, the answers un-permuted
        perm = np.random.default_rng(32 + bits).permutation(n)
        for sort in (False, True):
            got = trace32(ds, orig[perm].copy(), d[perm].copy(), None if tn is None else tn[perm].copy(), sort=sort)
            back = object.__new__(Got)
            for k in ("t", "obj", "face", "normals"):
                a = np.empty_like(getattr(got, k))
                a[perm] = getattr(got, k)
                setattr(back, k, a)
            back.stats = got.stats
            same(back, base)
        # one call and two calls
        for cut in (64, 65, 100):
            a = trace32(ds, orig[:cut].copy(), d[:cut].copy(), cut_tn(0, cut))
            b = trace32(ds, orig[cut:].copy(), d[cut:].copy(), cut_tn(cut, n))
            same(_concat(a, b), base)
        # n = 1, 63, 64, 65 and single rays: each ray's answer is the one it has in the whole batch
        for k in (1, 63, 64, 65):
            got = trace32(ds, orig[:k].copy(), d[:k].copy(), cut_tn(0, k))
            same(got, base.take(slice(0, k)), stats=False)
        for k in (0, 64, 164):
            got = trace32(ds, orig[k:k + 1].copy(), d[k:k + 1].copy(), cut_tn(k, k + 1))
            same(got, base.take(slice(k, k + 1)), stats=False)
    # picks: the sort, the form of the call, the batch around a position
    xy =np.array(sc.sample_xy(sc.W1, sc.H1), np.float32)
    o = pick_opts(sc.W1, sc.H1)
    base = pick32(ds, o, xy)
    assert base.stats.numPrimaryRays == n and (base.obj >= 0).any() and (base.obj < 0).any()
    for kw in ({"sort": True}, {"device": True}, {"device": True, "sort": True}):
        same(pick32(ds, o, xy, **kw), base)
    same(_concat(pick32(ds, o, xy[:65].copy()), pick32(ds, o, xy[65:].copy())), base)
    same(pick32(ds, o, xy[164:].copy()), base.take(slice(164, 165)), stats=False)


# ---- 5. the contract ---------------------------------------------------------------------------
def test_t_near_at_and_just_past_the_hit(gpu, oracle_mod):
    orig, d = t32.frame_rays(oracle_mod)
    ds = device_scene(15)
    free = trace32(ds, orig, d)
    sel = np.flatnonzero(free.obj >= 0)[::7]
    assert len(sel) >= 1000
    o, dd, t0 = orig[sel].copy(), d[sel].copy(), free.t[sel].copy()
    at = trace32(ds, o, dd, t0)                       # strict <: nothing is hit
    assert (at.obj == -1).all() and (at.face == -1).all() and sc.same_bits(at.t, t0) and not at.normals.any()
    past = trace32(ds, o, dd, np.nextafter(t0, INF32))    # one ulp further: the hit, as without a t_near
    same(past, free.take(sel), stats=False)
    neg = trace32(ds, o, dd, np.full(len(sel), -1.0, np.float32))
    assert (neg.obj == -1).all() and (neg.t == np.float32(-1.0)).all()
    assert neg.stats.numIntersectionHits == 0 and neg.stats.numIntersectionTests == len(sel) * 5
    anyneg = trace32(ds, o, dd, np.full(len(sel), -1.0, np.float32), any_hit=True, normals=False)
    assert (anyneg.obj == -1).all()


KINDS = ("component", "zero", "tnear")


def _spoil(orig, d, tn, i, kind):
    if kind == "component":
        if i % 2:
            orig[i, 1] = np.nan
        else:
            d[i, 2] = -np.inf
    elif kind == "zero":
        d[i] = (0.0, -0.0, 0.0)
    else:
        tn[i] = np.nan


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_degenerate_rays(gpu, oracle_mod, shift):
    """All three kinds at lanes 0, 63 and 64 (slot 64 is lane 0 of the second
    wave), the kinds rotated over the lanes by `shift`."""
    orig, d = (np.array(a) for a in t32.small_rays(oracle_mod))
    n = len(orig)
    ds = device_scene(15)
    tn = np.full(n, 30.0, np.float32)
    clean = trace32(ds, orig, d, tn)
    lanes = (0, 63, 64)
    for k, i in enumerate(lanes):
        _spoil(orig, d, tn, i, KINDS[(k + shift) % 3])
    bad = np.zeros(n, bool)
    bad[list(lanes)] = True
    good = ~bad
    for kw in ({}, {"sort": True, "device": True}):
        got = trace32(ds, orig, d, tn, **kw)
        assert (got.obj[bad] == -1).all() and (got.face[bad] == -1).all() and not got.normals[bad].any()
        assert sc.same_bits(got.t[bad], tn[bad])        # t_near as given, NaN as NaN
        same(got.take(good), clean.take(good), stats=False)
        rest = trace32(ds, orig[good].copy(), d[good].copy(), tn[good].copy())
        same(got.take(good), rest, stats=False)
        assert got.stats == rest.stats and got.stats.numIntersectionTests == (n - 3) * 5
    anyhit = trace32(ds, orig, d, tn, any_hit=True, normals=False)
    assert (anyhit.obj[bad] == -1).all() and sc.same_bits(anyhit.t, tn)
    assert anyhit.stats.numIntersectionTests == (n - 3) * 5


def test_degenerate_picks_and_huge_rays(gpu, oracle_mod):
    ds = device_scene(15)
    xy = np.array(sc.sample_xy(sc.W1, sc.H1), np.float32)
    o = pick_opts(sc.W1, sc.H1)
    clean = pick32(ds, o, xy)
    xy[0] = (np.nan, 3.0)
    xy[63] = (2.0, np.inf)
    xy[64] = (-np.inf, np.nan)
    bad = np.zeros(len(xy), bool)
    bad[[0, 63, 64]] = True
    for kw in ({}, {"sort": True, "device": True}):
        got = pick32(ds, o, xy, **kw)
        assert got.stats.numPrimaryRays == len(xy) - 3
        assert (got.obj[bad] == -1).all() and (got.t[bad] == INF32).all() and not got.normals[bad].any()
        same(got.take(~bad), clean.take(~bad), stats=False)
    # fractional and out-of-image positions are legal
    out = pick32(ds, o, np.array([[-7.5, 3.25], [40.0, -2.0], [7.5, 100.0], [7.3, 5.6]], np.float32))
    assert out.stats.numPrimaryRays == 4
    # finite rays of any magnitude are answered (whatever the answer), their neighbours unchanged
    orig, d = (np.array(a) for a in t32.small_rays(oracle_mod))
    base = trace32(ds, orig, d)
    big = np.float32(3.0e38)
    orig[5] = (big, -big, big)
    d[70] = (big, big, -big)
    d[100] = (1e-38, -1e-38, 1e-38)
    orig[130] = (-big, 1e-38, 0.0)
    got = trace32(ds, orig, d)
    keep = np.ones(len(orig), bool)
    keep[[5, 70, 100, 130]] = False
    same(got.take(keep), base.take(keep), stats=False)


@pytest.mark.parametrize("scale", [0.25, 3.0])
def test_unnormalised_directions(gpu, oracle_mod, scale):
    """t is in units of |dir|: on planes, boxes and meshes scaling the
    direction scales t inversely. (Subset 14, without spheres: the
    reference's Sphere.intersect divides by 2 and multiplies by a where the
    quadratic formula divides by 2a (geom.nim:215-237), which the float32
    kernel keeps, so a sphere's t does not scale with a direction that is
    not a unit vector: the oracle gives 12.35, 0.2305 and 0.0508 along one
    direction at lengths 1, 0.25 and 3.)"""
    orig, d = t32.frame_rays(oracle_mod)
    ds = device_scene(14)
    unit = trace32(ds, orig, d)
    got = trace32(ds, orig, (d * np.float32(scale)).astype(np.float32))
    agree = (got.obj == unit.obj) & (got.face == unit.face)
    assert float(agree.mean()) >= CAP
    k = agree & (unit.obj >= 0)
    t1 = unit.t[k].astype(np.float64)
    err = np.abs(got.t[k].astype(np.float64) * scale - t1) / np.maximum(1.0, t1)
    print(f"scale {scale}: largest relative error of t * scale {err.max():.3g}")
    assert k.sum() >= 10000 and (unit.obj[k] == 0).any() and (unit.obj[k] == 1).any() and (unit.obj[k] == 2).any()
    assert err.max() <= T_BOUND
    n_err = np.abs(got.normals[k] - unit.normals[k]).max(axis=1)
    assert _quantile(n_err, CAP) <= N_BOUND


def test_after_edits(gpu, oracle_mod):
    orig, d = t32.small_rays(oracle_mod)
    xy = np.array(sc.sample_xy(sc.W1, sc.H1), np.float32)
    o = pick_opts(sc.W1, sc.H1)
    bits = ss.SPHERE | ss.MESH
    edited = ss.subset_scene(bits)
    ds = DeviceScene(edited)                # holds the description as it is now; `edited` changes below
    assert ds.trace32_subset() == bits

    def answers(s):
        return (s.trace32_subset(), trace32(s, orig, d), trace32(s, orig, d, sort=True, device=True),
                trace32(s, orig, d, any_hit=True, normals=False), pick32(s, o, xy))

    def check(want_bits):
        other = DeviceScene(edited)
        try:
            fresh = answers(other)
        finally:
            other.close()
        mine = answers(ds)
        assert mine[0] == fresh[0] == want_bits
        for a, b in zip(mine[1:], fresh[1:]):
            same(a, b)
        return mine[1]

    before = check(bits)
    edited.lights = list(edited.lights) + [PointLight(color=vec3(0.6, 0.8, 1.0), intensity=2000.0,
                                                      pos=point(-4.0, 9.0, -6.0))]
    ds.set_lights(edited.lights)
    same(check(bits), before)               # lights do not change what a ray hits
    # the first sphere takes a general transform: another specialisation
    moved = ss.subset_scene(bits | ss.XF_GENERAL)
    edited.objects[0].geometry = moved.objects[0].geometry
    ds.set_objects(edited.objects)
    turned = check(bits | ss.XF_GENERAL)
    assert turned.raw() != before.raw()
    mesh = next(ob.geometry for ob in edited.objects if isinstance(ob.geometry, TriangleMesh))
    v = mesh.vertices.copy()
    v[:, 1] = v[:, 1] * (1.0 + 0.25 * np.sin(2.0 * v[:, 0]))   # the torus, unevenly taller
    mesh.vertices = np.ascontiguousarray(v)
    ds.set_mesh_vertices(0, mesh.vertices)
    deformed = check(bits | ss.XF_GENERAL)
    assert deformed.raw() != turned.raw()
    ds.close()


def _last_stats(ds):
    st = abi.rt_stats()
    assert lib().rt_scene_last_stats(ds.h, C.byref(st)) == abi.RT_OK
    return st.as_dict()


def test_render_state_untouched(gpu, oracle_mod):
    import torch
    ds = DeviceScene(ss.subset_scene(4))       # the torus on the ground: a two-class float32 launch
    opts = Options(width=64, height=48, antialias=Antialias(akGrid, 8), bias=1e-4, precision=Precision.fp32)
    fb = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    before = (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds))
    assert before[3]["num_primary_rays"] == st.numPrimaryRays == 64 * 48 * 64
    orig, d = t32.small_rays(oracle_mod)
    got = trace32(ds, orig, d, sort=True)
    assert (got.obj >= 0).any() and got.stats.numIntersectionTests == 165 * 2
    trace32(ds, orig, d, device=True, any_hit=True, normals=False)
    pick32(ds, pick_opts(64, 48), np.array(sc.sample_xy(64, 48), np.float32), device=True, sort=True)
    assert (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds)) == before
    fb2 = torch.zeros_like(fb)
    assert ds.render_device(opts, fb2) == st
    assert torch.equal(fb, fb2)
    ds.close()


def test_errors(gpu, oracle_mod):
    import torch
    ds = device_scene(15)
    orig, d = (np.array(a[:12]) for a in t32.small_rays(oracle_mod))
    tn = np.full(12, 50.0, np.float32)
    xy = np.array(sc.sample_xy(4, 3), np.float32)
    hits = (abi.rt_hit32 * 12)()
    nrm = np.zeros((12, 3), np.float32)
    st = abi.rt_stats()
    o32 = pick_opts(4, 3).to_c()
    L = lib()

    def call(n=12, flags=0, a=orig, b=d, t=tn, out=hits, normals=nrm):
        return L.rt_trace_rays_f32(ds.h, n, _fp(a) if a is not None else None, _fp(b) if b is not None else None,
                                   _fp(t) if t is not None else None, flags, out,
                                   _fp(normals) if normals is not None else None, C.byref(st))

    def pick(n=12, flags=0, opts=o32, p=xy, out=hits, normals=nrm):
        return L.rt_pick_pixels_f32(ds.h, C.byref(opts) if opts is not None else None, n,
                                    _fp(p) if p is not None else None, flags, out,
                                    _fp(normals) if normals is not None else None, C.byref(st))

    assert call() == abi.RT_OK and st.num_intersection_tests == 12 * 5 and st.num_primary_rays == 0
    assert all(h.reserved == 0 for h in hits)
    assert call(t=None, normals=None) == abi.RT_OK
    assert call(n=-1) == abi.RT_E_INVALID
    assert call(flags=0x4) == abi.RT_E_INVALID and call(flags=0x80000000) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID and b"normals" in L.rt_last_error()
    assert call(flags=abi.RT_QUERY_ANY_HIT | abi.RT_QUERY_SORT, normals=None) == abi.RT_OK
    assert call(a=None) == abi.RT_E_INVALID and call(b=None) == abi.RT_E_INVALID
    assert call(out=None) == abi.RT_E_INVALID
    assert call(n=2 ** 31) == abi.RT_E_UNSUPPORTED
    st.num_intersection_tests = 7
    assert call(n=0, a=None, b=None, t=None, out=None, normals=None) == abi.RT_OK and st.num_intersection_tests == 0
    assert pick() == abi.RT_OK and st.num_primary_rays == 12 and st.num_intersection_tests == 12 * 5
    assert pick(n=-1) == abi.RT_E_INVALID and pick(flags=0x10) == abi.RT_E_INVALID
    assert pick(flags=abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID
    assert pick(flags=abi.RT_QUERY_ANY_HIT, normals=None) == abi.RT_OK
    assert pick(opts=None) == abi.RT_E_INVALID and pick(p=None) == abi.RT_E_INVALID and pick(out=None) == abi.RT_E_INVALID
    assert pick(n=2 ** 31) == abi.RT_E_UNSUPPORTED
    o64 = pick_opts(4, 3, Precision.fp64).to_c()
    assert pick(opts=o64) == abi.RT_E_INVALID and b"rt_pick_pixels" in L.rt_last_error()
    zero = pick_opts(4, 3).to_c()
    zero.width = 0
    assert pick(opts=zero) == abi.RT_E_INVALID
    st.num_primary_rays = 7
    assert pick(n=0, p=None, out=None, normals=None) == abi.RT_OK and st.num_primary_rays == 0
    # only width, height and precision of opts are read
    odd = pick_opts(4, 3).to_c()
    odd.aa_kind, odd.grid_size, odd.bias, odd.max_ray_depth, odd.flags = 3, 0, -1.0, 99, 0xffff
    assert pick() == abi.RT_OK
    first = bytes(hits)
    assert pick(opts=odd) == abi.RT_OK and bytes(hits) == first
    # the float64 pick still refuses RT_FP32
    with pytest.raises(RtmiError) as e:
        ds.pick(pick_opts(4, 3), xy.astype(np.float64))
    assert e.value.code == abi.RT_E_UNSUPPORTED
    # the device forms check the same things before they touch the device
    dev, dpick = L.rt_trace_rays_f32_device, L.rt_pick_pixels_f32_device
    assert dev(ds.h, 12, None, None, None, 0, None, None, None, None) == abi.RT_E_INVALID
    assert dev(ds.h, 0, None, None, None, 0, None, None, None, C.byref(st)) == abi.RT_OK
    assert dpick(ds.h, C.byref(o32), 12, None, 0, None, None, None, None) == abi.RT_E_INVALID
    assert dpick(ds.h, C.byref(o64), 0, None, 0, None, None, None, None) == abi.RT_E_INVALID
    # device hits must be 16-byte aligned
    do, dd = _dev(orig), _dev(d)
    buf = torch.zeros(12 * 4 + 4, dtype=torch.float32, device="cuda")
    assert dev(ds.h, 12, C.c_void_p(do.data_ptr()), C.c_void_p(dd.data_ptr()), None, 0, C.c_void_p(buf.data_ptr() + 4),
               None, None, None) == abi.RT_E_INVALID and b"aligned" in L.rt_last_error()
    assert dev(ds.h, 12, C.c_void_p(do.data_ptr()), C.c_void_p(dd.data_ptr()), None, 0, C.c_void_p(buf.data_ptr()),
               None, None, C.byref(st)) == abi.RT_OK
    # the Python methods raise with the code, and refuse other dtypes and shapes
    with pytest.raises(RtmiError) as e:
        ds.pick_f32(pick_opts(4, 3, Precision.fp64), xy)
    assert e.value.code == abi.RT_E_INVALID
    with pytest.raises(RtmiError) as e:
        ds.trace_rays_f32(orig, d, any_hit=True, normals=True)
    assert e.value.code == abi.RT_E_INVALID
    with pytest.raises(ValueError):
        ds.trace_rays_f32(orig, d[:6])
    with pytest.raises(ValueError):
        ds.trace_rays_f32(orig.astype(np.float64), d.astype(np.float64))
    with pytest.raises(ValueError):
        ds.trace_rays_f32(orig, d, tn[:5])
    with pytest.raises(ValueError):
        ds.pick_f32(pick_opts(4, 3), xy.astype(np.float64))
