"""The float32 ray, pick and radiance queries (DeviceScene.trace_rays_f32 /
pick_f32 / shade_rays_f32) against the multiprecision truth (truth.py), from
the recorded fixtures tests/golden/truth32_*.npz alone: no oracle, no mpmath.

test_gpu_trace32.py and test_gpu_shade32.py send one camera's primary rays
(coherent, one origin, outside every object) and compare with the float64
query under an agreement cap. Here the rays are incoherent (truth32_cases:
origins inside boxes, spheres and mesh boxes and below the ground, zero
direction components of either sign, finite t_near), every value is exactly
float32, the expected answer is the written specification's, and there is no
cap: on every ray the truth decides with room for float32 (its float32 query
margins reach EPS32; test_truth32_cpu.py proves on a numpy float32 brute
force that the room is there) the object and the face are equal, t and the
normal within test_gpu_trace32.py's bounds, a colour within 1e-4. Only
decided rays are sent, as in test_gpu_truth.py.

RTMI_PARITY_LOG=<file> appends the measured errors
(profiles/trace32/truth_fp32.jsonl)."""
import functools
import json
import os

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, akNone
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH
from rtmi.renderer import DeviceScene

import truth
import truth32_cases as c

pytestmark = pytest.mark.gpu

INF32 = np.float32(np.inf)
BUILDERS = {RT_BVH_SAH: "sah", RT_BVH_PLOC: "ploc"}
RAYS = list(c.RAY_SCENES) + list(c.CORPUS)
RAY_CASES = [(n, b) for n in RAYS for b in ((RT_BVH_SAH, RT_BVH_PLOC) if c.has_mesh(c.scene_of(n)) else (RT_BVH_SAH,))]
_ids = [f"{n}-{BUILDERS[b]}" for n, b in RAY_CASES]


@functools.lru_cache(maxsize=None)
def device_scene(name, builder=RT_BVH_SAH):
    return DeviceScene(c.scene_of(name), bvh_builder=builder)


@functools.lru_cache(maxsize=None)
def decided(name):
    """The fixture restricted to the rays whose hit is decided: only those are sent."""
    b = c.load(name)
    ok = c.decided(b, c.threshold(name))[0]
    out = {k: np.ascontiguousarray(v[ok]) for k, v in b.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _np(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def trace32(ds, orig, d, tn, device=False, normals=True, **kw):
    """One call's answers as compare takes them, and its Stats."""
    if device:
        orig, d, tn = _dev(orig), _dev(d), _dev(tn)
    res = list(ds.trace_rays_f32(orig, d, tn, normals=normals, stats=True, **kw))
    got = {"t": _np(res[0]), "obj": _np(res[1]), "face": _np(res[2]), "normal": _np(res[3]) if normals else None}
    return got, res[-1]


def raw(got, idx=slice(None)):
    return b"".join(got[k][idx].tobytes() for k in ("t", "obj", "face", "normal") if got[k] is not None)


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("RTMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def check(what, b, got, st, thr, nobj, primary=False):
    e_t, e_n = c.compare(b, got, thr)
    n = len(b["obj"])
    assert st.numIntersectionTests == n * nobj, (what, st)
    assert st.numIntersectionHits == int(b["hits"].sum()), (what, st, int(b["hits"].sum()))
    assert st.numPrimaryRays == (n if primary else 0)
    assert st.numShadowRays == 0 and st.numReflectionRays == 0
    _log({"what": what, "rays": n, "hits": int((b["obj"] >= 0).sum()), "face_hits": int((b["face"] >= 0).sum()),
          "normals_judged": int(((b["obj"] >= 0) & (b["normal32"] >= thr)).sum()), "t_rel_max": e_t, "normal_max": e_n})


# ---- rt_trace_rays_f32 -------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", RAY_CASES, ids=_ids)
def test_trace_rays(gpu, name, builder):
    b = decided(name)
    assert len(b["obj"]) >= c.HIT_SHARE * c.N_RAYS
    ds = device_scene(name, builder)
    got, st = trace32(ds, b["orig"], b["dir"], b["tnear"])
    check(f"{name} {BUILDERS[builder]} trace_rays_f32", b, got, st, c.threshold(name), len(c.scene_of(name).objects))


@pytest.mark.parametrize("name,builder", RAY_CASES, ids=_ids)
def test_any_hit(gpu, name, builder):
    b = decided(name)
    got, st = trace32(device_scene(name, builder), b["orig"], b["dir"], b["tnear"], normals=False, any_hit=True)
    bad = np.flatnonzero((got["obj"] >= 0) != (b["obj"] >= 0))
    assert bad.size == 0, [(int(i), int(got["obj"][i]), int(b["obj"][i])) for i in bad[:8]]
    assert got["t"].tobytes() == b["tnear"].tobytes() and (got["face"] == -1).all()
    assert st.numIntersectionTests == len(b["obj"]) * len(c.scene_of(name).objects)


# ---- independence on incoherent rays -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(c.RAY_SCENES) + ["soup_1025", "torus_2304"])
def test_independence(gpu, name):
    """Every ray of the WHOLE batch (undecided rays included: the rule does
    not depend on the answer being decided), bit for bit."""
    f = c.load(name)
    orig, d, tn = f["orig"], f["dir"], f["tnear"]
    n = len(orig)
    assert n == c.N_RAYS
    ds = device_scene(name)
    base, st = trace32(ds, orig, d, tn)
    for kw in ({"sort": True}, {"device": True}, {"device": True, "sort": True}):
        got, st2 = trace32(ds, orig, d, tn, **kw)
        assert raw(got) == raw(base), (kw, np.flatnonzero((got["obj"] != base["obj"]) | (got["t"] != base["t"]))[:8])
        assert st2 == st, (kw, st2, st)
    perm = np.random.default_rng(c.SEEDS.get(name, 1) + 7).permutation(n)
    for sort in (False, True):
        got, _ = trace32(ds, orig[perm].copy(), d[perm].copy(), tn[perm].copy(), sort=sort)
        back = {k: np.empty_like(v) for k, v in got.items()}
        for k in back:
            back[k][perm] = got[k]
        assert raw(back) == raw(base), np.flatnonzero((back["obj"] != base["obj"]) | (back["t"] != base["t"]))[:8]
    for sort in (False, True):                      # 511 rays: the eighth wave has a tail
        got, _ = trace32(ds, orig[:511].copy(), d[:511].copy(), tn[:511].copy(), sort=sort)
        assert raw(got) == raw(base, slice(0, 511))
    anybase, ast = trace32(ds, orig, d, tn, normals=False, any_hit=True)
    for kw in ({"sort": True}, {"device": True, "sort": True}):
        got, st2 = trace32(ds, orig, d, tn, normals=False, any_hit=True, **kw)
        assert raw(got) == raw(anybase) and st2 == ast, kw
    got, _ = trace32(ds, orig[:511].copy(), d[:511].copy(), tn[:511].copy(), normals=False, any_hit=True)
    assert raw(got) == raw(anybase, slice(0, 511))


# ---- rt_pick_pixels_f32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", c.PICK_SCENES)
def test_pick_pixels(gpu, name):
    b = decided(f"pick_{name}")
    n = len(b["obj"])
    assert n >= c.HIT_SHARE * 120
    xy = b["xy"]
    assert xy.dtype == np.float32
    inside = (xy >= 0).all(1) & (xy[:, 0] < c.PICK_W) & (xy[:, 1] < c.PICK_H)
    assert (~inside).sum() >= 10 and (xy != np.floor(xy)).any(1).sum() >= 40
    opts = Options(width=c.PICK_W, height=c.PICK_H, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp32)
    ds = device_scene(name)
    res = list(ds.pick_f32(opts, xy, normals=True, stats=True))
    got = {"t": _np(res[0]), "obj": _np(res[1]), "face": _np(res[2]), "normal": _np(res[3])}
    check(f"{name} pick_f32", b, got, res[-1], c.threshold(f"pick_{name}"), len(c.scene_of(name).objects), primary=True)
    res2 = list(ds.pick_f32(opts, _dev(xy), normals=True, sort=True, stats=True))
    got2 = {"t": _np(res2[0]), "obj": _np(res2[1]), "face": _np(res2[2]), "normal": _np(res2[3])}
    assert raw(got2) == raw(got) and res2[-1] == res[-1]


# ---- rt_shade_rays_f32 -------------------------------------------------------------------------------
def _opts32():
    return Options(width=1, height=1, antialias=Antialias(akNone, 1), bias=c.BIAS, maxRayDepth=c.DEPTH,
                   precision=Precision.fp32)


@pytest.mark.parametrize("name", list(c.SHADE_SCENES))
def test_shade_rays(gpu, name):
    f = c.load(f"shade_{name}")
    ok = f["normal32"] >= truth.EPS32
    assert ok.mean() >= c.SHADE_SHARE
    n = int(ok.sum()) // 4 * 4                  # whole groups of 4
    sel = np.flatnonzero(ok)[:n]
    orig, d, want = np.ascontiguousarray(f["orig"][sel]), np.ascontiguousarray(f["dir"][sel]), f["rgb"][sel]
    scene = c.scene_of(name)
    box = (f["obj"][sel] >= 0) & (c.kinds(scene)[np.maximum(f["obj"][sel], 0)] == 2)
    assert box.sum() >= 10                      # decided rays whose primary hit is a box are present
    ds = device_scene(name)
    rgb, st = ds.shade_rays_f32(_opts32(), orig, d, stats=True)
    assert rgb.dtype == np.float32 and rgb.shape == (n, 3)
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1)
    _log({"what": f"{name} shade_rays_f32", "rays": n, "box_hits": int(box.sum()), "rgb_max": float(err.max()),
          "rgb_max_box": float(err[box].max())})
    assert (err <= c.RGB_BOUND).all(), ([(int(sel[i]), float(err[i])) for i in np.flatnonzero(err > c.RGB_BOUND)[:8]])
    assert st.numPrimaryRays == n
    # the sort, bit for bit
    rgb_s, st_s = ds.shade_rays_f32(_opts32(), orig, d, sort=True, stats=True)
    assert rgb_s.tobytes() == rgb.tobytes() and st_s == st
    # groups of 4: the float32 sum in index order times float32(1 / 4)
    grp, st_g = ds.shade_rays_f32(_opts32(), orig, d, group=4, stats=True)
    acc = np.zeros((n // 4, 3), np.float32)
    for j in range(4):
        acc = acc + rgb.reshape(-1, 4, 3)[:, j]
    assert grp.shape == (n // 4, 3) and grp.tobytes() == (acc * np.float32(0.25)).tobytes()
    assert st_g == st
    mean = want.reshape(-1, 4, 3).mean(axis=1)
    assert np.abs(grp.astype(np.float64) - mean).max() <= c.RGB_BOUND
