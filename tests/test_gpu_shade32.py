"""Float32 radiance queries (DeviceScene.shade_rays_f32, rt_shade_rays_f32*)
on the device: the float32 render's colour along caller-supplied float32 rays.

* all 64 specialisations of k_shade_rays_f32 against the oracle's frames,
  under the criteria of test_gpu_subsets._compare32; the
  float64 query on the same float32 ray values is the control that proves the
  rounded inputs alone stay inside them;
* the independence rule, bit for bit: a ray's colour and Stats do not depend
  on the batch around it, the sort, the binning flag or the form of the call;
* group sums, degenerate rays, unnormalised directions against the
  multiprecision truth, the recursion limit, scene edits, the render state
  and the error codes.

Every test uses bias 1e-4. RTMI_PARITY_LOG=<file> appends the measured
distances of the first test (profiles/shade32/parity_fp32.jsonl)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import shade_cases as sc
import subset_scenes as ss
import truth
from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi import abi
from rtmi._lib import RtmiError, lib
from rtmi.glm import point, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import PointLight, Stats, TriangleMesh

pytestmark = pytest.mark.gpu

BIAS = 1e-4
M, GROUP = 4, 16
_fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731


def opts32(depth=5, flags=0, bias=BIAS):
    return Options(width=1, height=1, antialias=Antialias(akNone, 1), bias=bias, maxRayDepth=depth,
                   precision=Precision.fp32, flags=flags)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


def shade32(ds, orig, d, group=1, sort=False, device=False, o=None):
    """(rgb float32 numpy, Stats) of one call, host or device form."""
    o = o or opts32()
    if not device:
        return ds.shade_rays_f32(o, orig, d, group=group, sort=sort, stats=True)
    import torch
    rgb, st = ds.shade_rays_f32(o, torch.from_numpy(np.array(orig)).cuda(), torch.from_numpy(np.array(d)).cuda(),
                                group=group, sort=sort, stats=True)
    assert rgb.is_cuda and rgb.dtype == torch.float32
    return rgb.cpu().numpy(), st


def same(got, want):
    assert got[0].dtype == np.float32 and sc.same_bits(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert got[1] == want[1], (got[1], want[1])


@functools.lru_cache(maxsize=None)
def frame_rays(oracle_mod):
    """The float64 castPrimaryRay rays of the 96 x 64 akGrid m = 4 frame every
    subset scene shares (one camera), rounded to float32."""
    scene = ss.subset_scene(0)
    o, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, ss.W, ss.H, M)
    o, d = f32(o), f32(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def small_rays(oracle_mod):
    """The 165 akNone rays of W1 x H1 (two full waves and a 37-lane tail)."""
    scene = ss.subset_scene(0)
    o, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, sc.W1, sc.H1)
    o, d = f32(o), f32(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def device_scene(bits):
    return DeviceScene(ss.subset_scene(bits))


# ---- 1. all 64 specialisations -------------------------------------------------------------
def _judge(what, got, st, n, ref, rst, mask):
    err = ss.pixel_error(got.reshape(ss.H, ss.W, 3), ref)
    row = {"what": what, "pixels": int(err.size), "beyond_2e-3": int(np.count_nonzero(err > 2e-3)),
           "beyond_1e-4": int(np.count_nonzero(err > 1e-4)), "mean": float(err.mean()),
           "smooth_share": float(mask.mean()), "smooth_max": float(err[mask].max())}
    print(json.dumps(row))
    path = os.environ.get("RTMI_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")
    assert st.numPrimaryRays == n == rst.numPrimaryRays, (what, st, rst)
    assert st.numIntersectionTests == pytest.approx(rst.numIntersectionTests, rel=1e-2), (what, st, rst)
    assert st.numShadowRays == pytest.approx(rst.numShadowRays, rel=1e-2), (what, st, rst)
    assert st.numReflectionRays == pytest.approx(rst.numReflectionRays, rel=1e-2), (what, st, rst)
    assert row["smooth_share"] >= 0.65, row
    assert float((err <= 2e-3).mean()) >= 0.995, row
    assert row["mean"] <= 2e-4, row
    assert row["smooth_max"] <= 1e-4, (row, [tuple(p) for p in np.argwhere(mask & (err > 1e-4))[:8]])


@pytest.mark.parametrize("bits", range(64))
def test_every_specialisation_against_the_oracle(gpu, oracle_mod, bits):
    orig, d = frame_rays(oracle_mod)
    n = len(orig)
    assert n == ss.W * ss.H * GROUP == 98304
    ds = DeviceScene(ss.subset_scene(bits))
    assert ds.shade32_subset() == bits
    ref, rst, _, mask = ss.oracle_frames(oracle_mod, bits, akGrid, M)
    name = f"subset {bits} {ss.subset_name(bits)}"
    # the control: the float64 query on the same float32 values
    o64 = Options(width=1, height=1, antialias=Antialias(akNone, 1), bias=BIAS, maxRayDepth=5, precision=Precision.fp64)
    c_rgb, c_st = ds.shade_rays(o64, orig.astype(np.float64), d.astype(np.float64), group=GROUP, f32=True, stats=True)
    _judge(name + " control fp64 query on float32 rays", c_rgb, c_st, n, ref, rst, mask)
    rgb, st = shade32(ds, orig, d, group=GROUP)
    assert rgb.shape == (ss.W * ss.H, 3)
    _judge(name + " shade_rays_f32", rgb, st, n, ref, rst, mask)
    ds.close()


# ---- 2. independence, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("bits", [63, 7])
def test_independence(gpu, oracle_mod, bits):
    orig, d = small_rays(oracle_mod)
    n = len(orig)
    assert n == 165
    ds = device_scene(bits)
    base = shade32(ds, orig, d)
    assert base[1].numPrimaryRays == n and base[0].any()
    groups = {g: shade32(ds, orig, d, group=g) for g in (3, 5, 15)}
    nobin = opts32(flags=abi.RT_FLAG_NO_BINNING)
    for g in (1, 3, 5, 15):
        want = base if g == 1 else groups[g]
        same(shade32(ds, orig, d, group=g, sort=True), want)
        same(shade32(ds, orig, d, group=g, device=True), want)
        same(shade32(ds, orig, d, group=g, device=True, sort=True), want)
        same(shade32(ds, orig, d, group=g, o=nobin), want)
        same(shade32(ds, orig, d, group=g, sort=True, o=nobin), want)
    # a seeded permutation of the batch, the colours un-permuted
    perm = np.random.default_rng(32 + bits).permutation(n)
    for sort in (False, True):
        rgb, st = shade32(ds, orig[perm].copy(), d[perm].copy(), sort=sort)
        back = np.empty_like(rgb)
        back[perm] = rgb
        same((back, st), base)
    # one call and two calls
    for cut in (64, 65, 100):
        a, b = shade32(ds, orig[:cut].copy(), d[:cut].copy()), shade32(ds, orig[cut:].copy(), d[cut:].copy())
        total = Stats()
        total += a[1]
        total += b[1]
        same((np.concatenate([a[0], b[0]]), total), base)
    # n = 1, 63, 64, 65: each ray's colour is the one it has in the whole batch
    for k in (1, 63, 64, 65):
        rgb, st = shade32(ds, orig[:k].copy(), d[:k].copy())
        assert sc.same_bits(rgb, base[0][:k]) and st.numPrimaryRays == k
    singles = [shade32(ds, orig[k:k + 1].copy(), d[k:k + 1].copy()) for k in (0, 64, 164)]
    assert sc.same_bits(np.concatenate([s[0] for s in singles]), base[0][[0, 64, 164]])


# ---- 3. groups -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.GRID_M)
def test_groups(gpu, oracle_mod, m):
    scene = ss.subset_scene(63)
    o, d = sc.camera_rays(oracle_mod, scene.cameraToWorld, scene.fov, sc.W2, sc.H2, m)
    o, d = f32(o), f32(d)
    g = m * m
    assert g in (4, 9, 64)
    ds = device_scene(63)
    per_ray, st1 = shade32(ds, o, d)
    acc = np.zeros((len(o) // g, 3), np.float32)
    c = per_ray.reshape(-1, g, 3)
    for j in range(g):
        acc = acc + c[:, j]
    want = acc * np.float32(1.0 / g)
    assert want.dtype == np.float32
    for sort in (False, True):
        rgb, st = shade32(ds, o, d, group=g, sort=sort)
        assert sc.same_bits(rgb, want), np.argwhere(rgb != want)[:5]
        assert st == st1


# ---- 4. degenerate rays ----------------------------------------------------------------------
BAD = {3: ("orig", (np.nan, 1.0, 2.0)), 70: ("dir", (0.0, -np.inf, 1.0)), 130: ("dir", (0.0, 0.0, 0.0)),
       131: ("dir", (-0.0, 0.0, -0.0)), 164: ("orig", (0.0, np.inf, 0.0)),
       **{k: ("dir", (0.0, 0.0, 0.0)) for k in range(45, 60)}}  # whole groups of 3, 5 and 15


@pytest.mark.parametrize("group", [1, 3, 5, 15])
def test_degenerate_rays(gpu, oracle_mod, group):
    orig, d = (np.array(a) for a in small_rays(oracle_mod))
    ds = device_scene(63)
    clean, _ = shade32(ds, orig, d)
    for k, (which, v) in BAD.items():
        (orig if which == "orig" else d)[k] = v
    good = np.ones(len(orig), bool)
    good[list(BAD)] = False
    rgb, st = shade32(ds, orig, d, group=group)
    # the Stats: those of the batch with the degenerate rays removed
    _, st_good = shade32(ds, orig[good].copy(), d[good].copy())
    assert st == st_good and st.numPrimaryRays == good.sum() == len(orig) - len(BAD)
    colours = np.where(good[:, None], clean, np.float32(0.0))
    if group == 1:
        assert sc.same_bits(rgb, colours)
        assert not rgb[~good].any() and not np.signbit(rgb[~good]).any()
    else:
        acc = np.zeros((len(orig) // group, 3), np.float32)
        for j in range(group):
            acc = acc + colours.reshape(-1, group, 3)[:, j]
        assert sc.same_bits(rgb, acc * np.float32(1.0 / group))
        whole = ~good.reshape(-1, group).any(1)     # groups of degenerate rays alone
        assert whole.any() and not rgb[whole].any() and not np.signbit(rgb[whole]).any()
    same(shade32(ds, orig, d, group=group, sort=True, device=True), (rgb, st))


# ---- 5. unnormalised directions: the multiprecision truth ------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("bits", sc.TRUTH_BITS)
def test_unnormalised_directions(gpu, bits, sort):
    f = truth.load(f"shade_{bits}")
    ok = f["normal32"] >= truth.EPS32          # the float32 query margin: box hits are judged too
    assert ok.mean() >= 0.5 and (ok >= (f["margin32"] >= truth.EPS32)).all()
    assert (f["obj"][ok] >= 0).sum() >= 60
    box = [type(o.geometry).__name__ for o in ss.subset_scene(bits).objects].index("Box")
    assert (f["obj"][ok] == box).sum() >= 5
    orig, d = f32(f["orig"]), f32(f["dir"])
    assert (np.abs(np.linalg.norm(d, axis=1) - 1.0) > 0.5).sum() >= len(d) // 2
    rgb, st = shade32(device_scene(bits), orig, d, sort=sort)
    err = np.abs(rgb.astype(np.float64) - f["rgb"]).max(axis=1)
    print(f"subset {bits}: {ok.mean():.3f} of the rays decided, largest error {err[ok].max():.3g}")
    assert (err[ok] <= 1e-4).all(), (np.argwhere(ok & (err > 1e-4))[:5], err[ok].max())
    assert st.numPrimaryRays == 96


# ---- 6. depth ----------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 1, 7])
def test_depth(gpu, oracle_mod, depth):
    orig, d = small_rays(oracle_mod)
    ds = device_scene(35)
    _, st = shade32(ds, orig, d, o=opts32(depth))
    _, st64 = ds.shade_rays(sc.options(1, 1, 0, BIAS, depth), orig.astype(np.float64), d.astype(np.float64), stats=True)
    assert st.numReflectionRays == pytest.approx(st64.numReflectionRays, rel=1e-2), (st, st64)
    assert (st.numReflectionRays == 0) == (depth == 0)
    assert (st64.numReflectionRays == 0) == (depth == 0)


def test_depth_limits(gpu, oracle_mod):
    orig, d = small_rays(oracle_mod)
    with pytest.raises(RtmiError) as e:
        device_scene(35).shade_rays_f32(opts32(8), orig, d)
    assert e.value.code == abi.RT_E_UNSUPPORTED
    # without reflective materials any depth is accepted, and changes nothing
    same(shade32(device_scene(7), orig, d, o=opts32(100)), shade32(device_scene(7), orig, d))


# ---- 7. after edits ----------------------------------------------------------------------------
def test_after_edits(gpu, oracle_mod):
    orig, d = small_rays(oracle_mod)
    bits = ss.SPHERE | ss.MESH
    edited = ss.subset_scene(bits)
    ds = DeviceScene(edited)                # holds the description as it is now; `edited` changes below
    assert ds.shade32_subset() == bits

    def fresh():
        other = DeviceScene(edited)
        try:
            return other.shade32_subset(), shade32(other, orig, d), shade32(other, orig, d, group=5, sort=True)
        finally:
            other.close()

    def check(want_bits):
        sub, one, five = fresh()
        assert sub == want_bits == ds.shade32_subset()
        same(shade32(ds, orig, d), one)
        same(shade32(ds, orig, d, group=5, sort=True), five)
        return one

    before = check(bits)
    edited.lights = list(edited.lights) + [PointLight(color=vec3(0.6, 0.8, 1.0), intensity=2000.0,
                                                      pos=point(-4.0, 9.0, -6.0))]
    ds.set_lights(edited.lights)
    lit = check(bits | ss.POINT)
    assert not sc.same_bits(lit[0], before[0]) and lit[1].numShadowRays > before[1].numShadowRays
    edited.objects[0].material.reflection = 0.6
    edited.objects[-1].material.reflection = 0.25
    ds.set_objects(edited.objects)
    mirrored = check(bits | ss.POINT | ss.REFLECT)
    assert mirrored[1].numReflectionRays > 0 == lit[1].numReflectionRays
    with pytest.raises(RtmiError) as e:     # and the depth limit now applies
        ds.shade_rays_f32(opts32(8), orig, d)
    assert e.value.code == abi.RT_E_UNSUPPORTED
    mesh = next(o.geometry for o in edited.objects if isinstance(o.geometry, TriangleMesh))
    v = mesh.vertices.copy()
    v[:, 1] = v[:, 1] * (1.0 + 0.25 * np.sin(2.0 * v[:, 0]))   # the torus, unevenly taller
    mesh.vertices = np.ascontiguousarray(v)
    ds.set_mesh_vertices(0, mesh.vertices)
    deformed = check(bits | ss.POINT | ss.REFLECT)
    assert not sc.same_bits(deformed[0], mirrored[0])
    ds.close()


# ---- 8. the render state is left alone ---------------------------------------------------------
def _last_stats(ds):
    st = abi.rt_stats()
    assert lib().rt_scene_last_stats(ds.h, C.byref(st)) == abi.RT_OK
    return st.as_dict()


def test_render_state_untouched(gpu, oracle_mod):
    import torch
    ds = DeviceScene(ss.subset_scene(4))       # the torus on the ground: a two-class float32 launch
    opts = Options(width=64, height=48, antialias=Antialias(akGrid, 8), bias=BIAS, precision=Precision.fp32)
    fb = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    before = (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds))
    assert before[3]["num_primary_rays"] == st.numPrimaryRays == 64 * 48 * 64
    orig, d = small_rays(oracle_mod)
    rgb, qst = shade32(ds, orig, d, group=5, sort=True)
    assert rgb.any() and qst.numPrimaryRays == 165
    shade32(ds, orig, d, device=True)
    assert (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds)) == before
    fb2 = torch.zeros_like(fb)
    assert ds.render_device(opts, fb2) == st
    assert torch.equal(fb, fb2)
    ds.close()


# ---- 9. errors ---------------------------------------------------------------------------------
def test_errors(gpu, oracle_mod):
    ds = device_scene(63)
    orig, d = (np.array(a[:12]) for a in small_rays(oracle_mod))
    o32 = opts32().to_c()
    rgb, st = np.zeros((12, 3), np.float32), abi.rt_stats()

    def call(n=12, group=1, flags=0, opts=o32, a=orig, b=d, out=rgb):
        return lib().rt_shade_rays_f32(ds.h, C.byref(opts) if opts is not None else None, n,
                                       _fp(a) if a is not None else None, _fp(b) if b is not None else None, group,
                                       flags, _fp(out) if out is not None else None, C.byref(st))

    assert call() == abi.RT_OK and st.num_primary_rays == 12
    assert call(group=5) == abi.RT_E_INVALID and b"group" in lib().rt_last_error()
    assert call(group=0) == abi.RT_E_INVALID
    assert call(group=-3) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_SORT | abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID
    assert call(flags=0x10) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_SORT) == abi.RT_OK
    o64 = opts32().to_c()
    o64.precision = abi.RT_FP64
    assert call(opts=o64) == abi.RT_E_INVALID and b"rt_shade_rays" in lib().rt_last_error()
    assert call(opts=None) == abi.RT_E_INVALID
    assert call(out=None) == abi.RT_E_INVALID
    assert call(a=None) == abi.RT_E_INVALID and call(b=None) == abi.RT_E_INVALID
    assert call(n=-1) == abi.RT_E_INVALID
    assert call(n=2 ** 31) == abi.RT_E_UNSUPPORTED
    # n == 0: RT_OK, nothing launched, zero Stats; a bad group is still refused
    st.num_primary_rays = 7
    assert call(n=0, a=None, b=None, out=None) == abi.RT_OK and st.num_primary_rays == 0
    assert call(n=0, group=0) == abi.RT_E_INVALID
    # the device form checks the same things before it touches the device
    dev = lib().rt_shade_rays_f32_device
    assert dev(ds.h, C.byref(o32), 12, None, None, 1, 0, None, None, None) == abi.RT_E_INVALID
    assert dev(ds.h, C.byref(o32), 0, None, None, 0, 0, None, None, None) == abi.RT_E_INVALID
    assert dev(ds.h, C.byref(o32), 0, None, None, 1, 0, None, None, C.byref(st)) == abi.RT_OK
    # the Python method raises with the code
    with pytest.raises(RtmiError) as e:
        ds.shade_rays_f32(opts32(), orig, d, group=5)
    assert e.value.code == abi.RT_E_INVALID
    with pytest.raises(ValueError):
        ds.shade_rays_f32(opts32(), orig, d[:6])
    with pytest.raises(ValueError):
        ds.shade_rays_f32(opts32(), orig.astype(np.float64), d.astype(np.float64))
