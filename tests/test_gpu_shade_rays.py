"""Radiance queries (DeviceScene.shade_rays, rt_shade_rays*) on the device:
shade(ray, trace(ray)) (renderer.nim:47-127) for caller-supplied rays.

Where the rays are what oracle.cast_primary_ray returns, the oracle's own
calc_pixel is the expected answer: colours are compared as bit patterns (NaN
equal to NaN), Stats with ==. Rays the oracle's camera cannot form
(unnormalised directions) are checked against the multiprecision truth
(tests/golden/truth_shade_*.npz, shade_cases.py). test_shade_cases_cpu.py
proves that the inputs hit every object, are lit and shadowed, and reflect."""
import ctypes as C
import functools

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, akGrid
from rtmi import abi
from rtmi._lib import RtmiError, check, lib
from rtmi.renderer import DeviceScene
from rtmi.scene import DistantLight, PointLight, Stats
from rtmi.glm import normalize, point, vec, vec3

import shade_cases as sc
import truth
from subset_scenes import subset_scene

pytestmark = pytest.mark.gpu

NAMES = list(sc.SCENES)
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731


@functools.lru_cache(maxsize=None)
def device_scene(name):
    return DeviceScene(sc.SCENES[name]())


def shade_both(ds, opts, orig, d, group=1, flags=0):
    """rt_shade_rays with both outputs: (rgb float64, rgb32 float32, Stats)."""
    orig, d = np.ascontiguousarray(orig, np.float64), np.ascontiguousarray(d, np.float64)
    n = len(orig)
    rgb = np.full((n // group, 3), np.nan)
    rgb32 = np.full((n // group, 3), np.nan, np.float32)
    o, st = opts.to_c(), abi.rt_stats()
    check(lib().rt_shade_rays(ds.h, C.byref(o), n, _dp(orig), _dp(d), group, flags, _dp(rgb),
                              rgb32.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return rgb, rgb32, Stats.from_c(st)


def same(got, want):
    rgb, rgb32, st = got
    w_rgb, w_rgb32, w_st = want[:3]
    assert sc.same_bits(rgb, w_rgb), np.argwhere(rgb != w_rgb)[:5]
    assert sc.same_bits(rgb32, w_rgb32), np.argwhere(rgb32 != w_rgb32)[:5]
    assert st == w_st, (st, w_st)


# ---- 1. calcPixelNoSampling --------------------------------------------------------------
@pytest.mark.parametrize("bias", [sc.BIAS, 1e-8])
@pytest.mark.parametrize("name", NAMES)
def test_calc_pixel_no_sampling(gpu, oracle_mod, name, bias):
    orig, d = sc.scene_rays(oracle_mod, name, sc.W1, sc.H1)
    assert len(orig) == 165
    opts = sc.options(sc.W1, sc.H1, 0, bias)
    want = sc.expected(oracle_mod, name, sc.W1, sc.H1, 0, bias)
    ds = device_scene(name)
    same(shade_both(ds, opts, orig, d), want)
    # the Python method: one output at a time, the same bytes
    rgb, st = ds.shade_rays(opts, orig, d, stats=True)
    assert rgb.dtype == np.float64 and sc.same_bits(rgb, want[0]) and st == want[2]
    rgb32 = ds.shade_rays(opts, orig, d, f32=True)
    assert rgb32.dtype == np.float32 and sc.same_bits(rgb32, want[1])


# ---- 2. calcPixel ------------------------------------------------------------------------
@pytest.mark.parametrize("m", sc.GRID_M)
@pytest.mark.parametrize("name", NAMES)
def test_calc_pixel(gpu, oracle_mod, name, m):
    orig, d = sc.scene_rays(oracle_mod, name, sc.W2, sc.H2, m)
    assert len(orig) == 20 * m * m
    opts = sc.options(sc.W2, sc.H2, m)
    same(shade_both(device_scene(name), opts, orig, d, group=m * m), sc.expected(oracle_mod, name, sc.W2, sc.H2, m))


# ---- 3. the scene's camera is not read ---------------------------------------------------
def test_camera_independence(gpu, oracle_mod):
    scene = subset_scene(63)
    ds = device_scene("s63")                # keeps its own camera throughout
    cams = sc.cameras63()
    parts = [sc.camera_rays(oracle_mod, c2w, fov, sc.CAM_W, sc.CAM_H) for c2w, fov in cams.values()]
    orig, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    opts = sc.options(sc.CAM_W, sc.CAM_H)
    rgb, rgb32, st = shade_both(ds, opts, orig, d)
    n = sc.CAM_W * sc.CAM_H
    total = Stats()
    for k, (cname, (c2w, fov)) in enumerate(cams.items()):
        w_rgb, w_fb, w_st, _ = sc.oracle_image(oracle_mod, sc.with_camera(scene, c2w, fov), sc.CAM_W, sc.CAM_H)
        assert sc.same_bits(rgb[k * n:(k + 1) * n], w_rgb), cname
        assert sc.same_bits(rgb32[k * n:(k + 1) * n], w_fb), cname
        # each part alone: its own Stats
        assert shade_both(ds, opts, *parts[k])[2] == w_st, cname
        total += w_st
    assert st == total


# ---- 4. RT_QUERY_SORT --------------------------------------------------------------------
def test_sort_gives_the_same_bytes(gpu, oracle_mod):
    orig, d = sc.scene_rays(oracle_mod, "s63", sc.W2, sc.H2, 3)
    perm = np.random.default_rng(4).permutation(len(orig))
    orig, d = orig[perm].copy(), d[perm].copy()
    d[7] = 0.0                              # degenerate rays sort last
    orig[100, 1] = np.nan
    opts = sc.options(sc.W2, sc.H2, 3)
    ds = device_scene("s63")
    plain = shade_both(ds, opts, orig, d, group=9)
    srt = shade_both(ds, opts, orig, d, group=9, flags=abi.RT_QUERY_SORT)
    same(srt, plain)
    assert plain[2].numPrimaryRays == len(orig) - 2
    # and one colour per ray
    same(shade_both(ds, opts, orig, d, flags=abi.RT_QUERY_SORT), shade_both(ds, opts, orig, d))
    assert sc.same_bits(ds.shade_rays(opts, orig, d, group=9, sort=True), plain[0])


# ---- 5. device form ----------------------------------------------------------------------
@pytest.mark.parametrize("group,m", [(1, 0), (9, 3)])
def test_device_form(gpu, oracle_mod, group, m):
    import torch
    w, h = (sc.W1, sc.H1) if m == 0 else (sc.W2, sc.H2)
    orig, d = sc.scene_rays(oracle_mod, "s63", w, h, m)
    opts = sc.options(w, h, m)
    ds = device_scene("s63")
    host = shade_both(ds, opts, orig, d, group=group)
    t_o, t_d = torch.from_numpy(np.array(orig)).cuda(), torch.from_numpy(np.array(d)).cuda()
    rgb, st = ds.shade_rays(opts, t_o, t_d, group=group, stats=True)
    assert rgb.is_cuda and rgb.dtype == torch.float64 and tuple(rgb.shape) == (len(orig) // group, 3)
    assert sc.same_bits(rgb.cpu().numpy(), host[0]) and st == host[2]
    # out == NULL: only enqueued, on the stream given; sorted or not
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    rgb32 = ds.shade_rays(opts, t_o, t_d, group=group, f32=True, sort=True, stream=stream)
    assert rgb32.is_cuda and rgb32.dtype == torch.float32
    stream.synchronize()
    assert sc.same_bits(rgb32.cpu().numpy(), host[1])


# ---- 6. depth ----------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 1, 7])
def test_depth(gpu, oracle_mod, depth):
    orig, d = sc.scene_rays(oracle_mod, "s63", sc.W1, sc.H1)
    opts = sc.options(sc.W1, sc.H1, 0, sc.BIAS, depth)
    want = sc.expected(oracle_mod, "s63", sc.W1, sc.H1, 0, sc.BIAS, depth)
    same(shade_both(device_scene("s63"), opts, orig, d), want)
    assert (want[2].numReflectionRays > 0) == (depth > 0)


def test_depth_limits(gpu, oracle_mod):
    orig, d = sc.scene_rays(oracle_mod, "s63", sc.W1, sc.H1)
    with pytest.raises(RtmiError) as e:
        device_scene("s63").shade_rays(sc.options(sc.W1, sc.H1, 0, sc.BIAS, 8), orig, d)
    assert e.value.code == abi.RT_E_UNSUPPORTED
    # without reflective materials any depth is accepted
    orig, d = sc.scene_rays(oracle_mod, "s19", sc.W1, sc.H1)
    want = sc.expected(oracle_mod, "s19", sc.W1, sc.H1, 0, sc.BIAS, 100)
    same(shade_both(device_scene("s19"), sc.options(sc.W1, sc.H1, 0, sc.BIAS, 100), orig, d), want)


# ---- 7. degenerate rays ------------------------------------------------------------------
BAD = {3: ("orig", (np.nan, 1.0, 2.0)), 70: ("dir", (0.0, -np.inf, 1.0)), 130: ("dir", (0.0, 0.0, 0.0)),
       131: ("dir", (-0.0, 0.0, -0.0)), 164: ("orig", (0.0, np.inf, 0.0)),
       **{k: ("dir", (0.0, 0.0, 0.0)) for k in range(45, 60)}}  # whole groups of 3, 5 and 15


@pytest.mark.parametrize("group", [1, 3, 5, 15])
def test_degenerate_rays(gpu, oracle_mod, group):
    orig, d = (np.array(a) for a in sc.scene_rays(oracle_mod, "s63", sc.W1, sc.H1))
    w_rgb, _, _, per_px = sc.expected(oracle_mod, "s63", sc.W1, sc.H1)
    for k, (which, v) in BAD.items():
        (orig if which == "orig" else d)[k] = v
    good = np.ones(len(orig), bool)
    good[list(BAD)] = False
    colours = np.where(good[:, None], w_rgb, 0.0)   # a degenerate ray: (+0, +0, +0)
    want = colours if group == 1 else sc.ordered_mean(colours, group)
    rgb, rgb32, st = shade_both(device_scene("s63"), sc.options(sc.W1, sc.H1), orig, d, group=group)
    assert sc.same_bits(rgb, want)
    assert sc.same_bits(rgb32, want.astype(np.float32))
    assert sc.stats_tuple(st) == tuple(per_px[good].sum(0))
    assert st.numPrimaryRays == good.sum()
    if group == 1:
        assert not rgb[~good].any() and not np.signbit(rgb[~good]).any()
    else:
        whole = ~good.reshape(-1, group).any(1)     # groups of degenerate rays alone
        assert whole.any() and not rgb[whole].any()


# ---- 8. after edits ------------------------------------------------------------------------
def test_after_edits(gpu, oracle_mod):
    scene = subset_scene(19)                # sphere, box, point light: nothing reflects
    ds = DeviceScene(scene)
    orig, d = sc.scene_rays(oracle_mod, "s19", sc.W1, sc.H1)
    opts = sc.options(sc.W1, sc.H1)
    before = sc.expected(oracle_mod, "s19", sc.W1, sc.H1)
    same(shade_both(ds, opts, orig, d), before)
    assert before[2].numReflectionRays == 0
    edited = subset_scene(19)
    edited.lights = [DistantLight(color=vec3(1.0, 0.9, 0.8), intensity=3.0, dir=normalize(vec(1.0, -1.0, -0.5))),
                     PointLight(color=vec3(0.6, 0.8, 1.0), intensity=2000.0, pos=point(-4.0, 9.0, -6.0)),
                     DistantLight(color=vec3(0.2, 0.3, 0.2), intensity=1.5, dir=normalize(vec(-0.2, -1.0, 0.4)))]
    ds.set_lights(edited.lights)
    same(shade_both(ds, opts, orig, d), sc.oracle_image(oracle_mod, edited, sc.W1, sc.H1))
    # a reflective box and ground: the other instantiation
    edited.objects[2].material.reflection = 0.6
    edited.objects[-1].material.reflection = 0.25
    ds.set_objects(edited.objects)
    want = sc.oracle_image(oracle_mod, edited, sc.W1, sc.H1)
    assert want[2].numReflectionRays > 0
    same(shade_both(ds, opts, orig, d), want)
    with pytest.raises(RtmiError) as e:     # and the depth limit now applies
        ds.shade_rays(sc.options(sc.W1, sc.H1, 0, sc.BIAS, 8), orig, d)
    assert e.value.code == abi.RT_E_UNSUPPORTED
    ds.close()


# ---- 9. unnormalised directions: the multiprecision truth ---------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("bits", sc.TRUTH_BITS)
def test_unnormalised_directions(gpu, bits, sort):
    f = truth.load(f"shade_{bits}")
    ok = f["margin"] >= truth.EPS
    assert ok.mean() >= 0.98
    orig, d = f["orig"][ok], f["dir"][ok]
    assert (np.abs(np.linalg.norm(d, axis=1) - 1.0) > 0.5).sum() >= len(d) // 2
    opts = sc.options(1, 1)
    rgb, rgb32, st = shade_both(device_scene(f"s{bits}"), opts, orig, d, flags=abi.RT_QUERY_SORT if sort else 0)
    bad = np.argwhere(~truth.within_f32_ulp(rgb32, f["rgb"][ok]))
    assert len(bad) == 0, (bad[:5], rgb32[bad[0][0]], f["rgb"][ok][bad[0][0]])
    assert sc.same_bits(rgb.astype(np.float32), rgb32)
    assert sc.stats_tuple(st) == tuple(int(x) for x in f["counts"][ok].sum(0))


# ---- 10. the render state is left alone -----------------------------------------------------
def _last_stats(ds):
    st = abi.rt_stats()
    assert lib().rt_scene_last_stats(ds.h, C.byref(st)) == abi.RT_OK
    return st.as_dict()


def test_render_state_untouched(gpu, oracle_mod):
    import torch
    ds = DeviceScene(subset_scene(4))       # the torus on the ground: a two-class float32 launch
    opts = Options(width=64, height=48, antialias=Antialias(akGrid, 8), bias=sc.BIAS, precision=Precision.fp32)
    fb = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    before = (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds))
    assert before[3]["num_primary_rays"] == st.numPrimaryRays == 64 * 48 * 64
    sc4 = subset_scene(4)
    orig, d = sc.camera_rays(oracle_mod, sc4.cameraToWorld, sc4.fov, sc.W2, sc.H2, 3)
    q_opts = sc.options(sc.W2, sc.H2, 3)
    got = shade_both(ds, q_opts, orig, d, group=9, flags=abi.RT_QUERY_SORT)
    assert (ds.last_split(), ds.last_lean_kernel(), ds.last_batch(), _last_stats(ds)) == before
    same(got, sc.oracle_image(oracle_mod, sc4, sc.W2, sc.H2, 3))
    fb2 = torch.zeros_like(fb)
    assert ds.render_device(opts, fb2) == st
    assert torch.equal(fb, fb2)
    ds.close()


# ---- 11. errors -------------------------------------------------------------------------------
def test_errors(gpu, oracle_mod):
    ds = device_scene("s63")
    orig, d = (np.array(a[:12]) for a in sc.scene_rays(oracle_mod, "s63", sc.W1, sc.H1))
    o64 = sc.options(4, 3).to_c()
    rgb, rgb32, st = np.zeros((12, 3)), np.zeros((12, 3), np.float32), abi.rt_stats()
    p32 = rgb32.ctypes.data_as(C.POINTER(C.c_float))

    def call(n=12, group=1, flags=0, opts=o64, a=orig, b=d, out=rgb, out32=p32):
        return lib().rt_shade_rays(ds.h, C.byref(opts) if opts is not None else None, n, _dp(a) if a is not None else None,
                                   _dp(b) if b is not None else None, group, flags,
                                   _dp(out) if out is not None else None, out32, C.byref(st))

    assert call() == abi.RT_OK
    assert call(group=5) == abi.RT_E_INVALID and b"group" in lib().rt_last_error()
    assert call(group=0) == abi.RT_E_INVALID
    assert call(group=-3) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID
    assert call(flags=abi.RT_QUERY_SORT | abi.RT_QUERY_ANY_HIT) == abi.RT_E_INVALID
    assert call(flags=0x10) == abi.RT_E_INVALID
    o32 = sc.options(4, 3).to_c()
    o32.precision = abi.RT_FP32
    assert call(opts=o32) == abi.RT_E_UNSUPPORTED and b"float64" in lib().rt_last_error()
    assert call(opts=None) == abi.RT_E_INVALID
    assert call(out=None, out32=None) == abi.RT_E_INVALID
    assert call(out=None) == abi.RT_OK and call(out32=None) == abi.RT_OK
    assert call(n=-1) == abi.RT_E_INVALID
    assert call(a=None) == abi.RT_E_INVALID and call(b=None) == abi.RT_E_INVALID
    assert call(n=2 ** 31) == abi.RT_E_UNSUPPORTED
    # n == 0: RT_OK, nothing launched, zero Stats; a bad group is still refused
    st.num_primary_rays = 7
    assert call(n=0, a=None, b=None, out=None, out32=None) == abi.RT_OK and st.num_primary_rays == 0
    assert call(n=0, group=0) == abi.RT_E_INVALID
    # the Python method raises with the code
    with pytest.raises(RtmiError) as e:
        ds.shade_rays(sc.options(4, 3), orig, d, group=5)
    assert e.value.code == abi.RT_E_INVALID
    with pytest.raises(ValueError):
        ds.shade_rays(sc.options(4, 3), orig, d[:6])
