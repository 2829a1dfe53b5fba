"""The device against the multiprecision truth (truth.py), from the recorded
fixtures tests/golden/truth_*.npz alone: no oracle, no mpmath. Every other
GPU test compares a kernel with oracle/rt_oracle.c, written from the same
reading of the reference as the kernels; these compare it with the written
specification evaluated in 200-bit arithmetic, so a misreading the two share
(a rotation's sense, a transposed matrix, how a normal reaches world space,
the point light's 4 pi r^2, the sphere's `/2*a`, the box normal's truncation)
fails here.

Answers the truth calls undecided (margin < EPS: float64 may honestly decide
them the other way) are left out; test_truth_cpu.py caps their share. The
tolerances on t and normals are TOL times the error of the oracle measured
on the CPU when the fixtures were written (truth_meta.json), never a device
result."""
import functools

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, akGrid, akNone
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH, RT_FLAG_F64_PER_LANE
from rtmi.renderer import DeviceScene

import truth
import truth_cases as tc
from subset_scenes import subset_scene

pytestmark = pytest.mark.gpu

META = truth.meta()
TOL = META["tol_factor"]
RAY_CASES = [(n, b) for n in tc.BATCHES for b in ((RT_BVH_SAH, RT_BVH_PLOC) if n in tc.HAS_MESH else (RT_BVH_SAH,))]


@functools.lru_cache(maxsize=None)
def device_scene(name, builder=RT_BVH_SAH):
    return DeviceScene(tc.BATCHES[name](), bvh_builder=builder)


@functools.lru_cache(maxsize=None)
def frame_scene(bits):
    return DeviceScene(subset_scene(bits))


def decided(b):
    """The batch restricted to its decided rays: only those are sent."""
    ok = b["margin"] >= truth.EPS
    return {k: v[ok] for k, v in b.items()}


def check_rays(b, res, entry):
    t, obj, face, nrm, st = res
    tc.compare(b, {"t": t, "obj": obj, "face": face, "normal": nrm}, TOL * entry["t_ulp"], TOL * entry["normal_ulp"])
    assert st.numIntersectionTests == int(b["tests"].sum())
    assert st.numIntersectionHits == int(b["hits"].sum())


# ---- rt_trace_rays ------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", RAY_CASES)
def test_trace_rays(gpu, name, builder):
    whole = truth.load(name)
    b = decided(whole)
    assert len(b["t"]) >= (1.0 - tc.UNDECIDED_CAP) * len(whole["t"])
    res = device_scene(name, builder).trace_rays(b["orig"], b["dir"], b["tnear"], normals=True, stats=True)
    check_rays(b, res, META["batches"][name])
    if name in tc.HAS_MESH:
        assert (b["face"] >= 0).sum() >= 25        # mesh faces are among the answers


def test_trace_rays_sorted(gpu):
    b = decided(truth.load("s15"))
    res = device_scene("s15").trace_rays(b["orig"], b["dir"], b["tnear"], sort=True, normals=True, stats=True)
    check_rays(b, res, META["batches"]["s15"])


def test_trace_rays_device_form(gpu):
    import torch
    b = decided(truth.load("boxes2"))
    dev = [torch.from_numpy(np.ascontiguousarray(b[k])).cuda() for k in ("orig", "dir", "tnear")]
    res = device_scene("boxes2").trace_rays(*dev, normals=True, stats=True)
    check_rays(b, [r.cpu().numpy() for r in res[:4]] + [res[4]], META["batches"]["boxes2"])


@pytest.mark.parametrize("name,builder", RAY_CASES)
def test_any_hit(gpu, name, builder):
    b = decided(truth.load(name))
    _, obj, _, st = device_scene(name, builder).trace_rays(b["orig"], b["dir"], b["tnear"], any_hit=True, stats=True)
    assert np.array_equal(obj >= 0, b["obj"] >= 0)
    assert st.numIntersectionTests == int(b["tests"].sum())     # rtmi.h: the Stats are still the reference's
    assert st.numIntersectionHits == int(b["hits"].sum())


# ---- rt_pick_pixels: castPrimaryRay on the device -------------------------------------
@pytest.mark.parametrize("name", tc.PICK_SCENES)
def test_pick_pixels(gpu, name):
    b = decided(truth.load(f"pick_{name}"))
    assert len(b["t"]) >= (1.0 - tc.UNDECIDED_CAP) * 120
    inside = (b["xy"] >= 0).all(1) & (b["xy"][:, 0] < tc.PICK_W) & (b["xy"][:, 1] < tc.PICK_H)
    assert (~inside).sum() >= 10 and (b["xy"] != np.floor(b["xy"])).any(1).sum() >= 50
    opts = Options(width=tc.PICK_W, height=tc.PICK_H, precision=Precision.fp64)
    res = device_scene(name).pick(opts, b["xy"], normals=True, stats=True)
    check_rays(b, res, META["picks"][name])
    assert res[4].numPrimaryRays == len(b["xy"])


# ---- frames --------------------------------------------------------------------------
def render(bits, m, precision, flags=0):
    import torch
    opts = Options(width=tc.FRAME_W, height=tc.FRAME_H, antialias=Antialias(akGrid if m else akNone, max(m, 1)),
                   bias=tc.BIAS, maxRayDepth=tc.DEPTH, precision=precision, flags=flags)
    fb = torch.zeros(tc.FRAME_W * tc.FRAME_H * 3, dtype=torch.float32, device="cuda")
    st = frame_scene(bits).render_device(opts, fb)
    return fb.view(tc.FRAME_H, tc.FRAME_W, 3).cpu().numpy(), st


# the three float64 paths: akNone, one lane per pixel, one pixel per wave (k_render_px64)
@pytest.mark.parametrize("m,flags", [(0, 0), (2, RT_FLAG_F64_PER_LANE), (8, 0)])
@pytest.mark.parametrize("bits", tc.FRAME_BITS)
def test_float64_frame(gpu, bits, m, flags):
    f = truth.load(f"frame_{bits}_m{m}")
    assert (f["margin"] >= truth.EPS).all()      # the Stats are compared: no sample is undecided
    got, st = render(bits, m, Precision.fp64, flags)
    bad = np.argwhere(~truth.within_f32_ulp(got, f["rgb"]))
    assert len(bad) == 0, (bad[:5], got[tuple(bad[0][:2])], f["rgb"][tuple(bad[0][:2])])
    want = f["stats"].reshape(-1, 5).sum(0)
    assert (st.numPrimaryRays, st.numIntersectionTests, st.numIntersectionHits, st.numShadowRays,
            st.numReflectionRays) == tuple(int(x) for x in want)


@pytest.mark.parametrize("m", [2, 8])
@pytest.mark.parametrize("bits", tc.FRAME_BITS)
def test_float32_frame(gpu, bits, m):
    """The smooth-pixel bound of test_gpu_subsets.py, on the pixels the truth
    decides with room for float32."""
    f = truth.load(f"frame_{bits}_m{m}")
    ok = f["margin32"] >= truth.EPS32
    assert ok.mean() >= 0.5
    got, st = render(bits, m, Precision.fp32)
    err = np.abs(got.astype(np.float64) - f["rgb"]).max(axis=2)
    print(f"subset {bits} m {m}: {ok.mean():.3f} of the pixels decided, largest error {err[ok].max():.3g}")
    assert (err[ok] <= 1e-4).all(), (np.argwhere(ok & (err > 1e-4))[:5], err[ok].max())
    assert st.numPrimaryRays == int(f["stats"][..., 0].sum())


# ---- the output quantiser -----------------------------------------------------------------
@pytest.mark.parametrize("bits,srgb", tc.QUANT_CASES)
def test_ppm_encode_against_the_definition(gpu, bits, srgb):
    import torch

    from rtmi.renderer import ppm_encode_device
    z = truth.load("quant")
    v, q, und = z["v"], z[f"q_{bits}_{int(srgb)}"], z[f"und_{bits}_{int(srgb)}"]
    assert und.mean() <= tc.QUANT_CAP
    _, payload = ppm_encode_device(torch.from_numpy(v).cuda(), len(v) // 3, 1, bits, srgb)
    got = payload.cpu().numpy()
    got = got.view(">u2").astype(np.uint16) if bits > 8 else got.astype(np.uint16)
    assert np.array_equal(got[~und], q[~und]), np.flatnonzero((got != q) & ~und)[:8]
