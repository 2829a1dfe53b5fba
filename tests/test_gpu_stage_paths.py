"""The host forms' staging across kinds on ONE scene: every host-form family
(trace, pick, shade and their _f32 forms, the feature buffers of both
precisions) called in turn, each followed by its device form on a side stream
with the same inputs — every returned array and the Stats equal byte for
byte. The sizes make the queries' staging buffer grow twice (64 -> 4096 ->
4097 rays) and be reused by smaller batches of another kind in between."""
import dataclasses

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, akGrid, scenes
from rtmi.glm import mat4, translate, vec3
from rtmi.renderer import DeviceScene
from rtmi.scene import Material, Object, initSphere

pytestmark = pytest.mark.gpu


def _scene():
    """A small mesh, a sphere and a plane."""
    sc = scenes._mesh_scene(scenes.torus_mesh(8, 6), "torus", (0.9, 0.5, 0.2))
    sc.objects.append(Object("ball", initSphere(r=1.5, objectToWorld=translate(mat4(1.0), vec3(5.0, 1.5, -11.0))),
                             Material(albedo=vec3(0.2, 0.5, 0.9))))
    return sc


def _rays(n, seed):
    """n rays from around the scene towards it (float64; directions not normalised)."""
    rng = np.random.default_rng(seed)
    orig = rng.normal(size=(n, 3))
    orig = 14.0 * orig / np.linalg.norm(orig, axis=1, keepdims=True) + np.array([0.0, 4.0, -12.0])
    orig[:, 1] = np.abs(orig[:, 1]) + 0.5
    target = np.array([1.5, 1.0, -12.0]) + rng.uniform(-4.0, 4.0, size=(n, 3))
    return np.ascontiguousarray(orig), np.ascontiguousarray((target - orig) * rng.uniform(0.5, 2.0, size=(n, 1)))


def _same(host, device, what):
    """Host-form results against device-form results: tuples of arrays (and a
    Stats), or a dict of arrays."""
    if isinstance(host, dict):
        assert host.keys() == device.keys(), what
        host, device = tuple(host.values()), tuple(device[k] for k in host)
    assert len(host) == len(device), what
    for k, (h, d) in enumerate(zip(host, device)):
        if dataclasses.is_dataclass(h):
            assert h == d, (what, h, d)
            continue
        d = d.cpu().numpy()
        assert h.dtype == d.dtype and h.shape == d.shape, (what, k, h.dtype, d.dtype, h.shape, d.shape)
        assert h.tobytes() == d.tobytes(), (what, k)


def test_host_forms_share_the_staging_across_kinds(gpu):
    import torch
    ds = DeviceScene(_scene(), device=0)
    side = torch.cuda.Stream(device="cuda:0")

    o32 = Options(width=16, height=16, antialias=Antialias(akGrid, 2), bias=1e-4, precision=Precision.fp32)
    o64 = dataclasses.replace(o32, precision=Precision.fp64)
    xy = np.random.default_rng(5).uniform(-1.0, 17.0, size=(65, 2))
    ins = {"xy32": xy.astype(np.float32), "xy1": xy[:1].copy()}
    for key, n, dt in (("a", 64, np.float64), ("b", 4096, np.float32), ("c", 4097, np.float32)):
        ins[key + ".orig"], ins[key + ".dir"] = (a.astype(dt) for a in _rays(n, n))
    on_device = {k: torch.from_numpy(a).to("cuda:0") for k, a in ins.items()}
    for key, ft in (("aov32", torch.float32), ("aov64", torch.float64)):  # the device forms' zeroed outputs
        ins[key] = None
        on_device[key] = {c: torch.zeros((16, 16, 3) if c in ("normal", "albedo") else (16, 16), device="cuda:0",
                                         dtype=torch.int32 if c in ("object", "face") else ft)
                          for c in DeviceScene.AOV_CHANNELS}
    torch.cuda.synchronize()  # the side stream reads them
    # (name, the call: given where the inputs are and the stream argument)
    steps = [
        ("trace_rays", lambda i, kw: ds.trace_rays(i["a.orig"], i["a.dir"], normals=True, stats=True, **kw)),
        ("shade_rays_f32", lambda i, kw: ds.shade_rays_f32(o32, i["b.orig"], i["b.dir"], group=4, stats=True, **kw)),
        ("pick_f32", lambda i, kw: ds.pick_f32(o32, i["xy32"], normals=True, stats=True, **kw)),
        ("render_aovs", lambda i, kw: ds.render_aovs(o32, stats=True, host=not kw, out=i["aov32"], **kw)),
        ("shade_rays", lambda i, kw: ds.shade_rays(o64, i["a.orig"], i["a.dir"], f32=True, stats=True, **kw)),
        ("trace_rays_f32", lambda i, kw: ds.trace_rays_f32(i["c.orig"], i["c.dir"], sort=True, stats=True, **kw)),
        ("render_aovs_f64", lambda i, kw: ds.render_aovs_f64(o64, y0=3, y1=9, stats=True, host=not kw, out=i["aov64"], **kw)),
        ("pick", lambda i, kw: ds.pick(o64, i["xy1"], stats=True, **kw)),
    ]
    for name, call in steps:
        host = call(ins, {})
        if name.startswith("trace_rays"):  # (the batch is worth comparing: hits and misses)
            assert 0 < int((host[1] >= 0).sum()) < len(host[1]), name
        device = call(on_device, {"stream": side})
        if name.startswith("render_aovs"):
            (hb, hs), (db, dst) = host, device
            _same(hb, db, name)
            assert hs == dst, (name, hs, dst)
        else:
            _same(host, device, name)
