#!/usr/bin/env python3
"""Float32 ray-query throughput on the C3 scene (bunny.geom baked x30 + ground
plane, mesh-bunny.nim camera): ms per call and Mray/s of
DeviceScene.trace_rays_f32 / pick_f32 (device forms, no Stats, no normals)
beside the float64 DeviceScene.trace_rays / pick on the same values, the two
alternating within a pair so that drift hits both alike:

  picks       the 1920x1080 integer pixel positions, in pixel order
  incoherent  2 M seeded rays in a random order: origins in a box three times
              the scene's extent, three quarters of the directions towards
              random points of the scene's bounds, the rest random (the
              batch of tests/test_gpu_query.py, larger), rounded to float32;
              the float64 query reads those float32 values widened

each as closest hit and as any-hit, without and with RT_QUERY_SORT (the sort
is inside the timed region: it is part of the call). `obj_equal` reports the
share of rays on which the float32 and the float64 query name the same object
(any-hit: agree on hit or no hit).

Each case: `--warmup` untimed calls, then `--repeats` calls timed one by one
with device events around the call; the median and the spread are reported.
Needs a GPU; prints one JSON line and appends it to --out.

    python tools/trace32_bench.py --out profiles/trace32/trace32_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from shade_bench import timed  # noqa: E402


def scene_bounds(scene):
    """World AABB of the scene's meshes (C3: the bunny)."""
    from rtmi.scene import TriangleMesh
    pts = []
    for o in scene.objects:
        g = o.geometry
        if isinstance(g, TriangleMesh):
            v = np.concatenate([g.vertices, np.ones((len(g.vertices), 1))], 1) @ np.asarray(g.objectToWorld, np.float64)
            pts += [v[:, :3].min(0), v[:, :3].max(0)]
    pts = np.array(pts)
    return pts.min(0), pts.max(0)


def incoherent_rays(scene, n, seed):
    lo, hi = scene_bounds(scene)
    rng = np.random.default_rng(seed)
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    d = rng.uniform(lo, hi, (n, 3)) - orig
    free = np.arange(n) % 4 == 3
    d[free] = rng.normal(0.0, 1.0, (int(free.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perm = rng.permutation(n)
    return np.ascontiguousarray(orig[perm].astype(np.float32)), np.ascontiguousarray(d[perm].astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace32", "trace32_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, akNone, scenes
    from rtmi._lib import library_source_hash
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("trace32_bench.py needs a GPU")
    w, h = args.width, args.height
    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    o32 = Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp32)
    o64 = Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64)

    out = {"tool": "trace32_bench", "scene": "C3 mesh-bunny (69,451 triangles + ground)", "width": w, "height": h,
           "library_source_hash": library_source_hash(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "trace32_subset": ds.trace32_subset(), "cases": {}}

    def run(name, pair, nrays, check):
        """pair: {label: call}; timed alternating; check(): extra fields."""
        res = {k: [] for k in pair}
        for k in pair:
            timed(torch, pair[k], args.warmup, 0)
        for _ in range(args.repeats):
            for k in pair:
                res[k] += timed(torch, pair[k], 0, 1)
        row = {"rays": nrays}
        for k, ms in res.items():
            ms = np.array(ms)
            med = float(np.median(ms))
            row[k] = {"ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4),
                      "ms_max": round(float(ms.max()), 4), "mray_per_s": round(nrays / med / 1e3, 2)}
        row["f64_over_f32"] = round(row["f64"]["ms_median"] / row["f32"]["ms_median"], 3)
        row.update(check())
        out["cases"][name] = row

    def equal(a, b, any_hit):
        oa, ob = a[1], b[1]
        same = ((oa >= 0) == (ob >= 0)) if any_hit else (oa == ob)
        return {"obj_equal": float(same.float().mean()), "hit_share": float((ob >= 0).float().mean())}

    X, Y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    xy32 = torch.from_numpy(np.ascontiguousarray(np.stack([X.ravel(), Y.ravel()], 1))).cuda()
    xy64 = xy32.double()
    ro, rd = incoherent_rays(scene, args.rays, args.seed)
    r32, d32 = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
    r64, d64 = r32.double(), d32.double()
    for any_hit in (False, True):
        for sort in (False, True):
            tag = ("any" if any_hit else "closest") + ("_sorted" if sort else "")
            kw = {"any_hit": any_hit, "sort": sort}
            run("picks_" + tag, {"f32": lambda: ds.pick_f32(o32, xy32, **kw), "f64": lambda: ds.pick(o64, xy64, **kw)},
                w * h, lambda: equal(ds.pick_f32(o32, xy32, **kw), ds.pick(o64, xy64, **kw), any_hit))
            run("incoherent_" + tag, {"f32": lambda: ds.trace_rays_f32(r32, d32, **kw),
                                      "f64": lambda: ds.trace_rays(r64, d64, **kw)},
                args.rays, lambda: equal(ds.trace_rays_f32(r32, d32, **kw), ds.trace_rays(r64, d64, **kw), any_hit))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
