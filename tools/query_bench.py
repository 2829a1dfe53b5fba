#!/usr/bin/env python3
"""Ray-query throughput on the C3 scene (bunny.geom baked x30 + ground plane,
mesh-bunny.nim camera), in Mray/s of DeviceScene.pick / trace_rays (device
forms, float64):

  picks       a whole 1920x1080 grid of integer pixel positions (coherent)
  incoherent  2 M rays with random origins around the scene and random
              targets inside it, without and with RT_QUERY_SORT (the sort is
              inside the timed region: it is part of the call)

Each case: `--warmup` untimed calls, then `--repeats` calls timed one by one
with device events around the call (no Stats: the call only enqueues), the
median and the spread reported. Needs a GPU; prints one JSON line and, with
--out, writes it to a file.

    python tools/query_bench.py --out profiles/query_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))


def scene_bounds(scene):
    """World AABB of the scene's meshes."""
    lo, hi = [], []
    for o in scene.objects:
        g = o.geometry
        if hasattr(g, "vertices"):
            v = np.concatenate([g.vertices, np.ones((len(g.vertices), 1))], 1) @ g.objectToWorld
            lo.append(v[:, :3].min(0))
            hi.append(v[:, :3].max(0))
    return np.min(lo, 0), np.max(hi, 0)


def incoherent_rays(scene, n, seed):
    """Origins in a box 3x the mesh's extent about its centre (above the
    ground), each aimed at a random point inside the mesh's bounds."""
    lo, hi = scene_bounds(scene)
    rng = np.random.default_rng(seed)
    c, e = 0.5 * (lo + hi), hi - lo
    orig = c + rng.uniform(-1.5, 1.5, (n, 3)) * e
    orig[:, 1] = np.abs(orig[:, 1]) + 0.01
    d = rng.uniform(lo, hi, (n, 3)) - orig
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return orig, d


def timed(torch, call, warmup, repeats):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, akNone, scenes
    from rtmi._lib import library_source_hash
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("query_bench.py needs a GPU")
    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    opts = Options(width=args.width, height=args.height, antialias=Antialias(akNone, 1), precision=Precision.fp64)
    X, Y = np.meshgrid(np.arange(args.width, dtype=np.float64), np.arange(args.height, dtype=np.float64))
    xy = torch.from_numpy(np.ascontiguousarray(np.stack([X.ravel(), Y.ravel()], 1))).cuda()
    o_h, d_h = incoherent_rays(scene, args.rays, args.seed)
    o, d = torch.from_numpy(o_h).cuda(), torch.from_numpy(d_h).cuda()

    cases = {
        "picks": (xy.shape[0], lambda: ds.pick(opts, xy)),
        "picks_sorted": (xy.shape[0], lambda: ds.pick(opts, xy, sort=True)),
        "incoherent": (args.rays, lambda: ds.trace_rays(o, d)),
        "incoherent_sorted": (args.rays, lambda: ds.trace_rays(o, d, sort=True)),
    }
    # the sorted and the unsorted call give the same answers (checked on what is timed)
    a, b = ds.trace_rays(o, d), ds.trace_rays(o, d, sort=True)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    hit = float((a[1] >= 0).float().mean())
    face = float((a[2] >= 0).float().mean())
    out = {"tool": "query_bench", "scene": "C3 mesh-bunny (69,451 triangles + ground)", "precision": "fp64",
           "library_source_hash": library_source_hash(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "sorted_equals_unsorted": bool(same),
           "incoherent_hit_fraction": hit, "incoherent_mesh_hit_fraction": face, "cases": {}}
    # alternate the incoherent pair so drift hits both alike
    results = {k: [] for k in cases}
    for k in ("picks", "picks_sorted"):
        results[k] = timed(torch, cases[k][1], args.warmup, args.repeats)
    for k in ("incoherent", "incoherent_sorted"):
        timed(torch, cases[k][1], args.warmup, 0)
    for _ in range(args.repeats):
        for k in ("incoherent", "incoherent_sorted"):
            results[k] += timed(torch, cases[k][1], 0, 1)
    for k, (n, _) in cases.items():
        ms = np.array(results[k])
        med = float(np.median(ms))
        out["cases"][k] = {"rays": int(n), "ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4),
                           "ms_max": round(float(ms.max()), 4), "mray_per_s": round(n / med / 1e3, 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
