#!/usr/bin/env python3
"""Radiance-query throughput on the C3 scene (bunny.geom baked x30 + ground
plane, mesh-bunny.nim camera): ms per call and Mray/s of
DeviceScene.shade_rays (device form, float64, float32 colours out, no Stats):

  primary         the 1920x1080 akNone primary rays, in pixel order
  shuffled        the same rays in a random order
  shuffled_sorted that order with RT_QUERY_SORT (the sort is inside the timed
                  region: it is part of the call)

and, beside them, the float64 akNone frame with RT_FLAG_F64_PER_LANE
(k_render<double>): the same rays through the same shade_path, formed in the
kernel instead of read from memory. The frame is there to expose a gross
defect of the query kernel, not as a target.

The rays are castPrimaryRay (renderer.nim:31-44) in numpy, operation for
operation as the float64 kernels form them, so `primary_equals_frame` reports
the share of pixels whose colour is the frame's bit for bit (1.0 expected);
`shuffled_equals_primary` and `sorted_equals_shuffled` compare the timed
calls' outputs.

Each case: `--warmup` untimed calls, then `--repeats` calls timed one by one
with device events around the call, the members of a pair alternating so that
drift hits both alike; the median and the spread are reported. Needs a GPU;
prints one JSON line and appends it to --out.

    python tools/shade_bench.py --out profiles/shade/shade_bench.jsonl
"""
import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))


def primary_rays(c2w, fov, w, h):
    """castPrimaryRay for every integer pixel, row by row: (orig, dir), (w*h, 3)."""
    m = np.asarray(c2w, np.float64).reshape(16)          # glm column-major
    f = math.tan(fov * (3.14159265358979323846 / 180.0) / 2)
    aspect = float(w) / float(h)
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px, py = X.ravel(), Y.ravel()
    cx = ((2.0 * px * aspect) / float(w) - aspect) * f
    cy = (1.0 - (2.0 * py) / float(h)) * f
    cz = np.full_like(cx, -1.0)
    ln = np.sqrt((((0.0 + cx * cx) + cy * cy) + cz * cz) + 0.0)
    v = (cx / ln, cy / ln, cz / ln)
    d = np.empty((w * h, 3))
    o = np.empty((w * h, 3))
    for r in range(3):                                   # glm Mat4 * Vec4: columns summed from zero, in order
        d[:, r] = (((0.0 + m[r] * v[0]) + m[4 + r] * v[1]) + m[8 + r] * v[2]) + m[12 + r] * 0.0
        o[:, r] = (((0.0 + m[r] * 0.0) + m[4 + r] * 0.0) + m[8 + r] * 0.0) + m[12 + r] * 1.0
    return o, d


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shade", "shade_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, akNone, scenes
    from rtmi._lib import library_source_hash
    from rtmi.abi import RT_FLAG_F64_PER_LANE
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("shade_bench.py needs a GPU")
    w, h = args.width, args.height
    n = w * h
    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    opts = Options(width=w, height=h, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64,
                   flags=RT_FLAG_F64_PER_LANE)
    o_h, d_h = primary_rays(scene.cameraToWorld, scene.fov, w, h)
    perm = np.random.default_rng(args.seed).permutation(n)
    o, d = torch.from_numpy(o_h).cuda(), torch.from_numpy(d_h).cuda()
    o_s, d_s = torch.from_numpy(o_h[perm]).cuda(), torch.from_numpy(d_h[perm]).cuda()
    fb = torch.zeros(n * 3, dtype=torch.float32, device="cuda")

    cases = {
        "primary": lambda: ds.shade_rays(opts, o, d, f32=True),
        "frame_f64_per_lane": lambda: ds.render_device(opts, fb, stats=False),
        "shuffled": lambda: ds.shade_rays(opts, o_s, d_s, f32=True),
        "shuffled_sorted": lambda: ds.shade_rays(opts, o_s, d_s, f32=True, sort=True),
    }
    # what is timed computes what it should
    a, st = ds.shade_rays(opts, o, d, f32=True, stats=True)
    fst = ds.render_device(opts, fb)
    b, c = cases["shuffled"](), cases["shuffled_sorted"]()
    torch.cuda.synchronize()
    frame = fb.view(n, 3)
    order = torch.from_numpy(perm).cuda()
    out = {"tool": "shade_bench", "scene": "C3 mesh-bunny (69,451 triangles + ground)", "precision": "fp64",
           "width": w, "height": h, "rays": n, "library_source_hash": library_source_hash(),
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
           "primary_equals_frame": float((a.view(torch.int32) == frame.view(torch.int32)).all(1).float().mean()),
           "stats_equal_frame": bool(st == fst),
           "shuffled_equals_primary": bool(torch.equal(b.view(torch.int32), a[order].view(torch.int32))),
           "sorted_equals_shuffled": bool(torch.equal(b.view(torch.int32), c.view(torch.int32))),
           "shadow_rays": st.numShadowRays, "cases": {}}
    results = {k: [] for k in cases}
    for pair in (("primary", "frame_f64_per_lane"), ("shuffled", "shuffled_sorted")):
        for k in pair:
            timed(torch, cases[k], args.warmup, 0)
        for _ in range(args.repeats):
            for k in pair:
                results[k] += timed(torch, cases[k], 0, 1)
    for k in cases:
        ms = np.array(results[k])
        med = float(np.median(ms))
        out["cases"][k] = {"ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4),
                           "ms_max": round(float(ms.max()), 4), "mray_per_s": round(n / med / 1e3, 2)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
