#!/usr/bin/env python3
"""Float64 feature-buffer call times on the C3 scene (bunny.geom baked x30 +
ground plane, mesh-bunny.nim camera) at 1920x1080, akGrid m = 4 (16 spp: one
lane per pixel) and m = 16 (256 spp: one pixel per wave). Per sampling,
alternating in one process so that drift hits all alike:

  aov64        DeviceScene.render_aovs_f64, all six channels, into buffers made once
  aov64_lane   the same with RT_FLAG_F64_PER_LANE (m = 16: the other layout)
  aov64_nobin  the same with RT_FLAG_NO_BINNING (camera rays through the BVH)
  colour       DeviceScene.render_device of the same RT_FP64 options (no Stats)
  picks        the only route without the call: DeviceScene.pick with normals
               over every sample position (made on the device once, outside
               the timed region); the caller's reduction is not timed either

Each route: `--warmup` untimed calls, then `--repeats` calls timed one by one
with device events around the call; the median and the spread are reported,
with the HBM bytes the route must move, computed from the shapes (the scene's
own reads not counted). The picks route at 256 spp moves 56 B per sample
(30 GB): it gets --pick-repeats calls after one warm-up. `equal` says whether
the picks' hit count, smallest t and its ids equal the call's alpha, depth,
object and face. Needs a GPU; prints one JSON line and appends it to --out.

    python tools/aov64_bench.py --out profiles/aov64/aov64_bench.jsonl
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pick-repeats", type=int, default=3)
    ap.add_argument("--grids", default="4,16")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "aov64", "aov64_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, scenes
    from rtmi._lib import library_source_hash
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("aov64_bench.py needs a GPU")
    w, h = args.width, args.height
    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    npx = w * h
    out = {"tool": "aov64_bench", "scene": "C3 mesh-bunny (69,451 triangles + ground)", "width": w, "height": h,
           "library_source_hash": library_source_hash(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "pick_repeats": args.pick_repeats, "cases": {}}

    def opts(kind, m, flags=0):
        return Options(width=w, height=h, antialias=Antialias(kind, m), bias=1e-4, precision=Precision.fp64,
                       flags=flags)

    for m in [int(v) for v in args.grids.split(",")]:
        spp = m * m
        bufs = ds.render_aovs_f64(opts(akGrid, m))
        fb = torch.zeros(npx * 3, dtype=torch.float32, device="cuda")
        pick_o = opts(akNone, 1)
        # grid(): i * (1/m) + (1/m) * 0.5 in float64, as the kernels form it
        xs = 1.0 / m
        off = np.arange(m, dtype=np.float64) * xs + xs * 0.5
        sx = torch.from_numpy(np.tile(off, m)).cuda()
        sy = torch.from_numpy(np.repeat(off, m)).cuda()
        X = torch.arange(w, dtype=torch.float64, device="cuda")
        Y = torch.arange(h, dtype=torch.float64, device="cuda")
        xy = torch.empty((h, w, spp, 2), dtype=torch.float64, device="cuda")
        xy[..., 0] = X[None, :, None] + sx[None, None, :]
        xy[..., 1] = Y[:, None, None] + sy[None, None, :]
        xy = xy.view(-1, 2)
        picked = {}

        def picks():
            picked["r"] = ds.pick(pick_o, xy, normals=True)

        routes = {
            "aov64": lambda: ds.render_aovs_f64(opts(akGrid, m), out=bufs),
            "aov64_lane": lambda: ds.render_aovs_f64(opts(akGrid, m, abi.RT_FLAG_F64_PER_LANE), out=bufs),
            "aov64_nobin": lambda: ds.render_aovs_f64(opts(akGrid, m, abi.RT_FLAG_NO_BINNING), out=bufs),
            "colour": lambda: ds.render_device(opts(akGrid, m, abi.RT_FLAG_NO_STATS), fb, stats=False),
            "picks": picks,
        }
        # the six channels out (8 + 8 + 4 + 4 + 24 + 24 B per pixel); a float32 frame; per pick 16 B in,
        # a 16-B hit and a 24-B normal out
        hbm = {"aov64": npx * 72, "aov64_lane": npx * 72, "aov64_nobin": npx * 72, "colour": npx * 12,
               "picks": npx * spp * 56}
        reps = {k: (args.pick_repeats if k == "picks" and spp > 16 else args.repeats) for k in routes}
        res = {k: [] for k in routes}
        for k in routes:
            timed(torch, routes[k], 1 if k == "picks" and spp > 16 else args.warmup, 0)
        for i in range(args.repeats):
            for k in routes:
                if i < reps[k]:
                    res[k] += timed(torch, routes[k], 0, 1)
        row = {"spp": spp, "samples": npx * spp}
        for k, ms in res.items():
            ms = np.array(ms)
            row[k] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                      "ms_max": round(float(ms.max()), 4), "calls": int(ms.size), "hbm_bytes": int(hbm[k])}
        routes["aov64"]()
        torch.cuda.synchronize()
        t, obj, face, _ = picked["r"]
        t, obj, face = t.view(h, w, spp), obj.view(h, w, spp), face.view(h, w, spp)
        hit = obj >= 0
        depth, win = torch.where(hit, t, torch.full_like(t, float("inf"))).min(2)
        row["equal"] = bool(torch.equal(hit.sum(2).double() * (1.0 / spp), bufs["alpha"])
                            and torch.equal(depth, bufs["depth"])
                            and torch.equal(torch.gather(obj, 2, win[..., None])[..., 0], bufs["object"])
                            and torch.equal(torch.gather(face, 2, win[..., None])[..., 0], bufs["face"]))
        out["cases"][f"spp{spp}"] = row
        del xy, picked, t, obj, face, hit, depth, win
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
