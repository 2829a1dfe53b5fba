#!/usr/bin/env python3
"""Feature-buffer call times on the C3 scene (bunny.geom baked x30 + ground
plane, mesh-bunny.nim camera) at 1920x1080, akNone (1 spp), akGrid m = 4 (16
spp) and m = 16 (256 spp). Per sampling, alternating in one process so that
drift hits all alike:

  aov          DeviceScene.render_aovs, all six channels, into buffers made once
  aov_nobin    the same with RT_FLAG_NO_BINNING (camera rays through the BVH)
  colour       DeviceScene.render_device of the same options (no Stats)
  picks        at 1 and 16 spp, the only route without the call: pick_f32 with
               normals over every sample position (uploaded once, outside the
               timed region) and the per-pixel reduction in torch

Each route: `--warmup` untimed calls, then `--repeats` calls timed one by one
with device events around the call; the median and the spread are reported,
with the HBM bytes the route must move, computed from the shapes (the scene's
own reads not counted). `equal` says whether the picks route's alpha, depth,
object and face equal the call's. Needs a GPU; prints one JSON line and
appends it to --out.

    python tools/aov_bench.py --out profiles/aov/aov_bench.jsonl
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "aov", "aov_bench.jsonl"))
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, scenes
    from rtmi._lib import library_source_hash
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("aov_bench.py needs a GPU")
    w, h = args.width, args.height
    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    npx = w * h
    albedo = torch.tensor([[float(np.float32(c)) for c in ob.material.albedo] for ob in scene.objects],
                          dtype=torch.float32, device="cuda")
    out = {"tool": "aov_bench", "scene": "C3 mesh-bunny (69,451 triangles + ground)", "width": w, "height": h,
           "library_source_hash": library_source_hash(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "cases": {}}

    def opts(kind, m, flags=0):
        return Options(width=w, height=h, antialias=Antialias(kind, m), bias=1e-4, precision=Precision.fp32,
                       flags=flags)

    for kind, m in ((akNone, 1), (akGrid, 4), (akGrid, 16)):
        spp = m * m
        bufs = ds.render_aovs(opts(kind, m))
        fb = torch.zeros(npx * 3, dtype=torch.float32, device="cuda")
        pick_o = opts(akNone, 1)
        routes = {
            "aov": lambda: ds.render_aovs(opts(kind, m), out=bufs),
            "aov_nobin": lambda: ds.render_aovs(opts(kind, m, abi.RT_FLAG_NO_BINNING), out=bufs),
            "colour": lambda: ds.render_device(opts(kind, m, abi.RT_FLAG_NO_STATS), fb, stats=False),
        }
        hbm = {"aov": npx * 40, "aov_nobin": npx * 40, "colour": npx * 12}
        reduced = {}
        if spp <= 16:
            off = (np.arange(m, dtype=np.float32) + 0.5) / m if kind == akGrid else np.zeros(1, np.float32)
            X = torch.arange(w, dtype=torch.float32, device="cuda")
            Y = torch.arange(h, dtype=torch.float32, device="cuda")
            sx = torch.from_numpy(np.tile(off, m)).cuda()
            sy = torch.from_numpy(np.repeat(off, m)).cuda()
            xy = torch.stack([(X[None, :, None] + sx[None, None, :]).expand(h, w, spp),
                              (Y[:, None, None] + sy[None, None, :]).expand(h, w, spp)], -1).reshape(-1, 2).contiguous()
            inv_len = float(np.float32(1.0 / spp))

            def picks():
                t, obj, face, nrm = ds.pick_f32(pick_o, xy, normals=True)
                t, obj, face = t.view(h, w, spp), obj.view(h, w, spp), face.view(h, w, spp)
                hit = obj >= 0
                reduced["alpha"] = hit.sum(2).float() * inv_len
                depth, win = torch.where(hit, t, torch.full_like(t, float("inf"))).min(2)
                reduced["depth"] = depth
                reduced["object"] = torch.gather(obj, 2, win[..., None])[..., 0]
                reduced["face"] = torch.gather(face, 2, win[..., None])[..., 0]
                reduced["normal"] = nrm.view(h, w, spp, 3).sum(2) * inv_len
                reduced["albedo"] = (albedo[obj.clamp(min=0).long()] * hit[..., None]).sum(2) * inv_len

            routes["picks"] = picks
            # positions in, hits and normals out; the reduction reads them back and writes the six channels
            hbm["picks"] = npx * spp * (8 + 2 * (16 + 12)) + npx * 40
        res = {k: [] for k in routes}
        for k in routes:
            timed(torch, routes[k], args.warmup, 0)
        for _ in range(args.repeats):
            for k in routes:
                res[k] += timed(torch, routes[k], 0, 1)
        row = {"spp": spp, "samples": npx * spp}
        for k, ms in res.items():
            ms = np.array(ms)
            row[k] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                      "ms_max": round(float(ms.max()), 4), "hbm_bytes": int(hbm[k])}
        if reduced:
            routes["aov"]()
            torch.cuda.synchronize()
            row["equal"] = bool(all(torch.equal(reduced[c], bufs[c]) for c in ("alpha", "depth", "object", "face")))
        out["cases"][f"spp{spp}"] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
