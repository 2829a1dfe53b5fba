#!/usr/bin/env python3
"""What it costs to change a scene's lights: rt_scene_set_lights against the
only way there was before it, rt_scene_destroy + rt_scene_create, with the
host SAH builder and with the device PLOC builder. Two scenes — C3 (bunny.geom
baked x30 + ground, 69,451 triangles) and C5 (the 1M-triangle torus) — each
relit with one and with two distant lights (the direction moves every run).

Each case: `--warmup` untimed runs, then `--repeats` runs timed one by one on
the host clock (all three are synchronous calls: they return when the scene
is ready), the median and the spread reported. After the timed runs the
relight's device passes are timed once more with events between them
(rtmi_test_relight_passes). Needs a GPU; prints one JSON line per case and,
with --out, appends them to a file.

    python tools/relight_bench.py --out profiles/relight/relight_bench.jsonl
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))

PASSES = ("faces", "count", "scan", "records", "fill_order", "prefix_sums")


def lights_for(k, n):
    """n distant lights, the first one swinging with k (a time-of-day sweep)."""
    from rtmi.glm import normalize, vec, vec3
    from rtmi.scene import DistantLight
    a = 0.3 + 0.05 * k
    out = [DistantLight(color=vec3(1.0), intensity=4.0, dir=normalize(vec(-2.0 * math.cos(a), -0.8, -2.0 * math.sin(a))))]
    if n > 1:
        out.append(DistantLight(color=vec3(0.8, 0.3, 0.0), intensity=1.0, dir=normalize(vec(2.0, -0.8, -1.3))))
    return out


def stats(ms):
    ms = np.array(ms)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(ms.min()), 3),
            "ms_max": round(float(ms.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="c3,c5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rtmi import abi, scenes
    from rtmi._lib import lib, library_source_hash
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("relight_bench.py needs a GPU")
    makers = {"c3": ("C3 mesh-bunny (69,451 triangles + ground)", scenes.mesh_bunny),
              "c5": ("C5 torus (1,000,000 triangles + ground)", scenes.torus_scene)}
    hook = lib().rtmi_test_relight_passes
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    lines = []
    for key in args.scenes.split(","):
        name, make = makers[key]
        scene = make()
        for nl in (1, 2):
            scene.lights = lights_for(0, nl)
            ds = DeviceScene(scene)
            relight = []
            for k in range(args.warmup + args.repeats):
                ls = lights_for(k + 1, nl)
                t0 = time.perf_counter()
                ds.set_lights(ls)
                if k >= args.warmup:
                    relight.append((time.perf_counter() - t0) * 1e3)
            hook(ds.h, 1, None)
            passes = np.zeros((3, 6), np.float32)
            for k in range(3):
                ds.set_lights(lights_for(k + 50, nl))
                hook(ds.h, 1, passes[k].ctypes.data_as(C.POINTER(C.c_float)))
            ds.close()
            rebuild = {}
            for label, builder in (("sah", abi.RT_BVH_SAH), ("ploc", abi.RT_BVH_PLOC)):
                ds = DeviceScene(scene, bvh_builder=builder)
                ms = []
                for k in range(args.warmup + args.repeats):
                    scene.lights = lights_for(k + 1, nl)
                    t0 = time.perf_counter()
                    ds.close()
                    ds = DeviceScene(scene, bvh_builder=builder)
                    if k >= args.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                ds.close()
                rebuild[label] = stats(ms)
            out = {"tool": "relight_bench", "scene": name, "distant_lights": nl,
                   "library_source_hash": library_source_hash(), "device": torch.cuda.get_device_name(0),
                   "warmup": args.warmup, "repeats": args.repeats, "set_lights": stats(relight),
                   "destroy_create_sah": rebuild["sah"], "destroy_create_ploc": rebuild["ploc"],
                   "set_lights_device_passes_ms": {p: round(float(v), 3)
                                                   for p, v in zip(PASSES, np.median(passes, axis=0))}}
            out["relight_cheaper_than_both"] = bool(
                out["set_lights"]["ms_median"] < min(rebuild["sah"]["ms_median"], rebuild["ploc"]["ms_median"]))
            line = json.dumps(out)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
