#!/usr/bin/env python3
"""What it costs to move an object: rt_scene_set_objects against the only way
there was before it, rt_scene_destroy + rt_scene_create (the host SAH builder,
the drop-in cache's path). Two scenes — C3 (bunny.geom baked x30 + ground: the
bunny slides along the ground every step) and C2 (boxes2, 16 primitives: one
box moves every step).

Each case: `--warmup` untimed runs, then `--repeats` runs timed one by one on
the host clock (both are synchronous calls: they return when the scene is
ready), the median and the spread reported. For C2 the object light grids'
pass alone is reported too, by the device builder (rt_objgrid_gpu.hip) and by
the host builder (rtmi_test_objgrid_pass switches between them). Needs a GPU;
prints one JSON line per case and, with --out, appends them to a file.

    python tools/object_update_bench.py --out profiles/objects/object_update_bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))


def stats(ms):
    ms = np.array(ms)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
            "ms_max": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rebuild-repeats", type=int, default=5)
    ap.add_argument("--scenes", default="c3,c2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rtmi import scenes
    from rtmi._lib import lib, library_source_hash
    from rtmi.glm import inverse, translate, vec3
    from rtmi.renderer import DeviceScene

    if not torch.cuda.is_available():
        sys.exit("object_update_bench.py needs a GPU")
    makers = {"c3": ("C3 mesh-bunny (69,451 triangles + ground), the bunny slides", scenes.mesh_bunny, "bunny"),
              "c2": ("C2 boxes2 (16 primitives), one box moves", scenes.boxes2, "box3")}
    hook = lib().rtmi_test_objgrid_pass
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    lines = []
    for key in args.scenes.split(","):
        name, make, moved = makers[key]
        scene = make()
        ob = next(o for o in scene.objects if o.name == moved)
        home = ob.geometry.objectToWorld

        def step(k):
            ob.geometry.objectToWorld = translate(home, vec3(0.02 * (k % 50), 0.0, 0.01 * (k % 50)))
            ob.geometry.worldToObject = inverse(ob.geometry.objectToWorld)

        ds = DeviceScene(scene)
        grid = {}
        update = {}
        for label, host in (("device", 0), ("host", 1)):
            hook(ds.h, host, None)
            ms, gms = [], []
            for k in range(args.warmup + args.repeats):
                step(k + 1)
                t0 = time.perf_counter()
                ds.set_objects()
                dt = (time.perf_counter() - t0) * 1e3
                g = C.c_double()
                hook(ds.h, -1, C.byref(g))
                if k >= args.warmup:
                    ms.append(dt)
                    gms.append(g.value)
            update[label] = stats(ms)
            grid[label] = stats(gms)
        hook(ds.h, 0, None)
        ms = []
        for k in range(1 + args.rebuild_repeats):
            step(k + 1)
            t0 = time.perf_counter()
            ds.close()
            ds = DeviceScene(scene)
            if k >= 1:
                ms.append((time.perf_counter() - t0) * 1e3)
        ds.close()
        out = {"tool": "object_update_bench", "scene": name, "library_source_hash": library_source_hash(),
               "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
               "set_objects": update["device"], "set_objects_host_object_grids": update["host"],
               "destroy_create_sah": stats(ms), "rebuild_repeats": args.rebuild_repeats}
        if key == "c2":
            out["object_grid_pass_device"] = grid["device"]
            out["object_grid_pass_host"] = grid["host"]
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
