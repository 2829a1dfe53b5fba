#!/usr/bin/env python3
"""What it costs to move a mesh's vertices: rt_scene_set_mesh_vertices_device
against the only way there was before it, rt_scene_destroy + rt_scene_create,
with the host SAH builder and with the device PLOC builder. Two scenes — C3
(bunny.geom baked x30 + ground, 69,451 triangles) and C5 (the 1M-triangle
torus) — deformed by a twist about y whose angle changes every run, computed
by torch on the GPU and handed over as a CUDA tensor.

Each case: `--warmup` untimed runs, then `--repeats` runs timed one by one on
the host clock (all three are synchronous calls: they return when the scene
is ready), the median and the spread reported. After the timed runs the
update's passes are timed in runs of their own, the stream waited for after
each pass (rtmi_test_mesh_update_passes). Last, at the largest twist, the
float32 headline frame (1920x1080, 256 spp) and a float64 frame (480x270,
4 spp) on the refitted tree against the same frames on a tree built for the
twisted mesh: the price of keeping the topology. Needs a GPU; prints one JSON
line per scene and, with --out, appends them to a file.

    python tools/mesh_update_bench.py --out profiles/mesh_update/mesh_update_bench.jsonl
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

PASSES = ("copy_in", "bounds", "buffer_copies", "records_normals", "refit_bins_boxes", "lights")


def stats(ms):
    ms = np.array(ms)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(ms.min()), 3),
            "ms_max": round(float(ms.max()), 3)}


def angle(k):
    return 0.01 * (k + 1)  # radians per unit of height; the meshes are 5 to 8 units tall


def twist_host(v, a):
    t = a * v[:, 1]
    out = v.copy()
    out[:, 0] = np.cos(t) * v[:, 0] + np.sin(t) * v[:, 2]
    out[:, 2] = -np.sin(t) * v[:, 0] + np.cos(t) * v[:, 2]
    return out


def twist_device(torch, d_v, a):
    t = a * d_v[:, 1]
    c, s = torch.cos(t), torch.sin(t)
    return torch.stack([c * d_v[:, 0] + s * d_v[:, 2], d_v[:, 1], -s * d_v[:, 0] + c * d_v[:, 2]], dim=1).contiguous()


def frame_ms(torch, ds, opts, runs=7):
    fb = torch.zeros(opts.width * opts.height * 3, dtype=torch.float32, device="cuda")
    ms = []
    for k in range(runs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.render_device(opts, fb)
        if k >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="c3,c5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rtmi import Antialias, Options, Precision, abi, akGrid, scenes
    from rtmi._lib import lib, library_source_hash
    from rtmi.renderer import DeviceScene
    from rtmi.scene import TriangleMesh

    if not torch.cuda.is_available():
        sys.exit("mesh_update_bench.py needs a GPU")
    makers = {"c3": ("C3 mesh-bunny (69,451 triangles + ground)", scenes.mesh_bunny),
              "c5": ("C5 torus (1,000,000 triangles + ground)", scenes.torus_scene)}
    hook = lib().rtmi_test_mesh_update_passes
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    o32 = Options(width=1920, height=1080, antialias=Antialias(akGrid, 16), bias=1e-4, precision=Precision.fp32)
    o64 = Options(width=480, height=270, antialias=Antialias(akGrid, 2), bias=1e-4, precision=Precision.fp64)
    lines = []
    n_runs = args.warmup + args.repeats
    for key in args.scenes.split(","):
        name, make = makers[key]
        scene = make()
        mesh = next(o.geometry for o in scene.objects if isinstance(o.geometry, TriangleMesh))
        rest = mesh.vertices.copy()
        d_rest = torch.from_numpy(rest).cuda()
        ds = DeviceScene(scene)
        update = []
        for k in range(n_runs):
            d_v = twist_device(torch, d_rest, angle(k))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds.set_mesh_vertices(0, d_v)
            if k >= args.warmup:
                update.append((time.perf_counter() - t0) * 1e3)
        hook(ds.h, 1, None)
        passes = np.zeros((3, 6), np.float32)
        for k in range(3):
            ds.set_mesh_vertices(0, twist_device(torch, d_rest, angle(n_runs - 3 + k)))
            hook(ds.h, 1, passes[k].ctypes.data_as(C.POINTER(C.c_float)))
        hook(ds.h, 0, None)
        # the refitted tree at the largest twist, against trees built for that mesh
        frames = {"refit": {"fp32_1920x1080_256spp": frame_ms(torch, ds, o32), "fp64_480x270_4spp": frame_ms(torch, ds, o64)}}
        ds.close()
        rebuild = {}
        for label, builder in (("sah", abi.RT_BVH_SAH), ("ploc", abi.RT_BVH_PLOC)):
            ds = DeviceScene(scene, bvh_builder=builder)
            ms = []
            for k in range(n_runs):
                mesh.vertices = np.ascontiguousarray(twist_host(rest, angle(k)))
                t0 = time.perf_counter()
                ds.close()
                ds = DeviceScene(scene, bvh_builder=builder)
                if k >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            rebuild[label] = stats(ms)
            frames["fresh_" + label] = {"fp32_1920x1080_256spp": frame_ms(torch, ds, o32),
                                        "fp64_480x270_4spp": frame_ms(torch, ds, o64)}
            ds.close()
        mesh.vertices = rest
        out = {"tool": "mesh_update_bench", "scene": name, "library_source_hash": library_source_hash(),
               "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
               "twist_rad_per_unit_height": [angle(args.warmup), angle(n_runs - 1)],
               "set_mesh_vertices_device": stats(update),
               "destroy_create_sah": rebuild["sah"], "destroy_create_ploc": rebuild["ploc"],
               "update_passes_ms": {p: round(float(v), 3) for p, v in zip(PASSES, np.median(passes, axis=0))},
               "frame_ms_at_largest_twist": frames}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
