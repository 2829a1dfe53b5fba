#!/usr/bin/env python3
"""Host time per call of the query and feature-buffer entry points, paired
over library builds (RTMI_LIB): the C3 scene (bunny + ground), for every
family — trace, pick, shade and their float32 forms, the feature buffers of
both precisions — three lines:

  <family>.host.small    the host form on 64 rays / a 16 x 16 image
  <family>.device.small  the device form on the same: an overhead measurement
  <family>.device.full   the device form at the size its own bench tool
                         defaults to (2 M incoherent rays, 1920 x 1080 camera
                         rays or pixels)

and the bench.py lines C2 and C3. One process per library and run, the
libraries alternating (NAME=PATH pairs; the same path under two names gives
the build-against-itself spread). In a process each line is warmed up, then
timed over windows of back-to-back calls that each end in a device
synchronise; the line's figure is the median window's time per call.

    python tools/host_calls_bench.py --libs parent=tools/ab/parent.so,parent_again=tools/ab/parent.so,this= \\
        --runs 3 --out profiles/host_calls/parent_vs_this.jsonl

(an empty path is the in-tree librtmi.so). Needs a GPU. Appends one JSON
record per line, library and run to --out, in the record shape of
profiles/host_units/parent_vs_this.jsonl, and prints the per-line medians.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nim-raytracer_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def windows(torch, call, warmup, nwin, per):
    """ms per call of `nwin` windows of `per` calls, each ended by a device synchronise."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        t0 = time.perf_counter()
        for _ in range(per):
            call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / per)
    return out


def child(args):
    import torch
    from query_bench import incoherent_rays
    from rtmi import Antialias, Options, Precision, akGrid, akNone, scenes
    from rtmi.renderer import DeviceScene

    scene = scenes.mesh_bunny()
    ds = DeviceScene(scene)
    W, H = 1920, 1080
    full = {"rays": incoherent_rays(scene, 2_000_000, 7), "shade": incoherent_rays(scene, W * H, 8)}
    small = incoherent_rays(scene, 64, 9)
    xy_small = np.random.default_rng(3).uniform(0.0, 16.0, (64, 2))
    yy, xx = np.mgrid[0:H, 0:W]
    xy_full = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)

    def both(a):
        return a, a.astype(np.float32)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def o(w, h, prec, aa=None):
        return Options(width=w, height=h, antialias=aa or Antialias(akNone, 1), bias=1e-4, precision=prec)

    g4 = Antialias(akGrid, 4)
    lines = {}  # name -> (call, calls per window)
    for size, (ro, rd), xy, (w, h), per in (("small", small, xy_small, (16, 16), 200),
                                            ("full", full["rays"], xy_full, (W, H), 2)):
        (o64, o32), (d64, d32), (p64, p32) = both(ro), both(rd), both(xy)
        so, sd = (ro, rd) if size == "small" else full["shade"]
        (s64o, s32o), (s64d, s32d) = both(so), both(sd)
        o_64, o_32 = o(w, h, Precision.fp64), o(w, h, Precision.fp32)
        forms = [("device", dev)] + ([("host", np.ascontiguousarray)] if size == "small" else [])
        for form, put in forms:
            a = {k: put(v) for k, v in dict(o64=o64, d64=d64, o32=o32, d32=d32, p64=p64, p32=p32, s64o=s64o,
                                            s64d=s64d, s32o=s32o, s32d=s32d).items()}
            host = form == "host"
            cases = {
                "trace": lambda a=a: ds.trace_rays(a["o64"], a["d64"]),
                "pick": lambda a=a, q=o_64: ds.pick(q, a["p64"]),
                "shade": lambda a=a, q=o_64: ds.shade_rays(q, a["s64o"], a["s64d"], f32=True),
                "trace32": lambda a=a: ds.trace_rays_f32(a["o32"], a["d32"]),
                "pick32": lambda a=a, q=o_32: ds.pick_f32(q, a["p32"]),
                "shade32": lambda a=a, q=o_32: ds.shade_rays_f32(q, a["s32o"], a["s32d"]),
                "aov": lambda q=o(w, h, Precision.fp32, g4), host=host: ds.render_aovs(q, host=host),
                "aov64": lambda q=o(w, h, Precision.fp64, g4), host=host: ds.render_aovs_f64(q, host=host),
            }
            for fam, call in cases.items():
                lines[f"{fam}.{form}.{size}"] = (call, per)
    torch.cuda.synchronize()
    for name, (call, per) in lines.items():
        ms = windows(torch, call, 3, args.windows, per)
        print(json.dumps({"config": name, "ms_per_step": round(statistics.median(ms), 5),
                          "windows_ms": [round(v, 5) for v in ms]}), flush=True)


def bench_line(env, cfg, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", cfg, "--steps",
                        str(steps), "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"bench.py {cfg} failed ({r.returncode}): {r.stderr[-400:]}")
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return {"config": cfg, "ms_per_step": d.get("ms_per_step"), "value": d.get("value"), "unit": d.get("unit")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--libs", default="this=")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--visit", default="first")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "host_calls", "parent_vs_this.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = [kv.split("=", 1) for kv in args.libs.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    seen = {}
    with open(args.out, "a") as out:
        for run in range(1, args.runs + 1):
            for name, path in libs:
                env = dict(os.environ)
                env.pop("RTMI_LIB", None)
                if path:
                    env["RTMI_LIB"] = os.path.abspath(path)
                # a fresh process per library and run; a failure ends the job: nothing more is started
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--windows",
                                    str(args.windows)], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"{name} run {run} failed ({r.returncode}): {r.stderr[-600:]}")
                recs = [dict(json.loads(ln), tool="tools/host_calls_bench.py")
                        for ln in r.stdout.splitlines() if ln.startswith("{")]
                recs += [dict(bench_line(env, c, args.bench_steps, args.bench_warmup), tool="bench.py")
                         for c in ("C2", "C3")]
                for rec in recs:
                    rec = {"tool": rec.pop("tool"), "visit": args.visit, "config": rec.pop("config"), "library": name,
                           "run": run, **rec}
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                    seen.setdefault(rec["config"], {}).setdefault(name, []).append(rec["ms_per_step"])
                print(f"run {run} {name}: {len(recs)} lines", flush=True)
    for cfg, by in seen.items():
        print(f"{cfg:24s} " + "  ".join(f"{n} {statistics.median(v):.5f}" for n, v in by.items()), flush=True)


if __name__ == "__main__":
    main()
