"""Registers, scratch and occupancy of every k_trace_rays_f32 instantiation.

    python tools/trace32_resources.py    # rewrites profiles/trace32/kernel_resources.txt

Compiles the two objects of rt_kernels_f32_part.hip that hold the 16 geometry
subsets (parts 0 and 1) with the Makefile's float32 flags (the occupancy table
of rt_occupancy.h in effect) and records what the compiler reports for the
float32 ray-query kernel (rt_fast_query.h): one row per subset, and a last
line that says whether any of them spills a VGPR or uses scratch.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nim-raytracer_amd")
OUT = os.path.join(REPO, "profiles", "trace32", "kernel_resources.txt")
sys.path.insert(0, os.path.join(REPO, "tools"))
from occupancy_table import subset_index  # noqa: E402

KEYS = {"TotalSGPRs": "sgpr", "SGPRs Spill": "sspill", "VGPRs": "vgpr", "VGPRs Spill": "spill", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occ", "LDS Size [bytes/block]": "lds"}
NAMES = ("sphere", "box", "mesh", "general")


def compile_part(part):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Xclang",
           "-target-feature", "-Xclang", "-packed-fp32-ops", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "csrc/rt_kernels_f32_part.hip", "-o",
           "/dev/null", f"-DRTMI_PART={part}"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=PKG).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            name = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
            fm = re.search(r"k_trace_rays_f32<(\d+)u>", name)
            cur = subset_index(int(fm.group(1))) if fm else None
            if cur is not None:
                res[cur] = {}
        elif cur is not None and k in KEYS:
            res[cur][KEYS[k]] = int(v)
    return res


def main():
    with ThreadPoolExecutor(max_workers=2) as ex:
        rows = {}
        for r in ex.map(compile_part, range(2)):
            rows.update(r)
    if sorted(rows) != list(range(16)):
        print(f"expected 16 instantiations, found {len(rows)}", file=sys.stderr)
        return 1
    lines = ["# k_trace_rays_f32<F>, gfx950, the Makefile's float32 flags: per geometry subset (rt_common.h SUB_* bits 0..3)",
             "# subset  features                     VGPRs  spilled  scratch B/lane  SGPRs  spilled  LDS B/block  waves/SIMD"]
    for i in range(16):
        r = rows[i]
        feat = "+".join(n for k, n in enumerate(NAMES) if i >> k & 1) or "plane"
        lines.append(f"{i:8d}  {feat:28s} {r['vgpr']:5d}  {r['spill']:7d}  {r['scratch']:14d}  {r['sgpr']:5d}  "
                     f"{r['sspill']:7d}  {r['lds']:11d}  {r['occ']:10d}")
    worst = max(max(r["scratch"], r["spill"]) for r in rows.values())
    lines.append(f"# VGPRs {min(r['vgpr'] for r in rows.values())}..{max(r['vgpr'] for r in rows.values())}, "
                 f"waves/SIMD {min(r['occ'] for r in rows.values())}..{max(r['occ'] for r in rows.values())}, "
                 f"largest scratch {max(r['scratch'] for r in rows.values())} B/lane: "
                 + ("no instantiation spills a VGPR or uses scratch" if worst == 0 else "SPILLS OR SCRATCH IN USE"))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 0 if worst == 0 else 2


if __name__ == "__main__":
    sys.exit(main())
