"""Registers, scratch and occupancy of every k_render_aov instantiation.

    python tools/aov_resources.py    # rewrites profiles/aov/kernel_resources.txt

Compiles the four objects of rt_kernels_f32_part.hip that hold the 16 geometry
subsets without and with stochastic sampling (parts 0, 1, 8 and 9) with the
Makefile's float32 flags and records what the compiler reports for the
feature-buffer kernel (rt_fast_aov.h): one row per subset, and a last line
that says whether any of them spills a VGPR or uses scratch.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nim-raytracer_amd")
OUT = os.path.join(REPO, "profiles", "aov", "kernel_resources.txt")
sys.path.insert(0, os.path.join(REPO, "tools"))
from occupancy_table import subset_index  # noqa: E402

KEYS = {"TotalSGPRs": "sgpr", "SGPRs Spill": "sspill", "VGPRs": "vgpr", "VGPRs Spill": "spill", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occ", "LDS Size [bytes/block]": "lds"}
NAMES = ("sphere", "box", "mesh", "general", "", "", "stochastic")


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
            fm = re.search(r"k_render_aov<(\d+)u>", name)
            cur = subset_index(int(fm.group(1))) if fm else None
            if cur is not None:
                res[cur] = {}
        elif cur is not None and k in KEYS:
            res[cur][KEYS[k]] = int(v)
    return res


def main():
    subsets = list(range(16)) + list(range(64, 80))
    with ThreadPoolExecutor(max_workers=4) as ex:
        rows = {}
        for r in ex.map(compile_part, (0, 1, 8, 9)):
            rows.update(r)
    if sorted(rows) != subsets:
        print(f"expected 32 instantiations, found {len(rows)}", file=sys.stderr)
        return 1
    lines = ["# k_render_aov<F>, gfx950, the Makefile's float32 flags: per subset (rt_common.h SUB_* bits 0..3 and 6)",
             "# subset  features                           VGPRs  spilled  scratch B/lane  SGPRs  spilled  LDS B/block  waves/SIMD"]
    for i in subsets:
        r = rows[i]
        feat = "+".join(n for k, n in enumerate(NAMES) if n and i >> k & 1) or "plane"
        lines.append(f"{i:8d}  {feat:34s} {r['vgpr']:5d}  {r['spill']:7d}  {r['scratch']:14d}  {r['sgpr']:5d}  "
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
