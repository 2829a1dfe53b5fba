"""Registers, scratch, LDS and occupancy of the float64 feature-buffer kernels.

    python tools/aov64_resources.py [P ...]   # rewrites profiles/aov64/kernel_resources.txt

Compiles rt_kernels_aov64.hip for gfx950 with the Makefile's flags for it
(-ffp-contract=off) and records what the compiler reports for k_aov64_lane
and k_aov64_px<P>: one row per kernel, and a last line that says whether any
of them spills a VGPR or uses scratch. With arguments, k_aov64_px is compiled
for each of those batch sizes P as well (-DRTMI_AOV64_P): the rows the choice
of P in DESIGN.md rests on. The library's own P comes first.
"""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "nim-raytracer_amd")
OUT = os.path.join(REPO, "profiles", "aov64", "kernel_resources.txt")

KEYS = {"TotalSGPRs": "sgpr", "SGPRs Spill": "sspill", "VGPRs": "vgpr", "VGPRs Spill": "spill",
        "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ", "LDS Size [bytes/block]": "lds"}


def compile_unit(p=None):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "csrc/rt_kernels_aov64.hip", "-o",
           "/dev/null"] + ([f"-DRTMI_AOV64_P={p}"] if p else [])
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=PKG).stderr
    res, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            name = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
            fm = re.search(r"(k_aov64_lane|k_aov64_px<\d+>)", name)
            cur = fm.group(1) if fm else None
            if cur:
                res[cur] = {}
        elif cur and k in KEYS:
            res[cur][KEYS[k]] = int(v)
    return res


def main():
    rows = compile_unit()
    if len(rows) != 2:
        print(f"expected k_aov64_lane and k_aov64_px, found {sorted(rows)}", file=sys.stderr)
        return 1
    own = dict(rows)
    for p in sys.argv[1:]:
        for name, r in compile_unit(int(p)).items():
            rows.setdefault(name, r)
    lines = ["# rt_kernels_aov64.hip, gfx950, -ffp-contract=off (the Makefile's rule for it)",
             "# kernel            VGPRs  spilled  scratch B/lane  SGPRs  spilled  LDS B/block  waves/SIMD  blocks/CU by LDS"]
    for name, r in rows.items():
        by_lds = 163840 // r["lds"] if r["lds"] else 8
        note = "" if name in own else "   (not built: for comparison)"
        lines.append(f"{name:18s} {r['vgpr']:5d}  {r['spill']:7d}  {r['scratch']:14d}  {r['sgpr']:5d}  {r['sspill']:7d}  "
                     f"{r['lds']:11d}  {r['occ']:10d}  {min(by_lds, 8):16d}{note}")
    worst = max(max(r["scratch"], r["spill"]) for r in own.values())
    lines.append("# the library's kernels: "
                 + ("no instantiation spills a VGPR or uses scratch" if worst == 0 else "SPILLS OR SCRATCH IN USE"))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if worst == 0 else 2


if __name__ == "__main__":
    sys.exit(main())
