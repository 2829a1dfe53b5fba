"""The inputs of test_gpu_trace32.py leave its criteria room: on the oracle
alone (no GPU), for each of the 16 geometry subset scenes, the 24,576 akGrid
m = 2 camera rays rounded to float32, and the same with every direction
component further moved by a seeded relative 2^-20, hit the same (object,
face) as the float64 rays on all but at most 0.02 % of the rays. The GPU
file's 99.9 % cap on (obj, face) agreement is therefore the float32
arithmetic's to use, not the inputs'."""
import numpy as np
import pytest

import trace32_cases as t32

CAP = 0.0002


@pytest.mark.parametrize("bits", t32.GEOMETRY_BITS)
def test_float32_rays_hit_what_the_float64_rays_hit(oracle_mod, bits):
    o64, d64 = t32.frame_rays64(oracle_mod)
    o32, d32 = t32.frame_rays(oracle_mod)
    n = len(o64)
    obj, face, t = t32.oracle_trace(oracle_mod, bits, o64, d64)
    assert (obj >= 0).sum() >= n // 10 and (obj < 0).sum() >= n // 10   # neither all hits nor all misses
    robj, rface, rt = t32.oracle_trace(oracle_mod, bits, o32, d32)
    pobj, pface, pt = t32.oracle_trace(oracle_mod, bits, o32, t32.perturbed_dirs(oracle_mod))
    differ_r = int(((robj != obj) | (rface != face)).sum())
    differ_p = int(((pobj != obj) | (pface != face)).sum())
    both = (pobj == robj) & (pface == rface) & (robj >= 0)
    rel = np.abs(pt[both] - rt[both]) / np.maximum(1.0, rt[both])
    print(f"subset {bits}: {differ_r} / {differ_p} of {n} rays differ after rounding / perturbing; "
          f"largest relative change of t under the perturbation {rel.max():.3g}")
    assert differ_r <= CAP * n and differ_p <= CAP * n, (bits, differ_r, differ_p)
