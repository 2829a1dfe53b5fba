"""Record the multiprecision truth of the radiance-query rays
(tests/shade_cases.py truth_rays: 96 rays with unnormalised directions on
subsets 35 and 63, which the oracle's camera cannot form):

    python tests/golden/make_truth_shade.py

writes truth_shade_35.npz and truth_shade_63.npz: the rays, per ray the colour
of truth._trace + truth.shade rounded to float64, its Counts, the primary
hit's object, both margins and the float32 query margins. It refuses to write a fixture with more than
2 % undecided rays, or one whose rays do not both hit and miss, or spawn no
reflection rays."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "nim-raytracer_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import shade_cases as sc  # noqa: E402
import truth  # noqa: E402
import truth_cases as tc  # noqa: E402


def main():
    t0 = time.time()
    for bits in sc.TRUTH_BITS:
        f = sc.truth_shade(bits)
        und = float((f["margin"] < truth.EPS).mean())
        hit = int((f["obj"] >= 0).sum())
        refl = int(f["counts"][:, 4].sum())
        assert und <= tc.UNDECIDED_CAP, (bits, und)
        assert 0 < hit < sc.N_TRUTH and refl > 0, (bits, hit, refl)
        np.savez_compressed(os.path.join(HERE, f"truth_shade_{bits}.npz"), **f)
        print(f"shade {bits}: {und:.3f} undecided, {hit} of {sc.N_TRUTH} rays hit, {refl} reflection rays, "
              f"{time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
