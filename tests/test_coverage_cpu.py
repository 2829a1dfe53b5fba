"""The exact-count scenes of coverage_scenes.py, on the CPU: the float64 model
of which samples hit (classify) against the oracle's frames, the room the
scenes leave test_gpu_coverage.py, and proof that wrong sample tables would
leave the bounds.

For every (scene, kind, m, seed) the GPU file renders in float32 up to
m = 32, and one case at m = 64: the oracle's channels are equal, value * spp
is within 0.05 of an integer, and that hit count lies in the model's
[k_lo, k_hi]. Then, from the oracle alone: at most 1 % of the samples are
undecided, at least 40 % of the pixels have k_lo == k_hi (m <= 32), at least
25 % (slat scenes) or 8 % (block scenes) of the pixels are partly covered
(m >= 2), and empty and full pixels both exist.

The mutants are numpy-made sample tables a subtly wrong kernel could build:
the last sample a copy of sample 0, sy paired one entry off, and the
correlated multi-jittered y shuffle drawing from the multi-jittered base.
Each leaves [k_lo, k_hi] of the true table on at least 20 pixels, so the GPU
file fails on such a kernel."""
import numpy as np
import pytest

import coverage_scenes as cs
from rtmi import akGrid
from rtmi.scene import akCorrelatedMultiJittered

CASES = sorted({c for c in cs.fp32_samplings() if c[2] <= 32} | {c for c in cs.FP64_SAMPLINGS if c[2] <= 64},
               key=lambda c: (c[0], int(c[1]), c[2], c[3]))
SLAT_SCENES = ("slats", "slats_mirror", "slats_ground")


@pytest.mark.parametrize("name,kind,m,seed", CASES, ids=[cs.case_id(*c) for c in CASES])
def test_oracle_counts_lie_in_the_model_bounds(oracle_mod, name, kind, m, seed):
    spp = cs.spp_of(kind, m)
    frame, st = cs.oracle_frame(name, kind, m, seed)
    assert st.numPrimaryRays == cs.W * cs.H * spp
    hits, off = cs.hit_counts(name, frame, spp)  # asserts equal channels
    assert off.max() <= 0.05, off.max()
    k_lo, k_hi = cs.bounds(name, kind, m, seed)
    bad = (hits < k_lo) | (hits > k_hi)
    assert not bad.any(), [(int(x), int(y), int(hits[y, x]), int(k_lo[y, x]), int(k_hi[y, x]))
                           for y, x in np.argwhere(bad)[:8]]
    # the room the case leaves the GPU file
    assert cs.undecided_share(name, kind, m, seed) <= 0.01
    if m <= 32:
        assert (k_lo == k_hi).mean() >= 0.40
    if m >= 2:
        partial = ((hits > 0) & (hits < spp)).mean()
        assert partial >= (0.25 if name in SLAT_SCENES else 0.08), partial
    assert (hits == 0).any() and (hits == spp).any()


def test_the_big_grids_leave_room():
    """The cases without an oracle frame (m >= 100): the 1 % cap, from the model."""
    for name, kind, m, seed in cs.fp32_samplings():
        if m == cs.M_BOUNDS_ONLY:  # 255 and 256 cost seconds each and are checked where they run, on the GPU
            assert cs.undecided_share(name, kind, m, seed) <= 0.01, (name, int(kind), m)


# ---- mutants ----------------------------------------------------------------

def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _draws(seed, x, y, k):
    """The oracle's draw_u(pixel_key(seed, x, y), k) for an array of draw indices."""
    key = _mix64(np.uint64(seed) ^ _mix64(np.uint64((y << 32) | x)))
    with np.errstate(over="ignore"):
        z = key + (np.asarray(k, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return (_mix64(z) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def cmj_table(m, seed, x, y, by_of_kind3=False):
    """correlatedMultiJittered (sampling.nim:79-113) with the oracle's draws,
    restated in numpy; by_of_kind3: the y shuffle's draws start where the
    multi-jittered sampler's do (after m * m x draws, not m)."""
    xs = 1.0 / m
    e = np.arange(m * m)
    j, i = e // m, e % m
    sx = ((i + (j + _draws(seed, x, y, 2 * e)) * xs) * xs).reshape(m, m)
    sy = ((j + (i + _draws(seed, x, y, 2 * e + 1)) * xs) * xs).reshape(m, m)
    bx = 2 * m * m
    by = bx + (m * m if by_of_kind3 else m)
    ux, uy = _draws(seed, x, y, bx + np.arange(m)), _draws(seed, x, y, by + np.arange(m))
    for r in range(m):
        k = r + int(ux[r] * (m - r))
        sx[[r, k]] = sx[[k, r]]
    for c in range(m):
        k = c + int(uy[c] * (m - c))
        sy[:, [c, k]] = sy[:, [k, c]]
    return sx.reshape(-1), sy.reshape(-1)


def test_numpy_cmj_table_is_the_oracles(oracle_mod):
    for m, seed, x, y in ((3, cs.SEEDS[0], 0, 0), (8, cs.SEEDS[1], 32, 18), (32, cs.SEEDS[0], 7, 11)):
        sx, sy = cmj_table(m, seed, x, y)
        ox, oy = oracle_mod.sample_table(akCorrelatedMultiJittered, m, seed, x, y)
        assert np.array_equal(sx, ox) and np.array_equal(sy, oy), (m, x, y)


def _last_is_first(kind, m, seed, x, y):
    sx, sy = (a.copy() for a in cs.pixel_offsets(kind, m, seed, x, y))
    sx[-1], sy[-1] = sx[0], sy[0]
    return sx, sy


def _sy_rolled(kind, m, seed, x, y):
    sx, sy = cs.pixel_offsets(kind, m, seed, x, y)
    return sx, np.roll(sy, 1)


def _by_of_kind3(kind, m, seed, x, y):
    return cmj_table(m, seed, x, y, by_of_kind3=True)


MUTANTS = [(mut, kind) for mut, kinds in ((_last_is_first, (akGrid,) + cs.STOCHASTIC), (_sy_rolled, cs.STOCHASTIC),
                                          (_by_of_kind3, (akCorrelatedMultiJittered,))) for kind in kinds]


# blocks has about 90 partly covered pixels, and one sample of 1024 moved or re-paired changes
# a pixel's count on fewer than half of them (9 to 27 found): the bar of 20 pixels is asked of
# blocks at m = 3 and 8, and of slats, which every sampler of the GPU file renders, at all three
MUTANT_SCENES = [("slats", 3), ("slats", 8), ("slats", 32), ("blocks", 3), ("blocks", 8)]


@pytest.mark.parametrize("mutant,kind", MUTANTS, ids=[f"{f.__name__[1:]}-k{int(k)}" for f, k in MUTANTS])
@pytest.mark.parametrize("name,m", MUTANT_SCENES)
def test_mutant_tables_leave_the_bounds(oracle_mod, name, mutant, kind, m):
    """A kernel that built this table would produce a count in the mutant's
    own [lo, hi]; where that interval lies wholly outside the true table's,
    the GPU file fails whatever the kernel's rounding."""
    seed = cs.SEEDS[m % 2]
    k_lo, k_hi = cs.bounds(name, kind, m, seed)
    lo, hi = cs.table_bounds(name, kind, m, seed, mutant)
    caught = int(np.count_nonzero((hi < k_lo) | (lo > k_hi)))
    print(name, mutant.__name__, int(kind), m, "caught on", caught, "pixels")
    assert caught >= 20, caught


# ---- div_small --------------------------------------------------------------

def test_div_small_formula_is_exact():
    """rt_fast_core.h div_small: q = int((float(n) + 0.5f) * float(1 / dv)),
    restated in float32 numpy and compared with n // dv for every n < 2^21
    and dv in 1..256. This checks the formula; the akGrid cases of
    test_gpu_coverage.py at m = 3 ... 255 check the code (a wrong quotient
    moves a sample to another row and column)."""
    n = np.arange(1 << 21, dtype=np.int32)
    nf = n.astype(np.float32) + np.float32(0.5)
    for dv in range(1, 257):
        q = (nf * np.float32(1.0 / dv)).astype(np.int32)
        assert np.array_equal(q, n // dv), dv
