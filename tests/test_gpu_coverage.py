"""Where the kernels put their samples, pinned by integer coverage counts.

The colour tolerances of the other parity files pass a pixel whose samples
all agree wherever the samples lie inside it, and let 0.5 % of a frame's
pixels be wrong; so they do not pin where a float32 kernel puts a sample, or
which sx it pairs with which sy. The scenes of coverage_scenes.py do: black
objects under a sky of 1, so a float32 pixel is exactly (samples that miss)
/ spp whatever the lane order and the reduction, and the number of samples
that hit must lie in the float64 model's [k_lo, k_hi], whose two ends differ
only by the samples within DELTA = 1e-3 pixel of an edge
(test_coverage_cpu.py: model and oracle agree, most pixels have k_lo == k_hi,
and a table with one sample duplicated, with sy one entry off, or with the
wrong draw base for the correlated sampler leaves the bounds on 50 to 260
pixels of slats).

float32, every case: equal channels, value * spp within 0.05 of an integer,
that integer inside [k_lo, k_hi], numPrimaryRays == w * h * spp.
  * slats, blocks: the three stochastic kinds at m = 1 ... 32 (1, 4, 8, 16,
    32 and 64 lanes per pixel; 16-lane object batches on blocks at m = 8, 9,
    11), two seeds, default and plain flags; akGrid at m that are no power of
    two (div_small) up to 255 and at 256; akJittered above the table kinds'
    limit (33, 100, 256); akNone.
  * blocks2 (no object grid), slats_mirror (the reflective level loop, and
    k_render_wave with RT_FLAG_COMPACT), slats_ground (the one-plane kernels
    at m = 16 and 32, the general two-class kernels at m = 8).
  * rows 5..14 alone, and three ranks' bands.
float64: frames and Stats equal the oracle's bit for bit at m = 5, and at
m = 64 and 256, where fill_params' scratch cap cuts the launch to 16 blocks
and to one.
Limits: the table kinds stop at m = 32 in float32 only; grid_size 257 is
invalid.

RTMI_COVERAGE_LOG=<file> appends one row per float32 case: how many pixels
differ from the oracle's own count (profiles/coverage/fp32_counts.jsonl)."""
import json
import os

import numpy as np
import pytest

import coverage_scenes as cs
from rtmi import Precision, akGrid, akNone
from rtmi._lib import RtmiError
from rtmi.abi import (RT_E_INVALID, RT_E_UNSUPPORTED, RT_FLAG_COMPACT, RT_FLAG_NO_BINNING, RT_FLAG_NO_OBJ_BATCH,
                      RT_FLAG_NO_REORDER, RT_FLAG_NO_SPLIT)
from rtmi.dist import band_rows, rank_rows
from rtmi.renderer import DeviceScene
from rtmi.scene import akCorrelatedMultiJittered, akMultiJittered

pytestmark = pytest.mark.gpu

PLAIN = RT_FLAG_NO_BINNING | RT_FLAG_NO_SPLIT | RT_FLAG_NO_OBJ_BATCH | RT_FLAG_NO_REORDER  # test_gpu_subsets.py's
FLAGS = {"default": 0, "plain": PLAIN, "compact": RT_FLAG_COMPACT}
STOCHASTIC_BIT = 64  # rt_common.h SUB_STOCHASTIC
SEEN = {}            # scene -> (f32_subset value, the kind was stochastic) of every float32 case run

CASES = [c + (fl,) for c in cs.fp32_samplings()
         for fl in (("default", "compact") if c[0] == "slats_mirror" else ("default", "plain"))]

_SCENES = {}


def _ds(name):
    """One DeviceScene per scene for the whole module."""
    if name not in _SCENES:
        _SCENES[name] = DeviceScene(cs.scene(name))
    return _SCENES[name]


def _render(ds, o, **kw):
    import torch
    fb = torch.zeros(o.height * o.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(o, fb, **kw)
    return fb.view(o.height, o.width, 3).cpu().numpy(), st


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("RTMI_COVERAGE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _check_counts(name, kind, m, seed, frame, what, rows=None):
    """The hit counts of `frame` (its `rows`, default all) obey the model's
    bounds; returns them. A violation is reported with the exclusion distance
    that would explain it (coverage_scenes.edge_distance)."""
    spp = cs.spp_of(kind, m)
    hits, off = cs.hit_counts(name, frame, spp)
    k_lo, k_hi = cs.bounds(name, kind, m, seed)
    sel = np.zeros((cs.H, cs.W), bool)
    sel[slice(None) if rows is None else rows] = True
    assert off[sel].max() <= 0.05, (what, float(off[sel].max()))
    bad = sel & ((hits < k_lo) | (hits > k_hi))
    out = [{"x": int(x), "y": int(y), "got": int(hits[y, x]), "k_lo": int(k_lo[y, x]), "k_hi": int(k_hi[y, x]),
            "edge_distance": cs.edge_distance(name, kind, m, seed, int(x), int(y), int(hits[y, x]))}
           for y, x in np.argwhere(bad)[:16]]
    row = {"case": what, "spp": spp, "outside_bounds": int(bad.sum()), "outside": out,
           "undecided_share": round(cs.undecided_share(name, kind, m, seed), 6),
           "exact_pixels": int((k_lo == k_hi)[sel].sum())}
    if m < cs.M_BOUNDS_ONLY and rows is None:
        ref, _ = cs.oracle_frame(name, kind, m, seed)
        ohits, _ = cs.hit_counts(name, ref, spp)
        diff = hits != ohits
        row["differs_from_oracle"] = int(diff.sum())
        row["differing"] = [[int(x), int(y), int(hits[y, x]), int(ohits[y, x])] for y, x in np.argwhere(diff)[:16]]
    _log(row)
    assert not bad.any(), row
    return hits


@pytest.mark.parametrize("name,kind,m,seed,flags", CASES, ids=[cs.case_id(*c) for c in CASES])
def test_fp32_counts(gpu, oracle_mod, name, kind, m, seed, flags):
    ds = _ds(name)
    o = cs.options(kind, m, seed, Precision.fp32, FLAGS[flags])
    sub = ds.f32_subset(o)
    SEEN.setdefault(name, set()).add((sub, kind in cs.STOCHASTIC))
    frame, st = _render(ds, o)
    spp = cs.spp_of(kind, m)
    assert st.numPrimaryRays == cs.W * cs.H * spp, st
    _check_counts(name, kind, m, seed, frame, cs.case_id(name, kind, m, seed, flags))
    if m >= cs.M_BOUNDS_ONLY:
        assert cs.undecided_share(name, kind, m, seed) <= 0.01
    assert ds.last_compacted() == (flags == "compact")
    if flags != "default":
        return
    # the kernels the default dispatch is meant to reach with this case
    k = ds.last_lean_kernel()
    lean, general = ds.last_split()
    if name == "slats_ground" and kind == akGrid:
        # the one-plane shape (rt_render.cpp lean1_ok): k_render_lean1q, or both lists merged in k_render_mix1
        assert k & 3 in (2, 3), (k, lean, general)
        assert lean > 0 and general > 0, (lean, general)
    elif name in ("slats", "slats_ground") and spp >= 64:
        # one pixel per wave: the two-class launch, k_render_lean<F> and k_render_gen<F>
        assert k & 3 and k >> 2 & 3, (k, lean, general)
        assert lean > 0 and general > 0 and lean + general == cs.W * cs.H, (lean, general)


def test_hook_saw_both_sampling_classes_of_every_scene():
    """Runs after test_fp32_counts: every scene launched one specialisation
    for its stochastic kinds and the same without the stochastic bit for the
    others, and (when the whole file ran) both."""
    assert SEEN, "runs after test_fp32_counts"
    for name, seen in SEEN.items():
        assert all(bool(sub & STOCHASTIC_BIT) == stochastic for sub, stochastic in seen), (name, sorted(seen))
        assert len({sub & ~STOCHASTIC_BIT for sub, _ in seen}) == 1, (name, sorted(seen))
    if set(SEEN) == set(cs.SCENES):
        assert all({st for _, st in seen} == {False, True} for seen in SEEN.values()), SEEN


# ---- rows and bands ----------------------------------------------------------

def test_rows_and_bands(gpu, oracle_mod):
    import torch
    name, kind, m, seed = "slats", akMultiJittered, 8, cs.SEEDS[0]
    ds = _ds(name)
    o = cs.options(kind, m, seed)
    rows = slice(5, 15)
    frame, st = _render(ds, o, y0=5, y1=15)
    assert st.numPrimaryRays == 10 * cs.W * 64, st
    _check_counts(name, kind, m, seed, frame, "slats-k3-m8-rows5..14", rows)
    assert not frame[:5].any() and not frame[15:].any()
    world, band_h = 3, 4
    n = band_rows(cs.H, band_h, world)
    whole = np.zeros((cs.H, cs.W, 3), np.float32)
    for rank in range(world):
        buf = torch.zeros(n * cs.W * 3, dtype=torch.float32, device="cuda")
        st = ds.render_bands_device(o, buf, band_h, rank, world)
        ys = rank_rows(cs.H, band_h, rank, world)
        assert st.numPrimaryRays == int((ys >= 0).sum()) * cs.W * 64, (rank, st)
        got = buf.view(n, cs.W, 3).cpu().numpy()
        assert not got[ys < 0].any(), rank  # padding rows stay as they were
        whole[ys[ys >= 0]] = got[ys >= 0]
    _check_counts(name, kind, m, seed, whole, "slats-k3-m8-bands3x4")


# ---- float64 -----------------------------------------------------------------

@pytest.mark.parametrize("name,kind,m,seed", cs.FP64_SAMPLINGS, ids=[cs.case_id(*c) for c in cs.FP64_SAMPLINGS])
def test_fp64_equals_oracle(gpu, oracle_mod, name, kind, m, seed):
    """The per-lane float64 sample tables, bit for bit; m = 64 and m = 256
    are the launches fill_params' scratch cap (256 MB) cuts to 16 blocks and
    to one."""
    ds = _ds(name)
    ref, rst = cs.oracle_frame(name, kind, m, seed)
    got, st = _render(ds, cs.options(kind, m, seed, Precision.fp64))
    assert np.array_equal(got, ref), int(np.count_nonzero((got != ref).any(axis=2)))
    assert st == rst, (st, rst)
    spp = cs.spp_of(kind, m)
    hits, off = cs.hit_counts(name, got, spp)
    k_lo, k_hi = cs.bounds(name, kind, m, seed)
    assert off.max() <= 0.05 and ((k_lo <= hits) & (hits <= k_hi)).all()


# ---- the samplers' limits ----------------------------------------------------

@pytest.mark.parametrize("kind", [akMultiJittered, akCorrelatedMultiJittered])
def test_table_kinds_stop_at_32_in_float32_only(gpu, oracle_mod, kind):
    ds = _ds("slats")
    seed = cs.SEEDS[1]
    with pytest.raises(RtmiError) as e:
        _render(ds, cs.options(kind, 33, seed, Precision.fp32))
    assert e.value.code == RT_E_UNSUPPORTED
    # the refused call leaves the scene as it was, and m = 32 is served
    frame, _ = _render(ds, cs.options(kind, 32, seed, Precision.fp32))
    _check_counts("slats", kind, 32, seed, frame, cs.case_id("slats", kind, 32, seed, "after-refusal"))
    ref, rst = cs.oracle_frame("slats", kind, 33, seed)
    got, st = _render(ds, cs.options(kind, 33, seed, Precision.fp64))
    assert np.array_equal(got, ref) and st == rst, (st, rst)


@pytest.mark.parametrize("prec", [Precision.fp32, Precision.fp64])
def test_grid_size_257_is_invalid(gpu, prec):
    ds = _ds("blocks2")
    for kind in (akGrid,) + cs.STOCHASTIC:
        with pytest.raises(RtmiError) as e:
            _render(ds, cs.options(kind, 257, cs.SEEDS[0], prec))
        assert e.value.code == RT_E_INVALID, int(kind)
    frame, st = _render(ds, cs.options(akNone, 1, 0, prec))
    assert st.numPrimaryRays == cs.W * cs.H
