"""The reference the float64 feature-buffer kernels are judged by
(aov64_model.py), anchored to the oracle and not to the library: the model
over oracle.trace / oracle.hit_normal at the sample positions of
coverage_scenes.pixel_offsets, on the five coverage scenes at 33 x 19.
round(alpha * spp) must lie in coverage_scenes' [k_lo, k_hi] on every pixel
(plain float64 geometry, independent of the oracle's trace), and the other
channels must be the ones the hits imply. No GPU."""
import numpy as np
import pytest

import aov64_model as am
import coverage_scenes as cs
import oracle
from rtmi import akGrid, glm
from rtmi.scene import akMultiJittered

CASES = [(akGrid, 2, 0), (akMultiJittered, 3, cs.SEEDS[1])]


def oracle_hits(name, kind, m, seed):
    sc = cs.scene(name)
    osc = oracle.OracleScene(sc)
    c2w = [float(v) for v in glm.flat(sc.cameraToWorld)]
    xy = am.sample_positions(cs.W, cs.H, kind, m, seed)
    n = cs.W * cs.H * xy.shape[2]
    t = np.full(n, np.inf)
    obj = np.full(n, -1, np.int32)
    face = np.full(n, -1, np.int32)
    nrm = np.zeros((n, 3))
    for i, (px, py) in enumerate(xy.reshape(-1, 2)):
        o, d = oracle.cast_primary_ray(cs.W, cs.H, float(px), float(py), sc.fov, c2w)
        ob, th, tri, _ = osc.trace(o, d)
        if ob >= 0:
            t[i], obj[i], face[i] = th, ob, tri
            nrm[i] = osc.hit_normal(o, d, ob, th, tri)
    osc.close()
    shape = xy.shape[:3]
    return t.reshape(shape), obj.reshape(shape), face.reshape(shape), nrm.reshape(shape + (3,)), sc


@pytest.mark.parametrize("kind,m,seed", CASES, ids=["grid2", "mj3"])
@pytest.mark.parametrize("name", cs.SCENES)
def test_model_over_the_oracle_counts_the_samples(name, kind, m, seed):
    t, obj, face, nrm, sc = oracle_hits(name, kind, m, seed)
    spp = cs.spp_of(kind, m)
    got = am.reduce_samples(t, obj, face, nrm, am.scene_albedo(sc))
    k = np.rint(got["alpha"] * spp).astype(np.int64)
    assert np.array_equal(k, (obj >= 0).sum(axis=2))  # round(alpha * spp) recovers the hit count
    k_lo, k_hi = cs.bounds(name, kind, m, seed)
    bad = np.argwhere((k < k_lo) | (k > k_hi))
    assert bad.size == 0, [(int(x), int(y), int(k[y, x]), int(k_lo[y, x]), int(k_hi[y, x])) for y, x in bad[:8]]
    assert 0 < k.sum() < cs.W * cs.H * spp
    # the other channels are the ones the hits imply
    none = k == 0
    assert np.isinf(got["depth"][none]).all() and (got["object"][none] == -1).all() and (got["face"][none] == -1).all()
    assert not got["normal"][none].any() and not np.signbit(got["normal"][none]).any()
    assert np.isfinite(got["depth"][~none]).all() and (got["object"][~none] >= 0).all()
    assert np.array_equal(got["depth"], np.where(obj >= 0, t, np.inf).min(axis=2))
    assert not got["albedo"].any()  # the coverage scenes are black


def test_the_sums_are_ordered_sums():
    """A pixel whose values cancel differently in another order: the model
    keeps the order of the sample index, starts from +0 and skips misses."""
    t = np.array([[3.0, 1.0, 1.0, 2.0]])
    obj = np.array([[0, 1, 0, -1]], np.int32)
    face = np.array([[-1, 5, 7, -1]], np.int32)
    nrm = np.zeros((1, 4, 3))
    nrm[0, :, 0] = (1e16, 1.0, -1e16, 123.0)  # (1e16 + 1) - 1e16 = 0 in this order; the miss's 123 is not added
    alb = np.array([[0.1, 0.2, 0.3], [0.7, 0.7, 0.7]])
    got = am.reduce_samples(t, obj, face, nrm, alb)
    assert got["alpha"][0] == 0.75 and got["depth"][0] == 1.0
    assert got["object"][0] == 1 and got["face"][0] == 5  # the tie on t = 1 goes to sample 1
    assert got["normal"][0, 0] == 0.0 and not np.signbit(got["normal"][0, 0])
    assert got["albedo"][0, 0] == ((0.0 + 0.1) + 0.7 + 0.1) * 0.25
