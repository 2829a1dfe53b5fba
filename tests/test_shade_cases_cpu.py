"""The radiance-query rays (shade_cases.py) on the oracle and tests/truth.py
alone: the inputs test_gpu_shade_rays.py sends leave its comparisons room.

* every camera batch of a scene (the 15 x 11 image, the 5 x 4 images at
  akGrid 2, 3 and 8) hits every object of its scene, so every kind, has hits
  with a hidden light and hits with a visible one, misses too, and in the
  reflective scenes spawns reflection rays;
* the four-camera batch of the independence test does the same as a whole,
  and each of its cameras is what its name says (the camera inside the
  torus's box and the one below the ground cannot, by their purpose, see
  every kind: the first misses the mesh it starts in, which is the point);
* a grid batch's positions are grid()'s, in calcPixel's order;
* the truth fixtures regenerate identically, at most UNDECIDED_CAP of their
  rays are undecided, they hit every object and miss, spawn reflection rays,
  and their first hits are the oracle's."""
import numpy as np
import pytest

import cameras
import shade_cases as sc
import truth
import truth_cases as tc
from rtmi.scene import TriangleMesh
from subset_scenes import subset_scene

BATCHES = [(sc.W1, sc.H1, 0)] + [(sc.W2, sc.H2, m) for m in sc.GRID_M]


@pytest.mark.parametrize("w,h,m", BATCHES)
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_camera_batches_leave_room(oracle_mod, name, w, h, m):
    scene = sc.SCENES[name]()
    orig, d = sc.scene_rays(oracle_mod, name, w, h, m)
    assert len(orig) == w * h * max(m, 1) ** 2
    obj, shadowed, lit = sc.classify(oracle_mod, scene, orig, d)
    assert set(obj[obj >= 0]) == set(range(len(scene.objects)))       # every object, so every kind
    assert (obj < 0).any()
    assert shadowed.sum() >= 4 and lit.sum() >= 4
    _, _, st, _ = sc.expected(oracle_mod, name, w, h, m)
    assert st.numPrimaryRays == len(orig)
    assert (st.numReflectionRays > 0) == (name in sc.REFLECTIVE)
    if name in sc.REFLECTIVE:
        assert st.numReflectionRays >= len(orig) // 4


def test_grid_positions():
    """sample_xy(w, h, m): m * m positions per pixel, pixels row by row, each
    inside its pixel, j (the row of the sample grid) outer, formed with
    grid()'s operations x + (i*xs + xoffs). (That they are the oracle's to the
    bit is what the device comparison with calc_pixel(akGrid, m) shows.)"""
    w, h, m = sc.W2, sc.H2, 3
    xy = sc.sample_xy(w, h, m)
    assert len(xy) == w * h * m * m
    px = np.array(xy).reshape(h, w, m, m, 2)
    assert (np.diff(px[..., 0], axis=3) > 0).all() and (np.diff(px[..., 1], axis=2) > 0).all()
    assert (np.floor(px[..., 0]) == np.arange(w)[None, :, None, None]).all()
    assert (np.floor(px[..., 1]) == np.arange(h)[:, None, None, None]).all()
    xs = 1.0 / 3.0
    assert tuple(px[1, 2, 1, 1]) == (2.0 + (1.0 * xs + xs * 0.5), 1.0 + (1.0 * xs + xs * 0.5))
    assert sc.sample_xy(3, 2) == [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (0.0, 1.0), (1.0, 1.0), (2.0, 1.0)]


def test_four_cameras(oracle_mod):
    scene = subset_scene(63)
    kinds = [sc.kind_of(o.geometry) for o in scene.objects]
    mesh_obj = kinds.index("mesh")
    mesh = scene.objects[mesh_obj].geometry
    assert isinstance(mesh, TriangleMesh)
    lo, hi = cameras.world_box(mesh)
    cams = sc.cameras63()
    assert list(cams) == ["default", "in_mesh_box", "below_ground", "fov120"]
    seen, parts = set(), {}
    for cname, (c2w, fov) in cams.items():
        orig, d = sc.camera_rays(oracle_mod, c2w, fov, sc.CAM_W, sc.CAM_H)
        obj, shadowed, lit = sc.classify(oracle_mod, scene, orig, d)
        parts[cname] = (orig, d, obj)
        seen |= set(obj[obj >= 0])
        assert shadowed.any() and lit.any(), cname
        _, _, st, _ = sc.oracle_image(oracle_mod, sc.with_camera(scene, c2w, fov), sc.CAM_W, sc.CAM_H)
        assert st.numReflectionRays > 0, cname
    assert seen == set(range(len(scene.objects)))
    # the default camera sees the torus; the camera inside its box does not
    # (the AABB gate), though it looks through where its faces are
    assert (parts["default"][2] == mesh_obj).sum() >= 4
    eye = parts["in_mesh_box"][0][0]
    assert (lo < eye).all() and (eye < hi).all()
    assert not (parts["in_mesh_box"][2] == mesh_obj).any()
    # below the ground, looking up: no ray gets away
    assert parts["below_ground"][0][0][1] < 0.0 and (parts["below_ground"][2] >= 0).all()
    assert (parts["below_ground"][2] == kinds.index("plane")).sum() >= sc.CAM_W * sc.CAM_H // 2
    # fov 120: the default camera's origin, other directions
    assert np.array_equal(parts["fov120"][0], parts["default"][0])
    assert not np.array_equal(parts["fov120"][1], parts["default"][1])
    # no two cameras share an origin except those two
    assert len({tuple(p[0][0]) for p in parts.values()}) == 3


@pytest.mark.parametrize("bits", sc.TRUTH_BITS)
def test_truth_rays(bits):
    orig, d = sc.truth_rays(bits)
    assert orig.shape == d.shape == (sc.N_TRUTH, 3)
    assert (orig[:, 1] >= 0.25).all()
    assert np.allclose(np.linalg.norm(d, axis=1), np.resize(sc.TRUTH_SCALES, sc.N_TRUTH), rtol=1e-12)
    f = truth.load(f"shade_{bits}")
    assert np.array_equal(f["orig"], orig) and np.array_equal(f["dir"], d)
    und = (f["margin"] < truth.EPS).mean()
    assert und <= tc.UNDECIDED_CAP
    hit = f["obj"] >= 0
    assert 0.5 <= hit.mean() <= 0.9                                   # hits and misses
    assert set(f["obj"][hit]) == set(range(len(subset_scene(bits).objects)))
    assert f["counts"][:, 4].sum() >= 48                              # reflection rays
    assert (f["counts"][:, 0] == 1).all()
    assert (f["counts"][hit, 3] >= len(subset_scene(bits).lights)).all()  # a shadow ray per light and hit
    assert (f["counts"][~hit, 3] == 0).all()
    assert np.isfinite(f["rgb"]).all()
    # a miss is the background
    assert np.array_equal(f["rgb"][~hit], np.tile(np.asarray(subset_scene(bits).bgColor, np.float64)[:3], ((~hit).sum(), 1)))


@pytest.mark.parametrize("bits", sc.TRUTH_BITS)
def test_truth_fixture_regenerates(bits):
    stored = truth.load(f"shade_{bits}")
    idx = np.arange(sc.N_TRUTH)
    again = sc.truth_shade(bits, idx)
    assert set(again) == set(stored)
    for k, v in again.items():
        assert sc.same_bits(np.asarray(stored[k][idx], v.dtype), v) if v.dtype.kind == "f" else np.array_equal(stored[k][idx], v), k


@pytest.mark.parametrize("bits", sc.TRUTH_BITS)
def test_truth_first_hits_are_the_oracles(oracle_mod, bits):
    """The oracle's camera cannot form these rays, but its trace takes them:
    the truth's first hits are the oracle's, object for object, on the
    decided rays."""
    f = truth.load(f"shade_{bits}")
    osc = oracle_mod.OracleScene(subset_scene(bits))
    ok = f["margin"] >= truth.EPS
    got = np.array([osc.trace(np.append(o, 1.0), np.append(d, 0.0))[0] for o, d in zip(f["orig"], f["dir"])])
    assert np.array_equal(got[ok], f["obj"][ok])
