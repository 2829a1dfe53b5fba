"""The float32 query fixtures (tests/golden/truth32_*.npz, what
test_gpu_truth32.py reads) on the CPU: that they are truth.py's, that enough
of every batch is decided at the float32 query margins, and that the
thresholds leave honest float32 arithmetic room: the specification written
out in plain numpy float32 (truth32_cases.brute_force: no tree, no list, no
clamp; independent of the oracle and of the kernels) names the truth's object
and face on every decided ray and stays within a quarter of the GPU tests'
bounds, on the inputs as they are and moved by one float32 ulp. A kernel that
disagrees on a decided ray is therefore wrong in its traversal, clamp or
lists, not in its rounding."""
import numpy as np
import pytest

import truth
import truth32_cases as c

META = c.meta()
RAYS = list(c.RAY_SCENES) + list(c.CORPUS)
FIXTURES = RAYS + [f"pick_{n}" for n in c.PICK_SCENES] + [f"shade_{n}" for n in c.SHADE_SCENES]


def _fresh(name, idx):
    if name.startswith("pick_"):
        return c.picks(name[5:], idx)
    if name.startswith("shade_"):
        return c.shade(name[6:], idx)
    return c.batch(name, idx)


# ---- the fixtures are truth.py's ---------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_regenerates(name):
    pytest.importorskip("mpmath")
    stored = c.load(name)
    n = len(stored["obj"])
    idx = np.sort(np.random.default_rng(len(name) + n).choice(n, max(6, n // 20), replace=False))
    for k, v in _fresh(name, idx).items():
        assert stored[k].dtype == v.dtype and stored[k][idx].tobytes() == np.ascontiguousarray(v).tobytes(), k


@pytest.mark.parametrize("name", list(c.RAY_SCENES) + list(c.SHADE_SCENES))
def test_rays_are_float32_and_meet_their_quotas(name):
    """make_rays asserts the quotas; the fixtures hold its rays."""
    if name in c.RAY_SCENES:
        b = c.load(name)
        for k, v in zip(("orig", "dir", "tnear"), c.make_rays(name)):
            assert v.dtype == np.float32 and b[k].tobytes() == v.tobytes()
        assert len(b["obj"]) == c.N_RAYS
        assert ((b["obj"] < 0) & np.isfinite(b["tnear"])).sum() >= 10       # t_near decides some answers
        assert ((b["obj"] >= 0) & np.isfinite(b["tnear"])).sum() >= 10
    if name in c.SHADE_SCENES:
        b = c.load(f"shade_{name}")
        for k, v in zip(("orig", "dir"), c.make_rays(name, c.N_SHADE)):
            assert b[k].tobytes() == v.tobytes()


@pytest.mark.parametrize("name", c.CORPUS)
def test_corpus_rays_are_the_generators(name):
    b = c.load(name)
    for k, v in zip(("orig", "dir", "tnear"), c.corpus_rays(name)):
        assert v.dtype == np.float32 and b[k].tobytes() == v.tobytes()
    assert len(b["obj"]) == c.N_RAYS


def test_inside_origins_meet_the_rules_they_are_there_for():
    """Origins inside a box, a sphere and a mesh's box occur with decided
    answers, and a ray that starts inside the mesh's box never hits the mesh."""
    for name in ("s15", "two_meshes", "mesh_mix"):
        b, scene = c.load(name), c.scene_of(name)
        ok = c.decided(b)[0]
        kinds = c.kinds(scene)
        for i in np.flatnonzero(kinds == 3):
            one = type(scene)(objects=[scene.objects[i]], lights=scene.lights, fov=scene.fov,
                              cameraToWorld=scene.cameraToWorld, bgColor=scene.bgColor)
            inside = c.inside_some_box(one, b["orig"])
            assert (inside & ok).sum() >= 3, name
            assert not (b["obj"][inside & ok] == i).any(), name
    pos = c.load("pick_s15")["xy"]
    assert (pos * 64 == np.round(pos * 64)).all() and ((pos < 0).any(1) | (pos[:, 0] >= c.PICK_W)).sum() >= 10


# ---- decided shares -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAYS + [f"pick_{n}" for n in c.PICK_SCENES])
def test_decided_shares(name):
    b = c.load(name)
    scene = c.scene_of(name[5:] if name.startswith("pick_") else name)
    ok, okn = c.decided(b, c.threshold(name))
    assert ok.mean() >= c.HIT_SHARE and okn.mean() >= c.NORMAL_SHARE, (ok.mean(), okn.mean())
    assert name.startswith("pick_") or 0.25 <= (b["obj"] >= 0).mean() <= 0.9      # hits and misses both
    if not name.startswith("pick_") and (c.kinds(scene) == 2).any():
        box = ok & (b["obj"] >= 0) & (c.kinds(scene)[np.maximum(b["obj"], 0)] == 2)
        assert box.sum() >= c.BOX_HITS and (box & okn).sum() >= c.BOX_HITS
        # the float64 margin calls every one of them undecided at EPS32: the hit axis' 1e-6
        assert (b["margin"][box] < truth.EPS32).all()
    if name in c.CORPUS:
        faces = b["face"][ok & okn & (b["face"] >= 0)]
        assert len(faces) >= 30 and len(set(faces)) >= 5    # mesh faces are among the decided answers


@pytest.mark.parametrize("name", list(c.SHADE_SCENES))
def test_radiance_shares(name):
    b, scene = c.load(f"shade_{name}"), c.scene_of(name)
    ok = b["normal32"] >= truth.EPS32
    assert ok.mean() >= c.SHADE_SHARE
    assert (b["counts"][:, 0] == 1).all() and (ok & (b["obj"] >= 0)).sum() >= 60
    box = ok & (b["obj"] >= 0) & (c.kinds(scene)[np.maximum(b["obj"], 0)] == 2)
    assert box.sum() >= 10
    if name in ("s35", "s63"):
        assert (b["counts"][ok, 4] > 0).sum() >= 30         # reflections are among them


# ---- the thresholds leave float32 room --------------------------------------------------------------
@pytest.mark.parametrize("name", RAYS + [f"pick_{n}" for n in c.PICK_SCENES])
def test_numpy_float32_specification_has_room(name):
    pick = name.startswith("pick_")
    scene = c.scene_of(name[5:] if pick else name)
    e = c.room(c.load(name), scene, c.threshold(name), pick)
    print(f"{name}: brute force t {e['t']:.3g} / {e['t_moved']:.3g} (bound {c.T_BOUND / 4:.3g}), "
          f"normal {e['normal']:.3g} / {e['normal_moved']:.3g} (bound {c.N_BOUND / 4:.3g})")
    rec = META["picks" if pick else "batches"][name[5:] if pick else name]["brute_force"]
    assert e == pytest.approx(rec, rel=0.5, abs=1e-7)       # the recorded figures are these


def test_bounds_are_the_trace32_file_s():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_trace32.py")) as f:
        src = f.read()
    assert float(re.search(r"^T_BOUND = (\S+)", src, re.M).group(1)) == c.T_BOUND
    assert float(re.search(r"^N_BOUND = (\S+)", src, re.M).group(1)) == c.N_BOUND


# ---- the comparison sees a wrong answer ---------------------------------------------------------------
def _right(b):
    """Answers that pass: the truth itself rounded to float32."""
    return {"t": np.where(b["obj"] >= 0, b["t"], b["tnear"].astype(np.float64)).astype(np.float32),
            "obj": b["obj"].copy(), "face": b["face"].copy(), "normal": b["normal"].astype(np.float32)}


@pytest.mark.parametrize("wrong", ["face", "normal", "t", "object", "miss_t", "miss_normal"])
def test_compare_fails_on_a_wrong_answer(wrong):
    b = c.load("s15")
    ok, okn = c.decided(b)
    c.compare(b, _right(b))
    got = _right(b)
    mesh_hit = np.flatnonzero(ok & okn & (b["face"] >= 0))[0]
    hit = np.flatnonzero(ok & okn & (b["obj"] >= 0) & (b["t"] >= 1.0))[3]
    miss = np.flatnonzero(ok & (b["obj"] < 0) & np.isfinite(b["tnear"]))[0]
    if wrong == "face":
        got["face"][mesh_hit] += 1
    elif wrong == "normal":
        got["normal"][hit] = -got["normal"][hit]
    elif wrong == "t":
        got["t"][hit] = np.float32(b["t"][hit] * (1.0 + 2.0 * c.T_BOUND))
        assert b["t"][hit] >= 1.0
    elif wrong == "object":
        got["obj"][miss] = 0
    elif wrong == "miss_t":
        got["t"][miss] = np.nextafter(got["t"][miss], np.float32(0.0))
    else:
        got["normal"][miss, 1] = 1e-30
    with pytest.raises(AssertionError):
        c.compare(b, got)


def test_an_undecided_ray_is_not_judged():
    b = c.load("s11")
    ok = c.decided(b)[0]
    assert not ok.all()
    got = _right(b)
    got["obj"][~ok] = 7
    c.compare(b, got)
