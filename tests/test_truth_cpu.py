"""The oracle, glm.py and the recorded fixtures against the multiprecision
truth (truth.py), on the CPU. The ~260 GPU tests compare kernels with
oracle/rt_oracle.c; this file anchors that oracle, and the matrices both
sides receive from rtmi/glm.py, to the written specification evaluated in
200-bit arithmetic, and pins tests/golden/truth_*.npz (what test_gpu_truth.py
reads) to truth.py.

Tolerances on t, normals and inverses are TOL times the oracle's error
measured when the fixtures were written (truth_meta.json)."""
import ctypes as C
import math

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, glm
from rtmi._lib import lib
from rtmi.framebuf import to_uint

import truth
import truth_cases as tc
from subset_scenes import subset_scene

META = truth.meta()
TOL = META["tol_factor"]
ANGLES = [-12.0, -15.0, -20.0, 35.0, 90.0] + [k * 360.0 / 13.0 for k in range(13)]
AXES = [glm.X_AXIS, glm.Y_AXIS, glm.Z_AXIS, np.array([1.0, -2.0, 0.5])]
# glm's entries against m * T, m * S, m * R: an entry of R takes at most 5
# float64 roundings (cos, sin, 1 - c, a product, a sum) after the axis' 3, an
# entry of the product a 3-term dot of them: under 16 roundings of half an
# ulp of the largest entry
GLM_ULPS = 8.0


def _base():
    """A matrix that is neither the identity nor symmetric."""
    m = glm.translate(glm.mat4(1.0), glm.vec3(0.5, -1.25, 3.0))
    m = glm.rotate(m, np.array([0.3, 1.0, -0.2]), 0.7)
    return glm.scale(m, glm.vec3(1.5, 0.75, 2.0))


def _err(got, want_rows):
    return float(truth.vec_ulps(np.asarray(got)[None], truth.to_glm(want_rows)[None])[0])


# ---- glm against mathematics -------------------------------------------------------------
@pytest.mark.parametrize("m", [glm.mat4(1.0), _base()], ids=["identity", "general"])
def test_translate_scale_are_post_multiplications(m):
    v = glm.vec3(1.0, 5.5, -3.5)
    assert _err(glm.translate(m, v), truth.mat_mul(truth.rows(m), truth.translation(v))) <= GLM_ULPS
    assert _err(glm.scale(m, v), truth.mat_mul(truth.rows(m), truth.scaling(v))) <= GLM_ULPS


@pytest.mark.parametrize("m", [glm.mat4(1.0), _base()], ids=["identity", "general"])
def test_rotate_is_m_times_the_right_handed_rotation(m):
    for axis in AXES:
        for deg in ANGLES:
            a = glm.degToRad(deg)
            want = truth.mat_mul(truth.rows(m), truth.rotation(axis, a))
            assert _err(glm.rotate(m, axis, a), want) <= GLM_ULPS, (axis, deg)
            assert _err(glm.rotate(m, a, axis), want) <= GLM_ULPS, (axis, deg)   # the other argument order


def test_rotation_sense():
    """+90 degrees about Y takes +Z to +X, about X takes +Y to +Z, about Z
    takes +X to +Y: in glm.py and in the truth's own rotation."""
    q = math.pi / 2
    for axis, src, dst in ((glm.Y_AXIS, (0, 0, 1), (1, 0, 0)), (glm.X_AXIS, (0, 1, 0), (0, 0, 1)),
                           (glm.Z_AXIS, (1, 0, 0), (0, 1, 0))):
        got = glm.mul(glm.rotate(glm.mat4(1.0), axis, q), glm.vec(*src))
        assert np.abs(got[:3] - np.array(dst, float)).max() <= 2e-16, (axis, got)
        mine = truth.xf_dir(truth.rotation(axis, q), truth._vec(src))
        assert max(abs(float(mine[i]) - dst[i]) for i in range(3)) <= 2e-16


def test_normalize():
    for v in ([-2.0, -0.8, -0.3, 0.0], [3.0, -0.5, -4.0, 0.0], [1e-3, 2e5, -7.0]):
        want = truth._normalize(truth._vec(v))
        got = glm.normalize(np.array(v))
        assert truth.vec_ulps(got[None, :3], np.array([[float(x) for x in want]]))[0] <= 2.0
        assert len(got) == len(v) and (len(v) == 3 or got[3] == 0.0)


def _native_inverse(m):
    out = (C.c_double * 16)()
    rc = lib().rt_mat4_inverse((C.c_double * 16)(*glm.flat(m)), out)
    return rc, np.array(list(out)).reshape(4, 4)


def test_inverses_against_the_multiprecision_inverse():
    mats = tc.matrices()
    assert len(mats) == 230
    tol = TOL * META["inverse_ulp"]
    worst = 0.0
    for m in mats:
        want = truth.mat_inverse(truth.rows(m))
        rc, nat = _native_inverse(m)
        assert rc == abi.RT_OK
        worst = max(worst, _err(glm.inverse(m), want), _err(nat, want))
    print(f"inverses: largest error {worst:.1f} ulps of the largest entry (recorded {META['inverse_ulp']})")
    assert worst <= tol


def test_singular_matrix_is_invalid():
    m = glm.mat4(1.0)
    m[2] = m[1] * 2.0
    assert _native_inverse(m)[0] == abi.RT_E_INVALID
    assert _native_inverse(np.zeros((4, 4)))[0] == abi.RT_E_INVALID
    with pytest.raises(ValueError):
        glm.inverse(np.zeros((4, 4)))


# ---- the oracle's primitives -----------------------------------------------------------------
@pytest.mark.parametrize("kind", tc.PRIMITIVES)
def test_oracle_primitive(oracle_mod, kind):
    args = tc.primitive_inputs(kind)
    want, margins = tc.primitive_truth(kind, args)
    e = tc.compare_primitive(kind, want, margins, tc.primitive_oracle(oracle_mod, kind, args),
                             TOL * META["primitives"][kind]["ulp"])
    print(f"{kind}: largest error {e:.1f} ulps (recorded {META['primitives'][kind]['ulp']})")


# ---- the oracle's trace and castPrimaryRay + trace -------------------------------------------
@pytest.mark.parametrize("name", list(tc.BATCHES))
def test_oracle_trace(oracle_mod, name):
    b, entry = truth.load(name), META["batches"][name]
    if name in tc.SEEDED:
        assert len(b["t"]) == tc.N_RAYS and (b["orig"][:, 1] > 0).all()
    hit = (b["obj"] >= 0).mean()
    assert 0.25 <= hit <= 0.9, hit
    if name != "edge4":
        assert ((b["obj"] < 0) & np.isfinite(b["tnear"])).sum() >= 10      # t_near decides some answers
    if name == "edge15":    # both sides of the plane's threshold, far from and just beside it
        ground = (b["obj"][200:] == 4).reshape(20, 6)
        assert not ground[:, :3].any() and ground[:, 3:].sum() >= 30
    if name == "edge4":     # both sides of det < 1e-6 on the face aimed at
        aimed = (b["face"] == 2 * np.arange(len(b["t"]))).reshape(-1, 8)
        assert not aimed[:, :3].any() and aimed[:, 3:].sum() >= 30
    got = tc.oracle_answers(oracle_mod.OracleScene(tc.BATCHES[name]()), b)
    e = tc.compare(b, got, TOL * entry["t_ulp"], TOL * entry["normal_ulp"])
    print(f"{name}: largest errors t {e[0]:.1f}, normal {e[1]:.1f} ulps (recorded {entry['t_ulp']}, {entry['normal_ulp']})")


@pytest.mark.parametrize("name", tc.PICK_SCENES)
def test_oracle_camera_rays(oracle_mod, name):
    """castPrimaryRay of the oracle, then its trace, against the truth's picks."""
    b, entry = truth.load(f"pick_{name}"), META["picks"][name]
    sc = tc.BATCHES[name]()
    rays = [oracle_mod.cast_primary_ray(tc.PICK_W, tc.PICK_H, x, y, sc.fov, sc.cameraToWorld) for x, y in b["xy"]]
    mine = dict(b, orig=np.array([r[0][:3] for r in rays]), dir=np.array([r[1][:3] for r in rays]))
    assert truth.vec_ulps(mine["dir"], b["dir"]).max() <= TOL * META["primitives"]["camera"]["ulp"]
    tc.compare(b, tc.oracle_answers(oracle_mod.OracleScene(sc), mine), TOL * entry["t_ulp"], TOL * entry["normal_ulp"])


# ---- the oracle's pixels ---------------------------------------------------------------------
def _oracle_frame(oracle_mod, scene, m, depth):
    opts = Options(width=tc.FRAME_W, height=tc.FRAME_H, antialias=Antialias(akGrid if m else akNone, max(m, 1)),
                   bias=tc.BIAS, maxRayDepth=depth, precision=Precision.fp64)
    osc = oracle_mod.OracleScene(scene)
    rgb = np.zeros((tc.FRAME_H, tc.FRAME_W, 3))
    stats = np.zeros((tc.FRAME_H, tc.FRAME_W, 5), np.int64)
    for y in range(tc.FRAME_H):
        for x in range(tc.FRAME_W):
            c, st = osc.calc_pixel(opts, x, y)
            rgb[y, x] = c
            stats[y, x] = (st.numPrimaryRays, st.numIntersectionTests, st.numIntersectionHits, st.numShadowRays,
                           st.numReflectionRays)
    return rgb, stats


def compare_frame(f, rgb, stats):
    ok = f["margin"] >= truth.EPS
    assert (~ok).mean() <= tc.UNDECIDED_CAP
    assert truth.within_f32_ulp(rgb, f["rgb"])[ok].all()
    assert np.array_equal(stats[ok], f["stats"][ok])


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("bits", tc.FRAME_BITS)
def test_oracle_pixels(oracle_mod, bits, m):
    compare_frame(truth.load(f"frame_{bits}_m{m}"), *_oracle_frame(oracle_mod, subset_scene(bits), m, tc.DEPTH))


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("bits", [35, 63])
def test_oracle_pixels_depth_1(oracle_mod, bits, m):
    """The recursion limit: the same frames at maxRayDepth 1, the truth computed here."""
    ts = truth.TruthScene(subset_scene(bits))
    px = [[truth.pixel(ts, tc.FRAME_W, tc.FRAME_H, x, y, m, tc.BIAS, 1) for x in range(tc.FRAME_W)]
          for y in range(tc.FRAME_H)]
    f = {"rgb": np.array([[p[0] for p in r] for r in px]), "stats": np.array([[p[1] for p in r] for r in px]),
         "margin": np.array([[p[2] for p in r] for r in px])}
    deep = truth.load(f"frame_{bits}_m{m}")
    assert (f["stats"][..., 4] < deep["stats"][..., 4]).any()      # the limit cut some reflection short
    compare_frame(f, *_oracle_frame(oracle_mod, subset_scene(bits), m, 1))


# ---- caps, on the truth alone ----------------------------------------------------------------
def test_caps():
    for name in tc.BATCHES:
        assert (truth.load(name)["margin"] < truth.EPS).mean() <= tc.UNDECIDED_CAP
        assert META["batches"][name]["undecided"] <= tc.UNDECIDED_CAP
    for name in tc.PICK_SCENES:
        assert (truth.load(f"pick_{name}")["margin"] < truth.EPS).mean() <= tc.UNDECIDED_CAP
    for bits in tc.FRAME_BITS:
        for m in tc.FRAME_M:
            f = truth.load(f"frame_{bits}_m{m}")
            assert (f["margin"] >= truth.EPS).all()        # their Stats are compared
            assert m == 0 or (f["margin32"] >= truth.EPS32).mean() >= 0.5
            assert f["stats"][..., 0].sum() == tc.FRAME_W * tc.FRAME_H * max(1, m * m)
    z = truth.load("quant")
    for bits, srgb in tc.QUANT_CASES:
        assert z[f"und_{bits}_{int(srgb)}"].mean() <= tc.QUANT_CAP


# ---- the fixtures are truth.py's ---------------------------------------------------------------
def _same(stored, fresh, sel):
    for k, v in fresh.items():
        assert stored[k][sel].tobytes() == np.ascontiguousarray(v).tobytes(), k


@pytest.mark.parametrize("name", list(tc.BATCHES))
def test_fixture_rays_regenerate(name):
    stored = truth.load(name)
    idx = np.arange(0, len(stored["t"]), 16)
    _same(stored, tc.batch(name, idx), idx)


@pytest.mark.parametrize("name", tc.PICK_SCENES)
def test_fixture_picks_regenerate(name):
    idx = np.arange(0, 120, 16)
    _same(truth.load(f"pick_{name}"), tc.picks(name, idx), idx)


@pytest.mark.parametrize("m", tc.FRAME_M)
@pytest.mark.parametrize("bits", tc.FRAME_BITS)
def test_fixture_frame_rows_regenerate(bits, m):
    rows = [3, 8]
    _same(truth.load(f"frame_{bits}_m{m}"), tc.frame(bits, m, rows), rows)


def test_fixture_quantiser_regenerates():
    z = truth.load("quant")
    v = tc.quant_inputs()
    assert z["v"].tobytes() == v.tobytes()
    idx = np.arange(0, len(v), 16)
    for bits, srgb in tc.QUANT_CASES:
        q, und = truth.quantise(v[idx], bits, srgb)
        assert np.array_equal(z[f"q_{bits}_{int(srgb)}"][idx], q) and np.array_equal(z[f"und_{bits}_{int(srgb)}"][idx], und)


# ---- the comparisons can see small errors ---------------------------------------------------------
def _xf_wrong(tx, ty, tz):
    """subset_scenes._xf's general transform with the Y angle negated."""
    m = glm.translate(glm.mat4(1.0), glm.vec3(tx, ty, tz))
    m = glm.rotate(m, glm.Y_AXIS, glm.degToRad(-35.0))
    m = glm.rotate(m, glm.X_AXIS, glm.degToRad(-20.0))
    return glm.scale(m, glm.vec3(1.3, 0.8, 1.1))


def _set_xf(geometry, m):
    geometry.objectToWorld = m
    geometry.worldToObject = glm.inverse(m)


def _oracle_fails(oracle_mod, name, scene):
    b, entry = truth.load(name), META["batches"][name]
    got = tc.oracle_answers(oracle_mod.OracleScene(scene), b)
    with pytest.raises(AssertionError):
        tc.compare(b, got, TOL * entry["t_ulp"], TOL * entry["normal_ulp"])


def test_sees_a_negated_rotation(oracle_mod):
    sc = subset_scene(11)
    _set_xf(sc.objects[0].geometry, _xf_wrong(-3.5, 1.6, -11.0))
    _set_xf(sc.objects[2].geometry, _xf_wrong(3.5, 1.4, -12.0))
    _oracle_fails(oracle_mod, "s11", sc)


def test_sees_a_radius_off_by_1e_9(oracle_mod):
    sc = subset_scene(3)
    sc.objects[0].geometry.r *= 1.0 + 1e-9
    _oracle_fails(oracle_mod, "s3", sc)


def test_sees_a_vertex_moved_by_1e_9(oracle_mod):
    b = truth.load("s4")
    faces, counts = np.unique(b["face"][b["face"] >= 0], return_counts=True)
    sc = subset_scene(4)
    mesh = sc.objects[0].geometry
    for f in faces[np.argsort(-counts)][:1]:       # one vertex, of the face most rays of the batch hit
        mesh.vertices[mesh.faces[f][0]] += 1e-9 / math.sqrt(3.0)
    _oracle_fails(oracle_mod, "s4", sc)


def test_sees_a_light_brighter_by_1e_5(oracle_mod):
    sc = subset_scene(19)
    sc.lights[0].intensity *= 1.0 + 1e-5
    with pytest.raises(AssertionError):
        compare_frame(truth.load("frame_19_m0"), *_oracle_frame(oracle_mod, sc, 0, tc.DEPTH))


# ---- the output quantiser against its definition ----------------------------------------------------
@pytest.mark.parametrize("bits,srgb", tc.QUANT_CASES)
def test_quantisers_against_the_definition(oracle_mod, bits, srgb):
    z = truth.load("quant")
    v, q, und = z["v"], z[f"q_{bits}_{int(srgb)}"], z[f"und_{bits}_{int(srgb)}"]
    assert np.array_equal(to_uint(v, bits, srgb)[~und], q[~und])
    mine = np.array([oracle_mod.ppm_outvalue(x, bits, srgb) for x in v])
    assert np.array_equal(mine[~und], q[~und])
