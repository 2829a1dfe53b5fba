"""The uniform-pixel proof (rt_bins_geom.h uniform_class, rt_render.cpp
uniform_cam) against every sample it speaks about, on the host: the class of
a pixel is a claim about all m x m samples of lean1q_loop's float32
arithmetic, which the GPU frames sample at a few thousand pixels and this file
checks at every pixel of a 64 x 40 frame for 200 seeded cameras (the
population of test_gpu_oneplane.py, cameras.oneplane_case) and m = 16, 32, 64:
about 2 x 10^9 samples.

The hooks (rt_hooks.cpp rtmi_test_uniform, rtmi_test_uniform_samples) form
FastParams and UniformCam through the functions a render call uses and
evaluate the kernel's cx, cy and N per sample with fmaf on the host; the
claims are checked here in numpy:
* uniform-sky: every sample's N is non-zero and of the sign opposite to nroy;
* uniform-lit: every sample's N has nroy's sign and
  |N| (1 - 3e-7) / sqrt(1 + cx^2 + cy^2) > float32(1e-6), the root in float64
  (3e-7: the proof's total for the kernel's roundings and v_rsq's ulp);
* lit_ok equals the stated per-call inequality;
* the proof reaches: where lit_ok holds, at least 90 % of the pixels two or
  more pixels away from any pixel with a sign change of N are classified."""
import ctypes as C

import numpy as np
import pytest

import cameras
from rtmi._lib import lib

W, H = 64, 40
NCAM = 200
SEED = cameras.ONEPLANE_SEED
EPS = 2.0 ** -23
MIXED, LIT, SKY = 0, 1, 2

_P = C.c_void_p


def _hooks():
    f = lib().rtmi_test_uniform
    f.restype = C.c_int
    f.argtypes = [_P, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32,
                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]
    g = lib().rtmi_test_uniform_samples
    g.restype = C.c_int
    g.argtypes = [_P, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]
    return f, g


def classify(c2w, fov, w, h, m, ty, bias, lights, rect=None):
    """(cls (rows, cols) uint8, lit_ok, the ten UniformCam floats)."""
    f, _ = _hooks()
    x0, y0, x1, y1 = rect or (0, 0, w, h)
    cam = np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(16))
    li = np.ascontiguousarray(np.asarray(lights, np.float64).reshape(-1, 3))
    cls = np.zeros((y1 - y0, x1 - x0), np.uint8)
    ok = C.c_int32(-1)
    u = np.zeros(10, np.float32)
    rc = f(cam.ctypes.data, fov, w, h, m, ty, bias, li.ctypes.data, len(li), x0, y0, x1, y1, cls.ctypes.data,
           C.addressof(ok), u.ctypes.data)
    assert rc == 0, rc
    return cls, int(ok.value), u


def samples(c2w, fov, w, h, m, ty, bias, rect=None):
    """(cx (cols, m), cy (rows, m), N (rows, cols, m (j), m (i))), float32."""
    _, g = _hooks()
    x0, y0, x1, y1 = rect or (0, 0, w, h)
    cam = np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(16))
    cx = np.zeros((x1 - x0, m), np.float32)
    cy = np.zeros((y1 - y0, m), np.float32)
    n = np.zeros((y1 - y0, x1 - x0, m, m), np.float32)
    rc = g(cam.ctypes.data, fov, w, h, m, ty, bias, x0, y0, x1, y1, cx.ctypes.data, cy.ctypes.data, n.ctypes.data)
    assert rc == 0, rc
    return cx, cy, n


def bound(oy, ty):
    """uniform_cam's bound on the bias as it states it: oy, ty and nroy in
    float32, their magnitudes summed in float64, times 16 x 2^-23."""
    oy, ty = np.float32(oy), np.float32(ty)
    nroy = np.float32(-(oy + ty))
    return 16.0 * EPS * (abs(float(oy)) + abs(float(ty)) + abs(float(nroy))), nroy


def lit_ok_stated(c2w, ty, bias, lights):
    b32 = np.float32(bias)
    bnd, _ = bound(np.asarray(c2w, np.float64)[3][1], ty)
    ok = bool(b32 >= np.float32(1e-30)) and float(b32) > bnd
    for d in lights:
        sdy = -np.float32(d[1])
        ok = ok and bool(sdy > np.float32(1e-6)) and bool(sdy <= np.float32(1e6))
    return ok


def _population():
    rng = np.random.default_rng(SEED)
    return [cameras.oneplane_case(rng) for _ in range(NCAM)]


def _far_from_a_sign_change(sign):
    """Pixels whose 5 x 5 neighbourhood (clipped to the frame) has N of the
    pixel's own strict sign at every sample: sign (rows, cols) in {-1, 0, +1},
    0 for a pixel with a zero or both signs among its samples."""
    h, w = sign.shape
    far = sign != 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, xs = slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx))
            yd, xd = slice(max(0, -dy), h + min(0, -dy)), slice(max(0, -dx), w + min(0, -dx))
            far[yd, xd] &= sign[ys, xs] == sign[yd, xd]
    return far


def _check_camera(k, c, m):
    """Checks the classes of camera k's every pixel against all its samples.
    Returns (lit_ok, lit, sky, far pixels, far pixels classified)."""
    ty = -c["gy"]  # the plane's world_to_object translation
    cls, ok, u = classify(c["c2w"], c["fov"], W, H, m, ty, c["bias"], c["lights"])
    what = (k, m, {q: c[q] for q in ("gy", "cam_h", "pitch", "roll", "fov", "lights", "bias")})
    assert ok == int(lit_ok_stated(c["c2w"], ty, c["bias"], c["lights"])), what
    nroy = u[9]
    assert nroy == bound(c["c2w"][3][1], ty)[1], what
    cx, cy, n = samples(c["c2w"], c["fov"], W, H, m, ty, c["bias"])
    nmin, nmax = n.min(axis=(2, 3)), n.max(axis=(2, 3))
    assert np.isfinite(nmin).all() and np.isfinite(nmax).all(), what
    sign = np.where(nmin > 0, 1, np.where(nmax < 0, -1, 0))
    toward = 1 if nroy > 0 else -1  # a hit: N of nroy's sign
    sky, lit = cls == SKY, cls == LIT
    assert set(np.unique(cls)) <= {MIXED, LIT, SKY}, what
    assert (sign[sky] == -toward).all(), (what, np.argwhere(sky & (sign != -toward))[:4])
    assert (sign[lit] == toward).all(), (what, np.argwhere(lit & (sign != toward))[:4])
    assert ok or not lit.any(), what
    if lit.any():
        ys, xs = np.nonzero(lit)
        root = np.sqrt(1.0 + (cx[xs].astype(np.float64) ** 2)[:, None, :] + (cy[ys].astype(np.float64) ** 2)[:, :, None])
        dy = np.abs(n[ys, xs].astype(np.float64)) * (1.0 - 3e-7) / root
        low = dy.min(axis=(1, 2))
        assert (low > float(np.float32(1e-6))).all(), (what, float(low.min()))
    far = _far_from_a_sign_change(sign)
    return ok, int(lit.sum()), int(sky.sum()), int(far.sum()), int((far & (cls != MIXED)).sum())


@pytest.mark.parametrize("m", [16, 32, 64])
def test_classes_hold_for_every_sample(m):
    lit = sky = far = far_cls = nok = 0
    worst = (1.0, None)
    for k, c in enumerate(_population()):
        ok, li, sk, fa, fc = _check_camera(k, c, m)
        lit += li
        sky += sk
        if ok:
            nok += 1
            far += fa
            far_cls += fc
            if fa and fc / fa < worst[0]:
                worst = (fc / fa, k)
    print(f"m={m}: lit_ok cameras {nok} of {NCAM}, lit {lit}, sky {sky}, far {far}, classified {far_cls}, "
          f"worst camera {worst}")
    assert lit > 0 and sky > 0 and nok > 0
    assert far > 0 and far_cls >= 0.9 * far, (far, far_cls, worst)


def test_hook_rectangle_equals_the_frame():
    """A pixel rectangle of either hook is that part of the whole frame."""
    c = _population()[3]
    ty = -c["gy"]
    rect = (5, 7, 23, 18)
    full, ok, u = classify(c["c2w"], c["fov"], W, H, 16, ty, c["bias"], c["lights"])
    part, ok2, u2 = classify(c["c2w"], c["fov"], W, H, 16, ty, c["bias"], c["lights"], rect)
    assert ok == ok2 and np.array_equal(u, u2) and np.array_equal(part, full[7:18, 5:23])
    cx, cy, n = samples(c["c2w"], c["fov"], W, H, 16, ty, c["bias"])
    px, py, pn = samples(c["c2w"], c["fov"], W, H, 16, ty, c["bias"], rect)
    assert np.array_equal(px, cx[5:23]) and np.array_equal(py, cy[7:18]) and np.array_equal(pn, n[7:18, 5:23])


def test_samples_equal_numpy_float32():
    """The hook's cx, cy and N are the listed expressions: numpy float32 for
    the roundings, float64 for each fma (a float32 product is exact there and
    the sum rounds once more than an fma only in double-rounding cases, which
    a difference of more than one ulp would not be)."""
    c = _population()[5]
    m = 16
    _, _, u = classify(c["c2w"], c["fov"], W, H, m, -c["gy"], c["bias"], c["lights"])
    cam_a, cam_b, cam_c, cam_d, c4, c7, c10, st, of, _ = u
    cx, cy, n = samples(c["c2w"], c["fov"], W, H, m, -c["gy"], c["bias"])
    idx = np.arange(m, dtype=np.float32)
    off = (idx.astype(np.float64) * float(st) + float(of)).astype(np.float32)
    ex = ((np.arange(W, dtype=np.float32)[:, None] + off[None, :]) - cam_b) * cam_a
    ey = (cam_d - (np.arange(H, dtype=np.float32)[:, None] + off[None, :])) * cam_c
    assert np.array_equal(ex.astype(np.float32), cx) and np.array_equal(ey.astype(np.float32), cy)
    ay = (cx.astype(np.float64) * float(c4) - float(c10)).astype(np.float32)  # (cols, i)
    en = (cy.astype(np.float64)[:, None, :, None] * float(c7) + ay.astype(np.float64)[None, :, None, :])
    ulp = np.spacing(np.abs(n).astype(np.float32)).astype(np.float64)
    assert (np.abs(en - n.astype(np.float64)) <= ulp).all()


@pytest.mark.parametrize("gy", [0.0, 2.5, -3.0, 700.0])
def test_bias_one_float32_either_side_of_the_bound(gy):
    """lit_ok flips between the largest float32 <= the bound and the next
    one, and the bound is set by |ty| when the plane is far from y = 0."""
    c2w = cameras.lookat([0.0, gy + 5.5, 1.5], [0.0, gy + 4.5, -3.0])
    bnd, _ = bound(c2w[3][1], -gy)
    below = np.float32(bnd)
    if float(below) > bnd:
        below = np.nextafter(below, np.float32(0.0))
    above = np.nextafter(below, np.float32(np.inf))
    assert float(below) <= bnd < float(above)
    light = [(-0.9, -0.4, -0.1)]
    assert classify(c2w, 50.0, W, H, 16, -gy, float(above), light)[1] == 1
    assert classify(c2w, 50.0, W, H, 16, -gy, float(below), light)[1] == 0
    if gy == 700.0:
        assert abs(bnd - 16.0 * EPS * (705.5 + 700.0 + 5.5)) < 1e-9 and bnd > 1e-4


@pytest.mark.parametrize("y,ok", [
    (-float(np.nextafter(np.float32(1e-6), np.float32(1.0))), 1), (-float(np.float32(1e-6)), 0),
    (-float(np.float32(1e6)), 1), (-float(np.nextafter(np.float32(1e6), np.float32(np.inf))), 0)])
def test_light_height_one_float32_either_side(y, ok):
    c2w = cameras.lookat([0.0, 5.5, 1.5], [0.0, 4.5, -3.0])
    assert classify(c2w, 50.0, W, H, 16, 0.0, 1e-4, [(-0.9, y, -0.1)])[1] == ok
    assert classify(c2w, 50.0, W, H, 16, 0.0, 1e-4, [(-0.9, -0.4, -0.1), (-0.9, y, -0.1)])[1] == ok
