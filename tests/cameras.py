"""Cameras the per-call builders (csrc/rt_frame.hip, rt_bins.cpp) have
branches for and the standard viewpoint never reaches: shared by
test_gpu_cameras.py and test_bins_cpu.py (which also checks, in numpy, that
the cameras are what their names say for the meshes both files use).

Every eye position is computed from the mesh's world box (lo, hi), so the
table follows the mesh it is given: a camera whose nearest box corner lies a
hair in front of the camera plane, views along and across the ground plane's
normal, from below it and from exactly on it, a mesh a few pixels wide, very
wide and very narrow fields of view, and the three cases of a mesh box that
reaches the camera plane (camera inside the box; plane through the box with
every vertex in front of it; whole mesh behind)."""
import math

import numpy as np

STD_FOV = 50.0
_STD_TILT = math.radians(-12.0)
# the view direction of scenes._std_camera: -Z rotated about X by -12 degrees
STD_DIR = np.array([0.0, math.sin(_STD_TILT), -math.cos(_STD_TILT)])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def lookat(eye, target, roll=0.0):
    """cameraToWorld (glm column-major, m[col][row]) of a camera at `eye`
    looking at `target` (the reference's cameras look along -Z with +Y up),
    rolled by `roll` degrees about the view direction. A view along the world
    Y axis takes -Z as its up vector."""
    eye = np.asarray(eye, np.float64)
    f = _unit(np.asarray(target, np.float64) - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.999 else np.array([0.0, 0.0, -1.0])
    x = _unit(np.cross(f, up))
    y = np.cross(x, f)
    a = math.radians(roll)
    x, y = math.cos(a) * x + math.sin(a) * y, math.cos(a) * y - math.sin(a) * x
    m = np.zeros((4, 4))
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = x, y, -f, eye
    m[3, 3] = 1.0
    return m


def world_vertices(mesh):
    m = np.asarray(mesh.objectToWorld, np.float64)  # m[col][row]
    return mesh.vertices @ m[:3, :3] + m[3, :3]


def world_box(mesh):
    v = world_vertices(mesh)
    return v.min(axis=0), v.max(axis=0)


def box_corners(lo, hi):
    return np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]]
                     for c in range(8)])


def depths(c2w, pts):
    """Distance of world points in front of the camera plane (<= 0: at or behind it)."""
    c2w = np.asarray(c2w, np.float64)
    return (np.asarray(pts, np.float64) - c2w[3, :3]) @ -c2w[2, :3]


def _in_front(lo, hi, d, gap, roll=0.0):
    """Looking along d at the box centre, the nearest box corner `gap` in
    front of the camera plane."""
    c = 0.5 * (lo + hi)
    d = _unit(d)
    s = gap - ((box_corners(lo, hi) - c) @ d).min()
    eye = c - s * d
    return lookat(eye, eye + d, roll)


def _beside(lo, hi, verts):
    """The camera plane halfway between the box's and the vertices' nearest
    points along a diagonal: it cuts the box, every vertex is in front."""
    c = 0.5 * (lo + hi)
    d = _unit([-1.0, -1.0, -1.0])
    mc, mv = (box_corners(lo, hi) @ d).min(), (verts @ d).min()
    eye = c + d * (0.5 * (mc + mv) - c @ d)
    return lookat(eye, eye + d)


def camera_table(mesh, std_c2w):
    """name -> (cameraToWorld, fov) for `mesh` (placed in the world by its
    objectToWorld, over a ground plane y = 0); std_c2w: the scene's camera."""
    lo, hi = world_box(mesh)
    c = 0.5 * (lo + hi)
    std_eye = np.asarray(std_c2w, np.float64)[3, :3]
    verts = world_vertices(mesh)
    tab = {
        "closeup": (_in_front(lo, hi, c - std_eye, 0.05), STD_FOV),
        "closeup_roll": (_in_front(lo, hi, c - std_eye, 0.3, roll=33.0), STD_FOV),
        "topdown": (lookat([c[0], hi[1] + 6.0, c[2]], [c[0], 0.0, c[2]]), STD_FOV),
        "grazing": (lookat([c[0], 0.05, hi[2] + 8.0], [c[0], 0.05, c[2]]), STD_FOV),
        "below": (lookat([c[0] + 1.0, -4.0, hi[2] + 5.0], c), STD_FOV),
        "far_side": (lookat(c + 60.0 * _unit([1.0, 0.15, 0.2]), c), STD_FOV),
        "fov_wide": (np.array(std_c2w, np.float64), 120.0),
        "fov_narrow": (np.array(std_c2w, np.float64), 3.0),  # (sees the ground beyond the mesh only)
        # the same, turned to the mesh's nearest vertex: a few faces fill the frame
        "fov_narrow_aimed": (lookat(std_eye, verts[np.argmin(np.linalg.norm(verts - std_eye, axis=1))]), 3.0),
        "straddle": (lookat(c, c + STD_DIR), STD_FOV),
        "beside": (_beside(lo, hi, verts), STD_FOV),
        "behind": (lookat(c + 8.0 * STD_DIR, c + 9.0 * STD_DIR), STD_FOV),
        "on_plane": (lookat([c[0] + 2.0, 0.0, hi[2] + 7.0], c), STD_FOV),
    }
    return tab


def _log_uniform(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


def _signed_log_uniform(rng, lo, hi):
    s = 1.0 if rng.random() < 0.5 else -1.0
    return s * _log_uniform(rng, lo, hi)


ONEPLANE_SEED = 20261020
ONEPLANE_SHAPES = ("whole", "rows", "scanlines", "band_rank", "progressive")


AIMED_SHARE = 2.0 / 3.0   # of the cases: the view axis meets the plane at the mesh
SHADOW_SHARE = 0.75       # of the aimed cases: at the mesh's shadow, not at the mesh
ABOVE_SHARE = 0.75        # of the cases: every light shines from above the plane


def oneplane_case(rng):
    """One draw of the one-plane population (test_gpu_oneplane.py section d,
    test_uniform_cpu.py): a ground plane at height gy, a camera `cam_h` over
    (or under) it, pitched and rolled, its field of view, one or two distant
    lights with directions uniform on the sphere (one in four not
    normalised), the bias, the grid side m, the frame size, the call shape
    and the mesh's distance `dist` along the view direction.

    Drawn independently, those leave most frames empty: the camera looks away
    from the plane in half the cases, the mesh (which stands on the plane) is
    in frame in a quarter, its shadow almost never, and the per-call
    condition for uniform-lit pixels holds in one case of four. So two of the
    draws are coupled, by shares stated above: in an aimed case the view
    axis meets the plane `dist` from the eye, where the mesh stands, either
    by a pitch that follows from the drawn height (every second aimed case,
    if |cam_h| < dist: grazing views from low cameras, the horizon near the
    axis) or by a height that follows from the drawn pitch (|cam_h| =
    dist sin |pitch|, at least 1e-3: steep views); and in ABOVE_SHARE of
    the cases the lights' directions are mirrored to shine from above the
    plane (dir.y < 0), the side the condition needs. The other cases keep
    the independent draws: cameras far above or under the plane looking
    anywhere, lights below and along it.

    Every value is drawn on every call, in a fixed order, so the stream does
    not depend on what a caller uses."""
    c = {}
    c["gy"] = 0.0 if rng.random() < 0.25 else _signed_log_uniform(rng, 1e-3, 1e3)
    c["cam_h"] = _signed_log_uniform(rng, 1e-3, 1e3)
    c["pitch"] = float(rng.uniform(-89.0, 89.0))
    c["roll"] = float(rng.uniform(-180.0, 180.0))
    c["fov"] = _log_uniform(rng, 0.05, 150.0)
    above = rng.random() < ABOVE_SHARE
    lights = []
    for _ in range(int(rng.integers(1, 3))):
        d = _unit(rng.standard_normal(3))
        if above:
            d[1] = -abs(d[1])
        if rng.random() < 0.25:
            d = d * _log_uniform(rng, 1e-3, 1e3)
        lights.append(tuple(float(v) for v in d))
    c["lights"] = lights
    c["bias"] = _log_uniform(rng, 1e-7, 1e-1)
    c["m"] = int(rng.choice([16, 32, 64]))
    c["w"] = int(rng.integers(17, 97))
    c["h"] = int(rng.integers(5, 65))
    c["shape"] = ONEPLANE_SHAPES[int(rng.integers(0, len(ONEPLANE_SHAPES)))]
    c["dist"] = float(rng.uniform(4.0, 30.0))
    c["cut"] = float(rng.uniform(0.0, 0.9)) if rng.random() < 0.5 else 0.0  # share of the mesh's height under the plane
    c["aimed"] = bool(rng.random() < AIMED_SHARE)
    c["aim_shadow"] = bool(rng.random() < SHADOW_SHARE) and c["aimed"]
    keep_height = bool(rng.random() < 0.5)
    if c["aimed"]:
        side = 1.0 if c["cam_h"] > 0 else -1.0
        if keep_height and abs(c["cam_h"]) <= c["dist"] * math.sin(math.radians(89.0)):
            c["pitch"] = -side * math.degrees(math.asin(abs(c["cam_h"]) / c["dist"]))
        else:
            c["pitch"] = -side * abs(c["pitch"])
            c["cam_h"] = side * max(1e-3, c["dist"] * math.sin(math.radians(abs(c["pitch"]))))
    # the camera: at the world origin in x and z, looking along -Z pitched by `pitch`
    a = math.radians(c["pitch"])
    eye = np.array([0.0, c["gy"] + c["cam_h"], 0.0])
    c["eye"] = eye
    c["dir"] = np.array([0.0, math.sin(a), -math.cos(a)])
    c["c2w"] = lookat(eye, eye + c["dir"], c["roll"])
    return c


def oneplane_mesh_translation(c, vertices, inner):
    """Where case c puts a mesh with these object-space vertices: its box
    centre `dist` in front of the eye along the view direction in x and z,
    and in y resting on the plane, sunk through it by the share `cut` of its
    height (a camera under the plane sees that part, and the shadow the rest
    casts on the plane's upper side, which is the side every camera ray
    shades). In a shadow-aimed case the mesh is then moved along
    the plane so that the first light's shadow of `inner` (a point inside
    the solid, so strictly inside its shadow) falls where the box centre
    was, on the view axis (when that light shines from above, the point is
    above the plane and the move is at most 30 units)."""
    v = np.asarray(vertices, np.float64)
    vlo, vhi = v.min(axis=0), v.max(axis=0)
    target = c["eye"] + c["dist"] * c["dir"]
    height = vhi[1] - vlo[1]
    base = c["gy"] + 1e-4 - c["cut"] * height
    mid = 0.5 * (vlo + vhi)
    t = np.array([target[0] - mid[0], base - vlo[1], target[2] - mid[2]])
    light = np.asarray(c["lights"][0], np.float64)
    top = np.asarray(inner, np.float64) + t
    if c["aim_shadow"] and light[1] < 0.0 and top[1] > c["gy"]:
        s = (top[1] - c["gy"]) / -light[1]
        move = np.array([target[0] - (top[0] + s * light[0]), 0.0, target[2] - (top[2] + s * light[2])])
        if np.linalg.norm(move) <= 30.0:
            t = t + move
    return t


# the mesh box reaches the camera plane: the device builds no lists
DECLINED_ON_DEVICE = ("straddle", "beside", "behind")
# a vertex at or behind the camera plane: the host builders decline too
DECLINED_ON_HOST = ("straddle", "behind")
