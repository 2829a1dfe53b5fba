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


# the mesh box reaches the camera plane: the device builds no lists
DECLINED_ON_DEVICE = ("straddle", "beside", "behind")
# a vertex at or behind the camera plane: the host builders decline too
DECLINED_ON_HOST = ("straddle", "behind")
