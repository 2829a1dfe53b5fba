"""rt_scene_set_mesh_vertices / _device / rt_multi_set_mesh_vertices without a
GPU: exported with the signatures abi.SIGNATURES lists, null handles are error
codes with a message; and the host refit (rt_bvh.cpp refit_bvh) through the
hook rtmi_test_refit_host: a tree built by the SAH builder on vertices A and
refitted to vertices B stays a valid tree whose boxes contain every face."""
import ctypes as C

import numpy as np
import pytest

from rtmi import abi
from rtmi._lib import LIB_PATH, lib

HOST_ARGS = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double)]
NAMES = {
    "rt_scene_set_mesh_vertices": HOST_ARGS,
    "rt_scene_set_mesh_vertices_device": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "rt_multi_set_mesh_vertices": HOST_ARGS,
}


def test_entry_points_exported_with_signatures():
    lib()
    raw = C.CDLL(LIB_PATH)
    for name, want in NAMES.items():
        assert hasattr(raw, name), name
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int
        assert args == want, name
        fn = getattr(lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_null_handles_are_invalid():
    L = lib()
    v = (C.c_double * 9)()
    for name in ("rt_scene_set_mesh_vertices", "rt_multi_set_mesh_vertices"):
        assert getattr(L, name)(None, 0, v, 3, None) == abi.RT_E_INVALID
        msg = L.rt_last_error()
        assert msg and b"null" in msg, msg
        assert getattr(L, name)(None, 0, None, 0, None) == abi.RT_E_INVALID
        assert L.rt_last_error()
    assert L.rt_scene_set_mesh_vertices_device(None, 0, None, 3, None, None) == abi.RT_E_INVALID
    msg = L.rt_last_error()
    assert msg and b"null" in msg, msg


def refit_host(va, vb, faces):
    f = lib().rtmi_test_refit_host
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64,
                  C.POINTER(C.c_int64)]
    va = np.ascontiguousarray(va, np.float64)
    vb = np.ascontiguousarray(vb, np.float64)
    faces = np.ascontiguousarray(faces, np.int32)
    assert va.shape == vb.shape
    out = (C.c_int64 * 3)()
    rc = f(va.ctypes.data_as(C.POINTER(C.c_double)), vb.ctypes.data_as(C.POINTER(C.c_double)), va.shape[0],
           faces.ctypes.data_as(C.POINTER(C.c_int32)), faces.shape[0], out)
    assert rc == abi.RT_OK, lib().rt_last_error()
    return {"valid": int(out[0]), "uncontained": int(out[1]), "node_bytes": int(out[2])}


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (c + rng.uniform(-0.15, 0.15, (n, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def torus(nu=48, nv=24, R=1.0, r=0.4):
    u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    w = np.linspace(0, 2 * np.pi, nv, endpoint=False)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), r * np.sin(ww), (R + r * np.cos(ww)) * np.sin(uu)], -1)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b = idx, np.roll(idx, -1, 0)
    c, d = np.roll(b, -1, 1), np.roll(idx, -1, 1)
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f.astype(np.int32)


def twist(v, k=1.5):
    a = k * v[:, 1]
    out = v.copy()
    out[:, 0] = np.cos(a) * v[:, 0] + np.sin(a) * v[:, 2]
    out[:, 2] = -np.sin(a) * v[:, 0] + np.cos(a) * v[:, 2]
    return out


def test_identity_refit_rebuilds_the_same_bytes():
    v, f = soup(300, seed=11)
    r = refit_host(v, v, f)
    assert r == {"valid": 1, "uncontained": 0, "node_bytes": 0}


@pytest.mark.parametrize("deform", ["twist", "scramble"])
def test_torus_refit_contains_every_face(deform):
    v, f = torus()
    vb = twist(v) if deform == "twist" else v[np.random.default_rng(5).permutation(len(v))]
    r = refit_host(v, vb, f)
    assert r["valid"] == 1 and r["uncontained"] == 0
    assert r["node_bytes"] > 0  # the boxes did move


@pytest.mark.parametrize("scale", [1000.0, 0.001])
def test_margin_follows_the_scale(scale):
    v, f = torus()
    r = refit_host(v, scale * v, f)
    assert r["valid"] == 1 and r["uncontained"] == 0
    # the refit of the scaled positions is the tree the builder makes of them
    # whenever the split decisions agree; at least the identity holds there too
    r2 = refit_host(scale * v, scale * v, f)
    assert r2 == {"valid": 1, "uncontained": 0, "node_bytes": 0}


def test_refit_declines_a_non_finite_vertex():
    v, f = soup(20, seed=3)
    vb = v.copy()
    vb[7, 1] = np.nan
    fn = lib().rtmi_test_refit_host
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64,
                   C.POINTER(C.c_int64)]
    out = (C.c_int64 * 3)()
    rc = fn(v.ctypes.data_as(C.POINTER(C.c_double)), vb.ctypes.data_as(C.POINTER(C.c_double)), len(v),
            f.ctypes.data_as(C.POINTER(C.c_int32)), len(f), out)
    assert rc == abi.RT_E_INVALID and b"non-finite" in lib().rt_last_error()
