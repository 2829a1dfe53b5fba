"""Device BVH builder (rt_scene_desc.bvh_builder = RT_BVH_PLOC,
csrc/rt_bvh_gpu.hip). Either tree must give the brute-force answer of
TriangleMesh.intersect (src/renderer/geom.nim:339-358: closest t, lowest face
on ties), so frames and Stats rendered through the PLOC tree must be
bit-identical to those through the host SAH tree, whose own parity with the
oracle test_gpu_parity.py pins — in both precisions, for meshes from 1 face to
the bunny, including degenerate ones (coincident faces, a flat grid).

From test_ploc_tree_structure on, the tree itself is read back and examined
(rtmi_test_bvh_check, csrc/rt_hooks.cpp) over the corpus of tests/bvh_corpus.py,
whose soundness test_bvh_corpus_cpu.py proves without a GPU: structure, boxes,
layout, depth, determinism; answers against the oracle's brute force; SAH cost
against the host builder's; and what becomes of a mesh whose device tree is
deeper than the traversal stack."""
import ctypes as C

import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, abi, akGrid, akNone, scenes
from rtmi._lib import lib
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH
from rtmi.renderer import DeviceScene

import bvh_corpus as bc
from bvh_corpus import coincident as _coincident, flat_grid as _flat_grid, soup as _soup
from query_checks import check, check_stats, trace

pytestmark = pytest.mark.gpu


def _scene(mesh):
    return scenes._mesh_scene(mesh, "m", (0.7, 0.6, 0.5))


CASES = {
    "one_face": lambda: _scene(_soup(1, 1)),
    "two_faces": lambda: _scene(_soup(2, 2)),
    "four_faces": lambda: _scene(_soup(4, 3)),
    "five_faces": lambda: _scene(_soup(5, 4)),
    "soup_300": lambda: _scene(_soup(300, 5)),
    "coincident": lambda: _scene(_coincident()),
    "flat_grid": lambda: _scene(_flat_grid()),
    "torus": lambda: _scene(scenes.torus_mesh(48, 24)),
    "mesh_mix": scenes.mesh_mix,
    "two_meshes": scenes.two_meshes,
}


def _render(ds, opts):
    import torch
    fb = torch.zeros(opts.height * opts.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    return fb, st


@pytest.mark.parametrize("name", list(CASES))
def test_ploc_tree_renders_identically(gpu, name):
    import torch
    scene = CASES[name]()
    a = DeviceScene(scene, bvh_builder=RT_BVH_SAH)
    b = DeviceScene(scene, bvh_builder=RT_BVH_PLOC)
    ia, ib = a.info(), b.info()
    assert ia["num_triangles"] == ib["num_triangles"]
    assert 1 <= ib["max_bvh_depth"] <= 60 and ib["num_bvh_nodes"] >= 1
    for opts in (Options(width=96, height=72, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64),
                 Options(width=160, height=120, antialias=Antialias(akGrid, 2), bias=1e-4,
                         precision=Precision.fp32)):
        fa, sa = _render(a, opts)
        fb, sb = _render(b, opts)
        assert sa == sb, (name, opts.precision)
        assert torch.equal(fa, fb), (name, opts.precision)


def test_ploc_bunny_identical_and_compact(gpu):
    import torch
    scene = scenes.mesh_bunny()
    a = DeviceScene(scene, bvh_builder=RT_BVH_SAH)
    b = DeviceScene(scene, bvh_builder=RT_BVH_PLOC)
    ia, ib = a.info(), b.info()
    # leaves of <= 4 faces: at least nf/4 leaves -> nf/4 - 1 inner nodes, and
    # a tree no more than 2x the SAH one
    assert ib["num_triangles"] // 4 - 1 <= ib["num_bvh_nodes"] <= 2 * ia["num_bvh_nodes"]
    opts = Options(width=320, height=180, antialias=Antialias(akGrid, 4), bias=1e-4, precision=Precision.fp32)
    fa, sa = _render(a, opts)
    fb, sb = _render(b, opts)
    assert sa == sb
    assert torch.equal(fa, fb)


def test_ploc_fp64_matches_oracle(gpu, oracle_mod):
    """Direct oracle check through the PLOC tree (float64: bit-exact)."""
    scene = scenes.mesh_mix()
    opts = Options(width=64, height=48, antialias=Antialias(akGrid, 2), bias=1e-4, precision=Precision.fp64)
    ds = DeviceScene(scene, bvh_builder=RT_BVH_PLOC)
    fb = np.zeros((48, 64, 3), np.float32)
    st = ds.render_lines(opts, fb, 0, 48)
    o = oracle_mod.OracleScene(scene)
    ref, rst, _ = o.render(opts)
    assert np.array_equal(fb, ref)
    assert st == rst


def test_bad_builder_rejected(gpu):
    from rtmi._lib import RtmiError
    with pytest.raises(RtmiError):
        DeviceScene(scenes.mesh_bunny(), bvh_builder=7)


# ---- the corpus (tests/bvh_corpus.py): the tree itself, not only what is seen through it ----
DIFF_NAMES = ["trifast", "trif64", "n32", "n64", "bins", "boxes64", "boxes32", "children", "devmesh32", "devmesh64",
              "fmesh", "fobj", "objbox", "meshbox", "r14", "r15"]


def _mesh_diff(ds):
    f = lib().rtmi_test_mesh_update_diff
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 16)()
    assert f(ds.h, out) == 0, lib().rt_last_error()
    return dict(zip(DIFF_NAMES, [int(x) for x in out]))


def _tree_hashes(ds):
    """rtmi_test_mesh_hash words 0, 1, 4, 5: both record arrays, both node arrays."""
    f = lib().rtmi_test_mesh_hash
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 8)()
    assert f(ds.h, 0, out) == 0, lib().rt_last_error()
    return [int(out[k]) for k in (0, 1, 4, 5)]


@pytest.mark.parametrize("name", list(bc.MESHES))
def test_ploc_tree_structure(gpu, name):
    """The tree RT_BVH_PLOC leaves in the scene, read back: valid, every face
    inside all of its ancestors' boxes (back-facing and occluded ones too),
    leaves of at most 4 faces, depth-first layout, the depth the scene
    reports and the stack holds, boxes in all three copies equal to the host
    refit's of the same topology, k_pack's records and normals equal to the
    host's, and the same bytes from a second build.
    (torus_540k, past the 524,288 faces at which k_bounds' threads stride:
    1.7 s on an MI355X with both builds and both read-backs.)"""
    ds = DeviceScene(bc.mesh_scene(name), bvh_builder=RT_BVH_PLOC)
    r = bc.check_scene(ds)
    print(name, r)
    assert bc.counters(r) == bc.ZERO, r
    assert 1 <= r["depth"] == r["reported_depth"] <= bc.MAX_DEPTH, r
    assert r["reported_depth"] == ds.info()["max_bvh_depth"] and r["nodes"] == ds.info()["num_bvh_nodes"]
    assert 1 <= r["leaf_max"] <= bc.LEAF_MAX
    d = _mesh_diff(ds)
    assert d == dict.fromkeys(d, 0), d
    again = DeviceScene(bc.mesh_scene(name), bvh_builder=RT_BVH_PLOC)
    assert _tree_hashes(again) == _tree_hashes(ds)


O64 = Options(width=48, height=36, antialias=Antialias(akNone, 1), bias=1e-4, precision=Precision.fp64)
O32 = Options(width=64, height=48, antialias=Antialias(akGrid, 2), bias=1e-4, precision=Precision.fp32)


@pytest.mark.parametrize("name", bc.SMALL)
def test_corpus_answers(gpu, oracle_mod, name):
    """512 rays at the mesh through either builder's tree against the
    oracle's brute force (objects, faces, t bit for bit, Stats), then a
    float64 and a float32 frame: equal bytes and Stats from the two trees."""
    import torch
    scene = bc.mesh_scene(name)
    orig, d = (np.array(a) for a in bc.rays(name))  # (torch wants writable arrays)
    want = bc.reference(name)
    trees = {b: DeviceScene(scene, bvh_builder=b) for b in (RT_BVH_SAH, RT_BVH_PLOC)}
    for ds in trees.values():
        assert 1 <= ds.info()["max_bvh_depth"] <= bc.MAX_DEPTH
        got = trace(ds, orig, d)
        check(got, want)
        check_stats(got, want)
    for opts in (O64, O32):
        fa, sa = _render(trees[RT_BVH_SAH], opts)
        fb, sb = _render(trees[RT_BVH_PLOC], opts)
        assert sa == sb, (name, opts.precision)
        assert torch.equal(fa, fb), (name, opts.precision)


# PLOC cost / host SAH cost (the checker's SAH cost, cost_node = cost_tri = 1)
# as measured on an MI355X (the device builder's table). A mesh
# whose device tree is deeper than the stack is built by the host builder: 1.
COST_RATIO = {
    "soup_257": 0.956,
    "soup_1025": 0.937,
    "torus_2304": 0.991,
    "bunny": 1.071,
    "fan": 1.0,
    "fan3d": 1.0,
    "spiral_fan": 1.0,
    "disc_log": 0.853,
    "line_pow2_nested": 0.531,
    "line_pow2_apart": 0.514,
}


@pytest.mark.parametrize("name", list(COST_RATIO))
def test_ploc_tree_quality(gpu, name):
    """A valid tree that has become a chain, or has lost its collapse into
    leaves, costs more: at most 1.5 x the recorded ratio to the SAH tree's
    cost (the margin absorbs a retuned radius or tie-break)."""
    mesh = scenes.baked_bunny() if name == "bunny" else bc.MESHES[name]()
    rc, host = bc.check_host(mesh)
    assert rc == 0 and host["cost"] > 0.0
    ds = DeviceScene(scenes._mesh_scene(mesh, "m", (0.7, 0.6, 0.5)), bvh_builder=RT_BVH_PLOC)
    r = bc.check_scene(ds)
    assert bc.counters(r) == bc.ZERO, r
    ratio = r["cost"] / host["cost"]
    print(name, "cost", r["cost"], "host", host["cost"], "ratio", ratio, "depth", r["depth"], "nodes", r["nodes"])
    assert ratio <= 1.5 * COST_RATIO[name], (name, ratio)


def test_nan_vertex_is_a_bad_argument_under_both_builders(gpu):
    """Neither builder's min / max sees a NaN; rt_scene_create looks for it."""
    from rtmi._lib import RtmiError
    mesh = bc.soup(33, 3)
    mesh.vertices[5, 1] = np.nan
    for builder in (RT_BVH_SAH, RT_BVH_PLOC):
        with pytest.raises(RtmiError) as e:
            DeviceScene(_scene(mesh), bvh_builder=builder)
        assert e.value.code == abi.RT_E_INVALID, builder
        assert b"non-finite" in lib().rt_last_error()
    mesh.vertices[5, 1] = 0.25  # and nothing else was wrong with it
    assert DeviceScene(_scene(mesh), bvh_builder=RT_BVH_PLOC).info()["num_triangles"] == 33


@pytest.mark.parametrize("name", bc.CHAINS + ("soup_1025", "coincident_1000"))
def test_a_mesh_the_host_builder_accepts_is_never_refused(gpu, name):
    """The clustering has no depth bound, the traversal stack has (60). Where
    the device builder alone declines its own tree for its depth, the scene
    holds the host builder's tree, byte for byte; where it accepts it, the
    scene holds that tree."""
    mesh = bc.MESHES[name]()
    accepted, depth, nodes = bc.ploc_raw(mesh)
    print(name, "device builder alone: accepted", accepted, "depth", depth, "nodes", nodes)
    assert accepted == (depth <= bc.MAX_DEPTH), lib().rt_last_error()
    ploc = DeviceScene(bc.mesh_scene(name), bvh_builder=RT_BVH_PLOC)
    info = ploc.info()
    assert 1 <= info["max_bvh_depth"] <= bc.MAX_DEPTH
    if accepted:
        assert (info["max_bvh_depth"], info["num_bvh_nodes"]) == (depth, nodes)
    else:
        sah = DeviceScene(bc.mesh_scene(name), bvh_builder=RT_BVH_SAH)
        assert _tree_hashes(ploc) == _tree_hashes(sah) and info == {**sah.info(), "build_ms": info["build_ms"]}
