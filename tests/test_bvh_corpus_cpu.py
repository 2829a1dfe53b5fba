"""The BVH corpus (tests/bvh_corpus.py) and the tree checker
(rtmi_test_bvh_check_host, csrc/rt_hooks.cpp) without a GPU: the proof that
both are sound before test_gpu_bvh.py puts the device builder's trees through
them.

For every mesh the host SAH builder (rt_bvh.cpp build_bvh) accepts it at a
depth the traversal stack holds; the checker finds nothing in its tree (valid,
every face inside all of its ancestors' boxes, leaves of at most 4 faces,
depth-first layout, boxes equal to refit_bvh's of the same topology) and walks
the depth the builder reports; and over the ray set the GPU file traces, the
oracle's brute-force answers are neither nearly all hits nor nearly all
misses. The checker itself is shown to see what it is there for: trees given
to it with one defect each."""
import numpy as np
import pytest

import bvh_corpus as bc
from rtmi import abi

# meshes whose faces the rays can see (the others are culled by the
# reference's absolute determinant threshold, or are thin slivers): there the
# mesh itself, not only the ground below it, is among the answers
FACES_SEEN = tuple(n for n in bc.SMALL if n.startswith(("soup_", "torus", "line_pow2", "planar", "axis", "flat"))
                   and n not in ("soup_1", "soup_2", "soup_3", "soup_4", "soup_5", "soup_8", "soup_9")) + (
    "fan", "spiral_fan_up", "disc_log_up", "coincident", "coincident_1000")


@pytest.mark.parametrize("name", list(bc.MESHES))
def test_host_builder_tree_is_sound(name):
    rc, r = bc.check_host(bc.MESHES[name]())
    assert rc == abi.RT_OK
    assert bc.counters(r) == bc.ZERO, r
    assert 1 <= r["depth"] == r["reported_depth"] <= bc.MAX_DEPTH, r
    assert 1 <= r["leaf_max"] <= bc.LEAF_MAX and r["nodes"] >= 1
    assert np.isfinite(r["cost"]) and r["cost"] >= 0.0


@pytest.mark.parametrize("name", bc.SMALL)
def test_rays_leave_the_comparisons_room(oracle_mod, name):
    want = bc.reference(name)
    hit = float((want.obj >= 0).mean())
    assert hit >= 0.25 and 1.0 - hit >= 0.10, (name, hit)
    if name in FACES_SEEN:
        assert float((want.face >= 0).mean()) >= 0.15, name
    if name == "degenerate_mix":  # the point and line faces are never an answer
        faces = want.face[want.face >= 0]
        assert len(faces) >= 16 and (faces >= bc.N_POINT_FACES + bc.N_LINE_FACES).all()


def test_chain_meshes_stay_shallow_under_the_host_builder():
    """Object-median splits past depth 38 bound the host tree whatever the
    geometry; these are the depths DESIGN.md records next to the device's."""
    depths = {n: bc.check_host(bc.MESHES[n]())[1]["depth"] for n in bc.CHAINS}
    assert all(d <= 38 for d in depths.values()), depths


def test_checker_sees_one_defect_at_a_time():
    mesh = bc.soup(1025, 1125)
    _, box = bc.check_host(mesh, bc.BOX_DEFECT)
    assert box["uncontained"] >= 1 and box["host_boxes"] == 1
    assert {k: v for k, v in bc.counters(box).items() if k not in ("uncontained", "host_boxes")} == \
        {k: 0 for k in bc.COUNTERS if k not in ("uncontained", "host_boxes")}
    _, order = bc.check_host(mesh, bc.ORDER_DEFECT)
    assert order["layout"] >= 1 and order["invalid"] == order["uncontained"] == order["host_boxes"] == 0
    _, depth = bc.check_host(mesh, bc.DEPTH_DEFECT)
    assert bc.counters(depth) == bc.ZERO and depth["reported_depth"] == depth["depth"] + 1


def test_checker_sees_a_non_finite_vertex_as_the_builder_does():
    m = bc.soup(33, 3)
    m.vertices[5, 1] = np.inf
    rc, _ = bc.check_host(m)
    assert rc == abi.RT_E_INVALID
