"""The tie rule of TriangleMesh.intersect (geom.nim:339-358: closest t, the
LOWEST face on ties), made observable.

64 coincident copies of one front-facing triangle tie exactly in t on every
ray that meets them. With computed normals every copy shades alike, so any
winner renders the same frame; here each copy carries a supplied face normal
n_k = (sin 0.02 k, 0, cos 0.02 k) — distinct, all towards the camera — and the
frame shows which copy a search kept. Three orders: the normals in forward
order, in reversed order, and the copies' face indices interleaved with the
three displaced faces (another face comes first, and the copies do not sit in
one leaf).

* float64: bit-equal to the brute-force oracle (OracleScene(bvh=False): the
  reference's face loop), frames and Stats, through the SAH and the PLOC
  tree: one lane per pixel (akNone, akGrid 2, RT_FLAG_F64_PER_LANE) and, at
  akGrid 8, one pixel per wave (k_render_px64) with the pixel's face list
  and with the BVH (RT_FLAG_NO_BINNING).
* float32: every kernel variant (test_gpu_split.FLAG_SETS, RT_FLAG_COMPACT)
  through either tree renders, bit for bit, the frame and Stats of the same
  geometry with the lowest copy's normal on EVERY copy — the same tree and
  arithmetic, so any difference is a copy other than the lowest one winning —
  and that frame differs from the one with the last copy's normal everywhere
  (the normals are visible at all)."""
import numpy as np
import pytest

from rtmi import Antialias, Options, Precision, akGrid, akNone, scenes
from rtmi.abi import RT_BVH_PLOC, RT_BVH_SAH, RT_FLAG_COMPACT, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING
from rtmi.renderer import DeviceScene
from rtmi.scene import TriangleMesh
from test_gpu_split import FLAG_SETS
from test_gpu_split import _opts as _opts32

pytestmark = pytest.mark.gpu

K = 64
ORDERS = ("forward", "reversed", "interleaved")
TREES = (RT_BVH_SAH, RT_BVH_PLOC)


def _mesh(order, normals="own"):
    """(scene, copy normals differ). normals: "own" (copy k: n_k in the
    order's sequence), "lowest" / "last": the lowest / highest copy's normal
    on every copy."""
    base = np.array([[-1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 3.0, 0.0]])
    others = [base + [2.5, 0.0, 0.5], base + [-2.5, 0.0, -0.5], base + [0.0, 0.5, 1.0]]
    k = np.arange(K, dtype=np.float64)
    nk = np.stack([np.sin(0.02 * k), np.zeros(K), np.cos(0.02 * k)], axis=1)
    if order == "reversed":
        nk = nk[::-1]
    if normals == "lowest":
        nk = np.tile(nk[0], (K, 1))
    elif normals == "last":
        nk = np.tile(nk[-1], (K, 1))
    other_n = np.array([0.0, 0.0, 1.0])  # the displaced faces' own normal ((v1 - v0) x (v2 - v0), unit)
    # face slots of the three displaced faces
    at = (0, 22, 44) if order == "interleaved" else (K, K + 1, K + 2)
    tris, ns, c, o = [], [], 0, 0
    for f in range(K + 3):
        if f in at:
            tris.append(others[o])
            ns.append(other_n)
            o += 1
        else:
            tris.append(base)
            ns.append(nk[c])
            c += 1
    v = np.concatenate(tris)
    mesh = TriangleMesh(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), normals=np.array(ns))
    return scenes._mesh_scene(mesh, "ties", (0.7, 0.6, 0.5))


def _render(ds, opts):
    import torch
    fb = torch.zeros(opts.height * opts.width * 3, dtype=torch.float32, device="cuda")
    st = ds.render_device(opts, fb)
    return fb, st


@pytest.mark.parametrize("order", ORDERS)
def test_fp64_lowest_face_wins_like_the_brute_force_loop(gpu, oracle_mod, order):
    scene = _mesh(order)
    w, h = 96, 72
    trees = [DeviceScene(scene, bvh_builder=b) for b in TREES]
    # akGrid 8 (64 spp) is the least at which flags 0 / NO_BINNING run
    # k_render_px64 (its own search over the pixel's face list, rt_device.h
    # list_tris, or the BVH inside a one-pixel wave); below that every flag
    # set is the one-lane-per-pixel kernel
    for aa in (Antialias(akNone, 1), Antialias(akGrid, 2), Antialias(akGrid, 8)):
        o = Options(width=w, height=h, antialias=aa, bias=1e-4, precision=Precision.fp64)
        ref, rst, _ = oracle_mod.OracleScene(scene, bvh=False).render(o)
        for ds in trees:
            for flags in (0, RT_FLAG_F64_PER_LANE, RT_FLAG_NO_BINNING):
                o.flags = flags
                fb, st = _render(ds, o)
                got = fb.view(h, w, 3).cpu().numpy()
                assert np.array_equal(got, ref), (order, aa, flags, float(np.abs(got - ref).max()))
                assert st == rst, (order, aa, flags, st, rst)


@pytest.mark.parametrize("m", [16, 2])
@pytest.mark.parametrize("order", ORDERS)
def test_fp32_every_kernel_keeps_the_lowest_face(gpu, order, m):
    import torch
    w, h = 200, 120
    flag_sets = FLAG_SETS + (RT_FLAG_COMPACT,)
    frames = {}
    for normals in ("own", "lowest"):
        scene = _mesh(order, normals)
        for b in TREES:
            ds = DeviceScene(scene, bvh_builder=b)
            for flags in flag_sets:
                frames[normals, b, flags] = _render(ds, _opts32(w, h, m, flags))
    ref_fb, ref_st = frames["lowest", RT_BVH_SAH, 0]
    for key, (fb, st) in frames.items():
        assert st == ref_st, (order, m, key, st, ref_st)
        assert torch.equal(fb, ref_fb), (order, m, key, float((fb - ref_fb).abs().max()))
    last_fb, _ = _render(DeviceScene(_mesh(order, "last")), _opts32(w, h, m))
    assert not torch.equal(last_fb, ref_fb)  # the copies' normals show in the frame
