"""The host model of the float64 feature buffers (include/rtmi.h
rt_aov_buffers64): the sample positions of an RT_FP64 frame and the reduction
of per-sample hits to the six channels, a numpy loop in sample order from +0.
Shared by test_aov64_model_cpu.py (the model over the oracle's hits, on the
CPU) and test_gpu_aov64.py (the model over rt_pick_pixels' hits, compared
with the kernels byte for byte)."""
import numpy as np

import coverage_scenes as cs

CHANNELS = ("alpha", "depth", "object", "face", "normal", "albedo")


def sample_positions(w, h, kind, m, seed=0):
    """(h, w, spp, 2) float64: the image position of sample s of pixel (x, y),
    x + sx[s] and y + sy[s] with the offsets of coverage_scenes.pixel_offsets
    (grid(): i * (1/m) + (1/m) * 0.5 in float64; the stochastic kinds: the
    oracle's table of that pixel)."""
    spp = cs.spp_of(kind, m)
    xy = np.empty((h, w, spp, 2), np.float64)
    if kind in cs.STOCHASTIC:
        for y in range(h):
            for x in range(w):
                sx, sy = cs.pixel_offsets(kind, m, seed, x, y)
                xy[y, x, :, 0] = x + sx
                xy[y, x, :, 1] = y + sy
    else:
        sx, sy = cs.pixel_offsets(kind, m, seed, 0, 0)
        xy[..., 0] = np.arange(w, dtype=np.float64)[None, :, None] + sx[None, None, :]
        xy[..., 1] = np.arange(h, dtype=np.float64)[:, None, None] + sy[None, None, :]
    return xy


def scene_albedo(scene):
    """(nobj, 3) float64: every object's albedo as given."""
    return np.array([[float(c) for c in ob.material.albedo][:3] for ob in scene.objects], np.float64).reshape(-1, 3)


def reduce_samples(t, obj, face, nrm, albedo):
    """The six channels of the pixels whose samples' hits are t, obj, face
    (..., spp) and nrm (..., spp, 3), sample s at index s; albedo: (nobj, 3).
    alpha = hits * (1 / spp); depth, object, face: the sample with the
    smallest (t, s); normal, albedo: from +0, plus the value of every hitting
    sample for s = 0 .. spp - 1 in that order, times 1 / spp once."""
    t = np.asarray(t, np.float64)
    obj = np.asarray(obj)
    face = np.asarray(face)
    nrm = np.asarray(nrm, np.float64)
    spp = t.shape[-1]
    hit = obj >= 0
    inv_len = np.float64(1.0) / np.float64(spp)
    out = {"alpha": hit.sum(axis=-1).astype(np.float64) * inv_len}
    tk = np.where(hit, t, np.inf)
    win = np.argmin(tk, axis=-1)[..., None]  # the first smallest: the lowest sample index on equal t
    out["depth"] = np.take_along_axis(tk, win, -1)[..., 0]
    any_hit = hit.any(axis=-1)
    out["object"] = np.where(any_hit, np.take_along_axis(obj, win, -1)[..., 0], -1).astype(np.int32)
    out["face"] = np.where(any_hit, np.take_along_axis(face, win, -1)[..., 0], -1).astype(np.int32)
    alb = np.asarray(albedo, np.float64).reshape(-1, 3)
    alb = alb[np.maximum(obj, 0)] if alb.size else np.zeros(obj.shape + (3,))
    nsum = np.zeros(t.shape[:-1] + (3,), np.float64)  # +0
    asum = np.zeros(t.shape[:-1] + (3,), np.float64)
    for s in range(spp):
        hs = hit[..., s, None]
        nsum = np.where(hs, nsum + nrm[..., s, :], nsum)
        asum = np.where(hs, asum + alb[..., s, :], asum)
    out["normal"] = nsum * inv_len
    out["albedo"] = asum * inv_len
    return out
