"""What the ray-query comparisons share (test_gpu_query.py, test_gpu_bvh.py,
test_bvh_corpus_cpu.py): the oracle's answers for a batch of rays
(renderer.nim:47-67 trace: brute force over every face), a device batch's
answers, and the comparison: objects and faces equal, t equal bit for bit, the
summed Stats equal."""
import numpy as np

INF = float("inf")


class Ref:
    """The oracle's answers for one batch."""

    def __init__(self, osc, orig, dirs, tnear=None):
        n = len(orig)
        self.obj = np.empty(n, np.int32)
        self.face = np.empty(n, np.int32)
        self.t = np.empty(n, np.float64)
        self.tests = np.zeros(n, np.int64)
        self.hits = np.zeros(n, np.int64)
        o4 = np.concatenate([orig, np.ones((n, 1))], 1)
        d4 = np.concatenate([dirs, np.zeros((n, 1))], 1)
        for i in range(n):
            ob, t, tri, st = osc.trace(o4[i], d4[i], INF if tnear is None else float(tnear[i]))
            self.obj[i], self.t[i], self.face[i] = ob, t, tri if ob >= 0 else -1
            self.tests[i], self.hits[i] = st.numIntersectionTests, st.numIntersectionHits


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


class Got:
    def __init__(self, res, normals=False):
        res = list(res)
        self.t, self.obj, self.face = (np.ascontiguousarray(x.cpu().numpy()) for x in res[:3])
        self.normals = res[3].cpu().numpy() if normals else None
        self.stats = res[-1]

    def raw(self):
        n = b"" if self.normals is None else self.normals.tobytes()
        return self.t.tobytes() + self.obj.tobytes() + self.face.tobytes() + n


def trace(ds, orig, dirs, tnear=None, normals=False, **kw):
    return Got(ds.trace_rays(_dev(orig), _dev(dirs), _dev(tnear), normals=normals, stats=True, **kw), normals)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def check(got, want, sel=None):
    """got == the oracle's answers (for the rays in sel), Stats included."""
    sel = slice(None) if sel is None else sel
    assert np.array_equal(got.obj[sel], want.obj[sel])
    assert np.array_equal(got.face[sel], want.face[sel])
    assert same_bits(got.t[sel], want.t[sel])


def check_stats(got, want, sel=None):
    sel = slice(None) if sel is None else sel
    assert got.stats.numIntersectionTests == int(want.tests[sel].sum())
    assert got.stats.numIntersectionHits == int(want.hits[sel].sum())
    assert got.stats.numPrimaryRays == got.stats.numShadowRays == got.stats.numReflectionRays == 0
