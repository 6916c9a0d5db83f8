"""Shared by tests/test_smooth_cpu.py and tests/test_gpu_smooth.py: the arithmetic of mcg_smooth_gaze (include/mcgaze_hip.h) restated in
numpy, one vector at a time; the kernel's table semantics on top of it; the inputs (unit vectors plus 1e-2 noise, fixed seeds); and the
fake engine of tests/test_stream_pool_cpu.py with the one method a lone GazeStream needs in addition."""
import numpy as np

from mcgaze_amd import harness
from tests.test_stream_pool_cpu import FakeEngine

ALPHA = 0.6
F = np.float32


def smooth_vector(x, p, q, alpha=ALPHA):
    """THE SPECIFICATION, for one vector x [3] with the same vector of the previous (p) and next (q) frame, None where there is none.
    Every operation is an f32 numpy scalar operation (numpy contracts nothing); each fma is taken in float64 and rounded once."""
    x = [F(v) for v in x]
    if p is None and q is None:
        return np.array(x, dtype=F)                          # a one-frame stream: x itself, not normalised
    a, b = F(alpha), F(1.0 - float(alpha))
    with np.errstate(all='ignore'):
        if p is not None and q is not None:
            o = []
            for k in range(3):
                v = a * x[k]
                o.append(v + (b * (F(p[k]) + F(q[k]))) / F(2))
        else:
            n = p if p is not None else q
            o = [a * x[k] + b * F(n[k]) for k in range(3)]
        fma = lambda u, w, c: F(np.float64(u) * np.float64(w) + np.float64(c))
        n = np.sqrt(fma(o[2], o[2], fma(o[1], o[1], o[0] * o[0])))
        return np.array([o[k] / n for k in range(3)], dtype=F)


def spec(seq, alpha=ALPHA):
    """The specification over a whole stream: seq [L, ..., 3] f32 (fused [L,3], others [L,3,3], ...) -> the same shape."""
    seq = np.asarray(seq, dtype=F)
    flat = seq.reshape(seq.shape[0], -1, 3)
    out = np.empty_like(flat)
    L = flat.shape[0]
    for t in range(L):
        for v in range(flat.shape[1]):
            out[t, v] = smooth_vector(flat[t, v], flat[t - 1, v] if t > 0 else None, flat[t + 1, v] if t + 1 < L else None, alpha)
    return out.reshape(seq.shape)


def emulate(store, plan, alpha=ALPHA):
    """mcg_smooth_gaze in numpy: store [rows,27], plan [n,3] (previous row, row, next row; -1 = none) -> out [n,12].  A row outside the
    store, or a neighbour that is neither -1 nor inside it, makes the output row NaN."""
    rows = store.shape[0]
    out = np.empty((len(plan), 12), dtype=F)
    inside = lambda r: 0 <= r < rows
    for i, (pr, r, nx) in enumerate(np.asarray(plan).tolist()):
        if not inside(r) or not (pr == -1 or inside(pr)) or not (nx == -1 or inside(nx)):
            out[i] = np.nan
            continue
        for v in range(4):
            at = slice(15 + 3 * v, 18 + 3 * v)
            out[i, 3 * v:3 * v + 3] = smooth_vector(store[r, at], store[pr, at] if pr >= 0 else None, store[nx, at] if nx >= 0 else None, alpha)
    return out


def gaze_sequence(seed, L, shape=()):
    """[L, *shape, 3] f32: unit vectors that drift from frame to frame, plus 1e-2 noise."""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((1,) + tuple(shape) + (3,)) + np.cumsum(0.3 * rs.standard_normal((L,) + tuple(shape) + (3,)), axis=0)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return (v + 1e-2 * rs.standard_normal(v.shape)).astype(F)


def ordered(a):
    """f32 -> int64 that rises with the value, one step per representable number: differences are distances in ulp."""
    i = np.ascontiguousarray(a, dtype=F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def bits(a):
    return np.ascontiguousarray(harness._host(a), dtype=F).view(np.int32)


def chunks(L, sizes):
    """L frames cut by the pattern ``sizes`` (repeated, the last piece cut short) -> [(a, b)]."""
    out, a, i = [], 0, 0
    while a < L:
        b = min(L, a + sizes[i % len(sizes)])
        out.append((a, b))
        a, i = b, i + 1
    return out


class RingFakeEngine(FakeEngine):
    """FakeEngine plus the trunk call of a lone GazeStream (PyramidRing.append): frames into consecutive rows; a ring overwrites the rows
    its stream released, so no row is ever handed back."""

    def backbone_fpn(self, img, out=None, row=0):
        for i, x in enumerate(img):
            self.live.add(row + i)
            self.tag_of_row[row + i] = int(x[0, 0, 0])
        return out
