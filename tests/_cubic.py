"""The checker of the cubic views decode (tests/test_cubic.py), independent of the code under test: a numpy implementation of the
rule of include/xpng_hip.h "antialiased bicubic resampling" with the C library's fmaf through ctypes (tests/_kit.py), numpy's fp32
+, - and /, and the narrowing of tests/_resize.py.  fmaf is never replaced by float64 arithmetic.

    Cubic(raster, rect, flip, OH, OW, colour=None)   v of the rule (clamped; with a matrix, R, G, B through it) computed once
    .raw                                      the axis operations' result before the clamp (what shows that the clamp is exercised)
    .bits(word, dtype, scale, bias)           the bit patterns of the caller's buffer for a layout word, reusing v (as Resized)
    .span                                     per axis the first and last source index an output index reads, in the rectangle
    .min_w                                    the smallest W of every window evaluated (each is asserted positive)"""
import numpy as np

from _kit import libm
from _resize import Resized, f32, fmaf


def window(u, k, n):
    """(f, j0, j1) of output index u of an axis of n source pixels with ratio k, all fp32"""
    f = f32(libm.fmaf(f32(u) + f32(0.5), k, f32(-0.5)))
    s = k if k > f32(1) else f32(1)
    r = s + s
    lo, hi = f - r, f + r
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return f, (int(lo) if lo > 0 else 0), min(int(hi), n - 1)


def weight(j, f, inv):
    """Keys' cubic, a = -0.5, at tap j of a window centred at f; inv is the inverse of the stretch"""
    d = np.abs(f32(j) - f)
    t = f32(libm.fmaf(d, inv, f32(0)))
    if t < f32(1):
        return f32(libm.fmaf(libm.fmaf(libm.fmaf(f32(1.5), t, f32(-2.5)), t, f32(0)), t, f32(1)))
    if t < f32(2):
        return f32(libm.fmaf(libm.fmaf(libm.fmaf(f32(-0.5), t, f32(2.5)), t, f32(-4)), t, f32(2)))
    return f32(0)


def axis_op(q, n_out, flip):
    """one axis of the rule over q of shape (n, M), fp32: ((n_out, M), the smallest W).  The same window whatever the ratio, its
    taps accumulated in ascending order"""
    assert q.dtype == np.float32
    n, M = q.shape
    k = f32(n) / f32(n_out)
    assert k.dtype == np.float32
    inv = f32(1) / k if k > f32(1) else f32(1)
    out = np.empty((n_out, M), f32)
    least = f32(np.inf)
    for o in range(n_out):
        f, j0, j1 = window(n_out - 1 - o if flip else o, k, n)
        assert 0 <= j0 <= j1 <= n - 1
        W, A = f32(0), np.zeros(M, f32)
        for j in range(j0, j1 + 1):
            w = weight(j, f, inv)
            W = W + w
            A = fmaf(w, q[j], A)
        assert W.dtype == np.float32 and W > 0, (n, n_out, o)
        least = min(least, W)
        out[o] = A / W
        assert out.dtype == np.float32
    return out, least


def span(n_out, n, flip):
    """(first, last) source index, inclusive, that every output index of an axis reads"""
    k = f32(n) / f32(n_out)
    w = [window(n_out - 1 - o if flip else o, k, n) for o in range(n_out)]
    return np.array([a for (_, a, _) in w], np.int64), np.array([b for (_, _, b) in w], np.int64)


class Cubic(Resized):
    """v of the rule for every source channel of `raster` ((h, w, 3|4) uint8), rectangle (x, y, w, h) or None, flip, output size;
    colour: None or 12 numbers, the matrix that R, G, B go through after the clamp"""

    def __init__(self, raster, rect, flip, OH, OW, colour=None):
        h, w, px = raster.shape
        rx, ry, rw, rh = rect if rect is not None else (0, 0, w, h)
        assert rw >= 1 and rh >= 1 and rx + rw <= w and ry + rh <= h
        crop = raster[ry:ry + rh, rx:rx + rw].astype(f32)                                   # (rh, rw, px)
        H, wx = axis_op(np.ascontiguousarray(crop.transpose(1, 0, 2)).reshape(rw, rh * px), OW, flip)   # (OW, rh * px): H(s) of every row
        H = np.ascontiguousarray(H.reshape(OW, rh, px).transpose(1, 0, 2)).reshape(rh, OW * px)
        raw, wy = axis_op(H, OH, False)
        self.raw = raw.reshape(OH, OW, px)
        self.min_w = min(wx, wy)
        self.clamped = np.where(self.raw < 0, f32(0), np.where(self.raw > 255, f32(255), self.raw)).astype(f32)
        self.span = span(OW, rw, flip) + span(OH, rh, False)                                # (x first, x last, y first, y last)
        self.px, self.OH, self.OW = px, OH, OW
        self.recolour(colour)

    def recolour(self, colour):
        """the same resampling with another matrix (None: none): only the colour step is redone"""
        self.v = self.clamped
        self._y = {}
        if colour is None:
            return self
        m = np.asarray(colour, dtype=np.float32).reshape(3, 4)
        c = self.clamped
        self.v = c.copy()
        for k in range(3):
            x = fmaf(m[k][0], c[..., 0], fmaf(m[k][1], c[..., 1], fmaf(m[k][2], c[..., 2], m[k][3])))
            self.v[..., k] = np.where(x < 0, f32(0), np.where(x > 255, f32(255), x))
        return self
