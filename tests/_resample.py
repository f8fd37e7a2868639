"""The checker of the resampled decode (tests/test_resample.py), independent of the code under test: a numpy implementation of the
rule of include/xpng_hip.h "XPNGHIP_FILTER_TRIANGLE_AA" with the C library's fmaf through ctypes (tests/_kit.py), numpy's fp32 +, -
and /, and the narrowing of tests/_resize.py.  fmaf is never replaced by float64 arithmetic.

    Resampled(raster, rect, flip, OH, OW)    v of the rule for the raster's own channels, computed once
    .bits(word, dtype, scale, bias)           the bit patterns of the caller's buffer for a layout word, reusing v (as Resized)
    .span                                     per axis the first and last source index an output index reads, in the rectangle"""
import numpy as np

from _kit import libm
from _resize import Resized, axis, f32, fmaf


def axis_op(q, n_out, flip):
    """one axis of the rule over q of shape (n, M), fp32: (n_out, M).  The two taps of tests/_resize.py where k <= 1, the clamped
    and renormalised triangle of half-width k where k > 1, its taps accumulated in ascending order"""
    assert q.dtype == np.float32
    n, M = q.shape
    k = f32(n) / f32(n_out)
    assert k.dtype == np.float32
    if not k > f32(1):
        i0, i1, l = axis(n_out, n, flip)
        return fmaf(l[:, None], q[i1] - q[i0], q[i0])
    ik = f32(1) / k
    out = np.empty((n_out, M), f32)
    for o in range(n_out):
        u = n_out - 1 - o if flip else o
        f = f32(libm.fmaf(f32(u) + f32(0.5), k, f32(-0.5)))
        lo, hi = f - k, f + k
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        j0 = int(lo) if lo > 0 else 0
        j1 = min(int(hi), n - 1)
        W, A = f32(0), np.zeros(M, f32)
        for j in range(j0, j1 + 1):
            d = np.abs(f32(j) - f)
            w = max(f32(libm.fmaf(-d, ik, f32(1))), f32(0))
            W = W + w
            A = fmaf(w, q[j], A)
        assert W.dtype == np.float32 and W > 0, (n, n_out, o)
        out[o] = A / W
        assert out.dtype == np.float32
    return out


def span(n_out, n, flip):
    """(first, last) source index, inclusive, that every output index of an axis reads: the two taps or the window"""
    k = f32(n) / f32(n_out)
    if not k > f32(1):
        i0, i1, _ = axis(n_out, n, flip)
        return i0, i1
    u = np.arange(n_out)[::-1] if flip else np.arange(n_out)
    f = fmaf(u.astype(f32) + f32(0.5), k, f32(-0.5))
    lo, hi = f - k, f + k
    return np.where(lo > 0, lo, 0).astype(np.int64), np.minimum(hi.astype(np.int64), n - 1)


class Resampled(Resized):
    """v of the rule for every source channel of `raster` ((h, w, 3|4) uint8), rectangle (x, y, w, h) or None, flip, output size"""

    def __init__(self, raster, rect, flip, OH, OW):
        h, w, px = raster.shape
        rx, ry, rw, rh = rect if rect is not None else (0, 0, w, h)
        assert rw >= 1 and rh >= 1 and rx + rw <= w and ry + rh <= h
        crop = raster[ry:ry + rh, rx:rx + rw].astype(f32)                                   # (rh, rw, px)
        H = axis_op(np.ascontiguousarray(crop.transpose(1, 0, 2)).reshape(rw, rh * px), OW, flip)   # (OW, rh * px): H(s) of every row
        H = np.ascontiguousarray(H.reshape(OW, rh, px).transpose(1, 0, 2)).reshape(rh, OW * px)
        self.v = axis_op(H, OH, False).reshape(OH, OW, px)
        self.span = span(OW, rw, flip) + span(OH, rh, False)                                # (x first, x last, y first, y last)
        self.px, self.OH, self.OW = px, OH, OW
        self._y = {}
