"""The checker of the blur views decode (tests/test_views_blur.py), independent of the code under test: a numpy statement of the
rule of include/xpng_hip.h "Gaussian blur and solarise per view" with the C library's fmaf through ctypes (tests/_kit.py), numpy's
fp32 +, the existing checkers for the intermediate T (tests/_resize.py for filter 0, tests/_resample.py for filter 1,
tests/_cubic.py for filter 2) and weights from its own float64 formula.  fmaf is never replaced by float64 arithmetic.

    weights(sigma, R)                                       the R + 1 fp32 weights, from the float64 formula
    Blurred(raster, rect, flip, OH, OW, filter, colour=None, blur=None)
                                                            blur = None or (sigma, R, threshold_or_None)
    .T                                                      the intermediate: (OH, OW, px) fp32 in byte units, matrix applied
    .raw                                                    the blur's result before its clamp (colour channels; None without a blur)
    .v                                                      the values before the constants
    .bits(word, dtype, scale, bias)                         the bit patterns of the caller's buffer for a layout word (as Resized)"""
import math

import numpy as np

from _cubic import Cubic
from _resample import Resampled
from _resize import Resized, f32, fmaf


def weights(sigma, R):
    """w[0 .. R]: g[d] = exp(-d^2 / (2 s^2)) in double, S = g[0] + 2 (g[1] + .. + g[R]) summed in ascending d, w[d] = float32(g[d] / S)"""
    s = float(np.float32(sigma))
    g = [math.exp(-float(d * d) / (2.0 * s * s)) for d in range(R + 1)]
    t = 0.0
    for d in range(1, R + 1):
        t += g[d]
    S = g[0] + 2.0 * t
    return np.array([g[d] / S for d in range(R + 1)], dtype=np.float64).astype(np.float32)


def refl(i, n):
    """torch's reflect, on an index array"""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def axis_blur(q, w, R):
    """the axis operation of the rule along the LAST axis of q (fp32): pairs from d = R down to 1, then the centre"""
    assert q.dtype == np.float32 and w.dtype == np.float32 and 1 <= R < q.shape[-1]
    n = q.shape[-1]
    x = np.arange(n)
    A = np.zeros(q.shape, f32)
    for d in range(R, 0, -1):
        pair = q[..., refl(x - d, n)] + q[..., refl(x + d, n)]
        assert pair.dtype == np.float32
        A = fmaf(w[d], pair, A)
    return fmaf(w[0], q, A)


def recoloured(v, colour):
    """the colour matrix of the views-colour call on the first three channels of v, and its clamp"""
    m = np.asarray(colour, dtype=np.float32).reshape(3, 4)
    out = v.copy()
    for k in range(3):
        x = fmaf(m[k][0], v[..., 0], fmaf(m[k][1], v[..., 1], fmaf(m[k][2], v[..., 2], m[k][3])))
        out[..., k] = np.where(x < 0, f32(0), np.where(x > 255, f32(255), x))
    return out


def clamp(a):
    return np.where(a < 0, f32(0), np.where(a > 255, f32(255), a)).astype(f32)


class Blurred(Resized):
    def __init__(self, raster, rect, flip, OH, OW, filter, colour=None, blur=None):
        if filter == 2:
            T = Cubic(raster, rect, flip, OH, OW, colour).v
        else:
            T = (Resampled if filter == 1 else Resized)(raster, rect, flip, OH, OW).v
            if colour is not None:
                T = recoloured(T, colour)
        self.T = np.ascontiguousarray(T, dtype=f32)
        self.px, self.OH, self.OW = raster.shape[2], OH, OW
        self.reblur(blur)

    def reblur(self, blur):
        """the same intermediate with another record: only the second pass is redone"""
        self.v, self.raw, self._y = self.T.copy(), None, {}
        if blur is None:
            return self
        sigma, R, thr = blur
        if R:
            assert R < self.OW and R < self.OH
            w = weights(sigma, R)
            q = np.ascontiguousarray(self.T[..., :3].transpose(2, 0, 1))                    # (3, OH, OW)
            h = axis_blur(q, w, R)                                                          # along x
            a = axis_blur(np.ascontiguousarray(h.transpose(0, 2, 1)), w, R).transpose(0, 2, 1)   # along y, over the horizontal results
            self.raw = np.ascontiguousarray(a.transpose(1, 2, 0))
            self.v[..., :3] = clamp(self.raw)
        if thr is not None:
            b = self.v[..., :3]
            self.v[..., :3] = np.where(b >= f32(thr), f32(255) - b, b)
            assert self.v.dtype == np.float32
        return self
