"""The checker of the tone views decodes (tests/test_views_tone.py), independent of the code under test: a numpy statement of the
rule of include/xpng_hip.h "autocontrast, equalise, posterise, solarise and invert per view" on top of the existing checkers for
the values the underlying call hands to the constants (tests/_blur.py Blurred, tests/_affine.py Affine).  Every operation is a
numpy fp32 operation or integer arithmetic; fmaf stays the C library's (tests/_kit.py, through the base classes); nothing is ever
computed in float64.

    NONE, AUTOCONTRAST, EQUALISE, POSTERISE, SOLARISE, INVERT     the ops
    plane(b, steps)                          the steps on one fp32 plane (any shape): entry clamp, then every (op, arg) in order
    Toned(raster, rect, flip, OH, OW, filter, colour=None, blur=None, tone=None)            behind the blur call
    AffineToned(raster, m, OH, OW, filter=0, fill=None, colour=None, tone=None)             behind the affine call
    .retone(steps)                           the same underlying values with other steps
    .bits(word, dtype, scale, bias)          the bit patterns of the caller's buffer for a layout word (as Resized)"""
import numpy as np

from _affine import Affine
from _blur import Blurred
from _resize import f32

NONE, AUTOCONTRAST, EQUALISE, POSTERISE, SOLARISE, INVERT = range(6)


def entry(q):
    """b = q > 0 ? (q > 255 ? 255 : q) : 0, which also turns -0.0 into +0.0"""
    q = np.asarray(q, dtype=f32)
    return np.where(q > f32(0), np.where(q > f32(255), f32(255), q), f32(0)).astype(f32)


def autocontrast(b):
    lo, hi = b.min(), b.max()
    if hi == lo:
        return b
    with np.errstate(over="ignore"):
        s = f32(255) / (hi - lo)                                   # numpy's fp32 division is correctly rounded
    assert s.dtype == np.float32
    if not np.isfinite(s):                                     # hi - lo below about 7.5e-37
        return b
    t = (b - lo) * s                                           # two fp32 array operations: numpy never fuses
    assert t.dtype == np.float32
    return np.where(t > f32(255), f32(255), t).astype(f32)


def equalise(b):
    n = np.rint(b).astype(np.int64)                            # ties to even
    h = np.bincount(n.ravel(), minlength=256)
    last = int(np.nonzero(h)[0][-1])
    step = (b.size - int(h[last])) // 255
    if step == 0:
        return b
    before = np.cumsum(h) - h                                  # h[0] + .. + h[n - 1]
    lut = np.minimum(255, (step // 2 + before) // step).astype(f32)
    return lut[n]


def posterise(b, bits):
    m = f32(2 ** (8 - int(bits)))
    r = b - np.fmod(b, m)
    assert r.dtype == np.float32
    return r


def plane(q, steps):
    b = entry(q)
    for op, arg in steps or ():
        if op == AUTOCONTRAST:
            b = autocontrast(b)
        elif op == EQUALISE:
            b = equalise(b)
        elif op == POSTERISE:
            b = posterise(b, arg)
        elif op == SOLARISE:
            b = np.where(b >= f32(arg), f32(255) - b, b).astype(f32)
        elif op == INVERT:
            b = f32(255) - b
        else:
            assert op == NONE
            break
        assert b.dtype == np.float32
    return b


class _Retone:
    def retone(self, steps):
        """the three colour planes of the underlying values through the steps; alpha untouched.  steps None or empty: nothing"""
        self.v, self._y = self.under.copy(), {}
        if steps:
            for k in range(3):
                self.v[..., k] = plane(self.under[..., k], steps)
        return self


class Toned(_Retone, Blurred):
    def __init__(self, raster, rect, flip, OH, OW, filter, colour=None, blur=None, tone=None):
        Blurred.__init__(self, raster, rect, flip, OH, OW, filter, colour, blur)
        self.under = np.ascontiguousarray(self.v, dtype=f32)
        self.retone(tone)


class AffineToned(_Retone, Affine):
    def __init__(self, raster, m, OH, OW, filter=0, fill=None, colour=None, tone=None):
        Affine.__init__(self, raster, m, OH, OW, filter, fill, colour)
        self.under = np.ascontiguousarray(self.v, dtype=f32)
        self.retone(tone)
