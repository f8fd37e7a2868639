"""The checker of the resized decode (tests/test_resize.py), independent of the code under test: a numpy implementation of the
rule of include/xpng_hip.h "crop, resize and flip" with the C library's fmaf through ctypes, numpy's astype(float16) and torch's
CPU .to(bfloat16) for the narrowing - as tests/test_float_layouts.py does for the float call.  fmaf is never replaced by float64
arithmetic: the last two stages of the rule can round twice that way.

    Resized(raster, rect, flip, OH, OW)      v of the rule for the raster's own channels, computed once
    .bits(word, dtype, scale, bias)           the bit patterns of the caller's buffer for a layout word, reusing v"""
import numpy as np

from _kit import F16, F32, libm

_fmaf = np.frompyfunc(libm.fmaf, 3, 1)
f32 = np.float32


def fmaf(a, b, c):
    """libm's fmaf, element by element with broadcasting, as a float32 array"""
    return np.asarray(_fmaf(a, b, c), dtype=np.float64).astype(np.float32)   # (the doubles hold float32 values: the cast is exact)


def axis(n_out, n_src, flip):
    """one axis of the rule: (i0, i1, l) for every output index; k is one fp32 division"""
    k = f32(n_src) / f32(n_out)
    assert k.dtype == np.float32
    u = np.arange(n_out, dtype=np.uint32)
    if flip:
        u = np.uint32(n_out - 1) - u
    c = u.astype(f32) + f32(0.5)
    f = fmaf(c, k, f32(-0.5))
    s = np.where(f > 0, f, f32(0)).astype(f32)
    i0 = np.minimum(s.astype(np.uint32), np.uint32(n_src - 1))
    i1 = np.minimum(i0 + np.uint32(1), np.uint32(n_src - 1))
    l = s - i0.astype(f32)
    assert l.dtype == np.float32
    return i0.astype(np.int64), i1.astype(np.int64), l


def narrow(y, dtype):
    """float32 array -> the bit patterns of its round-to-nearest-even conversion to the dtype"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    if dtype == F32:
        return y.view(np.uint32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return y.astype(np.float16).view(np.uint16)
    import torch
    return torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


class Resized:
    """v of the rule for every source channel of `raster` ((h, w, 3|4) uint8), rectangle (x, y, w, h) or None, flip, output size"""

    def __init__(self, raster, rect, flip, OH, OW):
        h, w, px = raster.shape
        rx, ry, rw, rh = rect if rect is not None else (0, 0, w, h)
        assert rw >= 1 and rh >= 1 and rx + rw <= w and ry + rh <= h
        crop = raster[ry:ry + rh, rx:rx + rw].astype(f32)
        x0, x1, lx = axis(OW, rw, flip)
        y0, y1, ly = axis(OH, rh, False)
        self.taps = (x0, x1, y0, y1)
        lx, ly = lx[None, :, None], ly[:, None, None]
        p00, p01, p10, p11 = crop[y0][:, x0], crop[y0][:, x1], crop[y1][:, x0], crop[y1][:, x1]
        a = fmaf(lx, p01 - p00, p00)
        b = fmaf(lx, p11 - p10, p10)
        self.v = fmaf(ly, b - a, a)                                  # (OH, OW, px)
        self.px, self.OH, self.OW = px, OH, OW
        self._y = {}

    def _chan(self, c, bgr, scale, bias):
        """y of the rule for channel position c of the caller's buffer: (OH, OW) float32"""
        s = 3 if c == 3 else (2 - c if bgr else c)
        key = (s, scale, bias)
        if key not in self._y:
            v = np.full((self.OH, self.OW), f32(255)) if s >= self.px else self.v[..., s]
            self._y[key] = fmaf(v, f32(scale), f32(bias))
        return self._y[key]

    def bits(self, word, dtype, scale, bias):
        """the caller's buffer for a layout word as bit patterns: (C, OH, OW) planar, (OH, OW, C) interleaved"""
        planar, bgr, ch = bool(word & 1), bool(word & 2), (word >> 8) or self.px
        y = np.stack([self._chan(c, bgr, float(scale[c]), float(bias[c])) for c in range(ch)], axis=0 if planar else 2)
        return narrow(y, dtype)
