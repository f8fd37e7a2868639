"""The checker of the resized decode (tests/test_resize.py), independent of the code under test: a numpy implementation of the
rule of include/xpng_hip.h "crop, resize and flip" with the C library's fmaf through ctypes, numpy's astype(float16) and torch's
CPU .to(bfloat16) for the narrowing - as tests/test_float_layouts.py does for the float call.  fmaf is never replaced by float64
arithmetic: the last two stages of the rule can round twice that way.

    Resized(raster, rect, flip, OH, OW)      v of the rule for the raster's own channels, computed once
    .bits(word, dtype, scale, bias)           the bit patterns of the caller's buffer for a layout word, reusing v

Also the sentinel arena the GPU tests write into (the one of tests/test_float_layouts.py)."""
import ctypes as C
import ctypes.util

import numpy as np

F16, BF16, F32 = 1, 2, 3
DTYPES = [F16, BF16, F32]
ES = {F16: 2, BF16: 2, F32: 4}
BITS = {F16: np.uint16, BF16: np.uint16, F32: np.uint32}
SENTINEL = 0xA5
LEAD, GUARD = 64, 256
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
_fmaf = np.frompyfunc(_libm.fmaf, 3, 1)
f32 = np.float32


def fmaf(a, b, c):
    """libm's fmaf, element by element with broadcasting, as a float32 array"""
    return np.asarray(_fmaf(a, b, c), dtype=np.float64).astype(np.float32)   # (the doubles hold float32 values: the cast is exact)


def f32_of(x):
    """a Python double rounded once to fp32 (and back to a Python float)"""
    return float(np.float32(x))


def consts_from(mean, std):
    """load_files' formula: scale = float32(1 / (255 std)), bias = float32(-mean / std), in Python doubles rounded once"""
    return [f32_of(1.0 / (255.0 * s)) for s in std], [f32_of(-m / s) for m, s in zip(mean, std)]


def mixed_consts(dtype):
    """four different (scale, bias) pairs, one per channel position: ImageNet's on 0 and 2, two scales whose products with small
    integers are exact rounding ties of the narrow type on 1 and 3 (tests/test_float_layouts.py mixed_consts)"""
    s, b = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    p = (257.0 / 256.0, 259.0 / 256.0) if dtype == BF16 else (2049.0 / 2048.0, 2051.0 / 2048.0)
    return [s[0], p[0], s[2], p[1]], [b[0], 0.0, b[2], 0.0]


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


class Arena:
    """one sentinel-filled device tensor holding a region per image: LEAD + es * (i % 8) sentinel bytes (so the buffers start at
    every multiple of the element size modulo 16), room for `sizes[i]` bytes, GUARD sentinel bytes"""

    def __init__(self, sizes, es):
        import torch
        self.sizes, self.off, total = sizes, [], 0
        for i, n in enumerate(sizes):
            self.off.append(total + LEAD + es * (i % 8))
            total += -(-(LEAD + 8 * es + n + GUARD) // 16) * 16
        self.host0 = np.full(total, SENTINEL, np.uint8)
        self.t = torch.from_numpy(self.host0.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.off]

    def refill(self):
        self.t.fill_(SENTINEL)

    def fetch(self):
        """the bytes of every image, after checking that every other byte still holds the sentinel"""
        import torch
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        mask = np.ones(got.size, bool)
        for o, n in zip(self.off, self.sizes):
            mask[o:o + n] = False
        assert (got[mask] == SENTINEL).all(), "a byte before or behind an image was written"
        return [got[o:o + n] for o, n in zip(self.off, self.sizes)]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), self.host0)
