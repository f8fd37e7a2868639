"""The checker of the staging from tensors (tests/test_store_tensors.py), independent of the code under test: a numpy implementation
of the quantisation rule of include/xpng_hip.h "staged batch from device tensors" with the C library's fmaf through ctypes, as
tests/_resize.py does for the resized decode.  fmaf is never replaced by float64 arithmetic.

    widen(bits, dtype)                        the elements of a buffer, given as bit patterns, as float32 (exact)
    quantize(x, scale, bias)                  the rule for float32 x and one (scale, bias) pair -> uint8
    stage(bits, npx, C, word, dtype, s, b)    the interleaved R,G,B[,A] bytes of a tight buffer in a layout: (npx, C) uint8
    pack(raster, word)                        an (h, w, C) array of elements in the file's order -> the tight buffer of a layout
"""
import numpy as np

from _kit import BF16, F16, F32  # noqa: F401  (the dtype codes of the library)
from _resize import f32, fmaf  # (libm's fmaf)

U8 = 0
DTYPES = [U8, F16, BF16, F32]
ES = {U8: 1, F16: 2, BF16: 2, F32: 4}
BITS = {U8: np.uint8, F16: np.uint16, BF16: np.uint16, F32: np.uint32}
PLANAR, BGR = 1, 2


def widen(bits, dtype):
    """bit patterns of the elements -> float32: f16 and bf16 widen exactly, subnormals kept"""
    bits = np.ascontiguousarray(bits, dtype=BITS[dtype])
    if dtype == F32:
        return bits.view(np.float32)
    if dtype == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def quantize(x, scale, bias):
    """y = fmaf(x, scale, bias); NaN or y <= 0 -> 0; y >= 255 -> 255; else round half to even"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size > 4096:                                                # a large array: fmaf once per distinct bit pattern
        u, inv = np.unique(x.view(np.uint32).reshape(-1), return_inverse=True)   # (on the bits: NaNs and -0 stay what they are)
        if u.size <= x.size // 2:
            return quantize(u.view(np.float32).reshape(-1, 1), scale, bias).reshape(-1)[inv.reshape(-1)].reshape(x.shape)
    y = fmaf(x, f32(scale), f32(bias))
    out = np.zeros(y.shape, np.uint8)
    mid = (y > 0) & (y < 255)                                        # (NaN fails both)
    out[mid] = np.rint(y[mid]).astype(np.uint8)                      # numpy's rint rounds half to even
    out[y >= 255] = 255
    return out


def caller_pos(c, bgr):
    """position in the caller's buffer of the file's channel c (R, G, B, A): alpha is always last"""
    return 2 - c if bgr and c < 3 else c


def stage(bits, npx, C, word, dtype, scale=None, bias=None):
    """the (npx, C) uint8 bytes, file order, of a tight buffer of C * npx elements given as bit patterns"""
    bits = np.ascontiguousarray(bits, dtype=BITS[dtype]).reshape(-1)
    assert bits.size == C * npx
    chan = bits.reshape(C, npx) if word & PLANAR else bits.reshape(npx, C).T   # [position in the caller's buffer][pixel]
    scale = [1.0] * 4 if scale is None else scale
    bias = [0.0] * 4 if bias is None else bias
    out = np.empty((npx, C), np.uint8)
    for c in range(C):
        cc = caller_pos(c, word & BGR)
        out[:, c] = chan[cc] if dtype == U8 else quantize(widen(chan[cc], dtype), scale[cc], bias[cc])
    return out


def pack(raster, word):
    """(h, w, C) elements in the file's order -> the tight buffer of the layout (a contiguous array)"""
    C = raster.shape[2]
    r = raster[..., [caller_pos(c, word & BGR) for c in range(C)]]   # (caller_pos is its own inverse)
    return np.ascontiguousarray(r.transpose(2, 0, 1) if word & PLANAR else r)


def inverse_consts(mean, std):
    """store_files' formula: scale = float32(255 std), bias = float32(255 mean), in Python doubles rounded once; four of each"""
    m, s = list(mean) + [0.0] * (4 - len(mean)), list(std) + [1.0] * (4 - len(std))
    return [float(np.float32(255.0 * x)) for x in s], [float(np.float32(255.0 * x)) for x in m]
