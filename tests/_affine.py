"""The checker of the affine views decode (tests/test_views_affine.py), independent of the code under test: a numpy implementation
of the rule of include/xpng_hip.h "an affine map per view" with the C library's fmaf through ctypes (tests/_kit.py), numpy's fp32
+ and -, and the narrowing of tests/_resize.py.  fmaf is never replaced by float64 arithmetic.

    footprint(dim, m, OH, OW)                  (x, y, w, h) of F in exact rational arithmetic, (0, 0, 0, 0) when empty
    tiles(dims, view_image, mats, sizes)       the launch list, restated plainly from the footprints and shard.tile_table
    Affine(raster, m, OH, OW, filter=0, fill=None, colour=None)   v of the rule, computed once
    .bits(word, dtype, scale, bias)            the bit patterns of the caller's buffer for a layout word, reusing v (as Resized)
    .reads                                     the (x, y) taps that read the raster: all inside F"""
import math
from fractions import Fraction

import numpy as np

from _resize import Resized, f32, fmaf

NEAREST = 3


def footprint(dim, m, OH, OW):
    """F of the header: the corners exactly (a float is a rational), floor - 1 and floor + 2, clipped to the image"""
    W, H = dim
    m = [Fraction(float(np.float32(v))) for v in np.asarray(m, dtype=np.float64).reshape(6)]
    lo, hi = [], []
    for a in range(2):
        s = [m[3 * a] * (ox + Fraction(1, 2)) + m[3 * a + 1] * (oy + Fraction(1, 2)) + m[3 * a + 2] - Fraction(1, 2)
             for ox in (0, OW - 1) for oy in (0, OH - 1)]
        lo.append(math.floor(min(s)) - 1)
        hi.append(math.floor(max(s)) + 2)
    x0, x1, y0, y1 = max(lo[0], 0), min(hi[0], W - 1), max(lo[1], 0), min(hi[1], H - 1)
    if x0 > x1 or y0 > y1:
        return (0, 0, 0, 0)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def tiles(dims, view_image, mats, sizes):
    """indices into the concatenated table (images in order, each tile_table's) of the tiles that intersect the footprint of some
    view of their image, by decreasing pixel count, equal sizes in table order; sizes[v] = (OH, OW)"""
    from xpng_amd.shard import tile_table
    table, first = [], []
    for (w, h) in dims:
        first.append(len(table))
        table += list(tile_table(w, h))
    first.append(len(table))
    keep = set()
    for v, m in enumerate(mats):
        i = v if view_image is None else view_image[v]
        fx, fy, fw, fh = footprint(dims[i], m, *sizes[v])
        if not fw or not fh:
            continue
        for t in range(first[i], first[i + 1]):
            x, y, tw, th = table[t]
            if x < fx + fw and fx < x + tw and y < fy + fh and fy < y + th:
                keep.add(t)
    order = sorted(range(len(table)), key=lambda t: (-table[t][2] * table[t][3], t))
    return [t for t in order if t in keep]


class Affine(Resized):
    """v of the rule for every source channel of `raster` ((h, w, 3|4) uint8) under the inverse matrix m, for an (OH, OW) output"""

    def __init__(self, raster, m, OH, OW, filter=0, fill=None, colour=None):
        h, w, px = raster.shape
        m = np.asarray(m, dtype=np.float64).reshape(6).astype(f32)
        fl = np.zeros(4, f32) if fill is None else np.asarray(fill, dtype=f32)
        fx, fy, fw, fh = footprint((w, h), m, OH, OW)
        X = (np.arange(OW, dtype=np.uint32).astype(f32) + f32(0.5))[None, :]
        Y = (np.arange(OH, dtype=np.uint32).astype(f32) + f32(0.5))[:, None]
        sx = fmaf(m[0], X, fmaf(m[1], Y, m[2])) - f32(0.5)
        sy = fmaf(m[3], X, fmaf(m[4], Y, m[5])) - f32(0.5)
        assert sx.dtype == np.float32 and sy.dtype == np.float32 and sx.shape == (OH, OW)
        src = raster.astype(f32)
        reads = []

        def q(j, i):
            """the taps (j, i), int64 arrays of (OH, OW): (OH, OW, px) fp32"""
            inside = (j >= fx) & (j < fx + fw) & (i >= fy) & (i < fy + fh)
            reads.append((j[inside], i[inside]))
            out = np.broadcast_to(fl[:px], (OH, OW, px)).copy()
            out[inside] = src[i[inside], j[inside]]
            return out

        if filter == NEAREST:
            v = q(np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64))     # (numpy's rint: ties to even)
        else:
            x0, y0 = np.floor(sx), np.floor(sy)
            lx, ly = (sx - x0)[..., None], (sy - y0)[..., None]
            assert lx.dtype == np.float32
            j, i = x0.astype(np.int64), y0.astype(np.int64)
            q00, q10, q01, q11 = q(j, i), q(j + 1, i), q(j, i + 1), q(j + 1, i + 1)
            t = fmaf(lx, q10 - q00, q00)
            u = fmaf(lx, q11 - q01, q01)
            v = fmaf(ly, u - t, t)
        self.reads = (np.concatenate([a for a, _ in reads]), np.concatenate([b for _, b in reads]))
        self.foot = (fx, fy, fw, fh)
        self.sx, self.sy = sx, sy
        self.raw = v
        self.px, self.OH, self.OW = px, OH, OW
        self.recolour(colour)

    def recolour(self, colour):
        """the same sampling with another colour matrix (None: none)"""
        self.v = self.raw
        self._y = {}
        if colour is None:
            return self
        cm = np.asarray(colour, dtype=np.float32).reshape(3, 4)
        c = self.raw
        self.v = c.copy()
        for k in range(3):
            x = fmaf(cm[k][0], c[..., 0], fmaf(cm[k][1], c[..., 1], fmaf(cm[k][2], c[..., 2], cm[k][3])))
            self.v[..., k] = np.where(x < 0, f32(0), np.where(x > 255, f32(255), x))
        return self
