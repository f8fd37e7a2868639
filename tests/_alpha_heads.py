"""Single-tile RGBA rasters whose alpha planes are chosen against the alpha reconstruction of the level-1 decode, and the plain
rules they are judged by (test infrastructure).

The decode rebuilds alpha from its symbols in two forms (xpng_amd/csrc/m1_decode.hpp).  k_dec_resid<4, THREADS, true> (FOLD) walks
a tile in raster order, 4 * THREADS pixels per iteration, a lane owning four consecutive pixels; a row start inside a lane's four
pixels is a HEAD, at position hk = 0 .. 3 of the lane.  Column 0 comes from a prologue of THREADS rows per iteration; every other
pixel from one running sum that is never reset and the offset of the latest head, which travels through a wave scan, an LDS record
per wavefront and two bytes carried from iteration to iteration.  k_dec_alpha<THREADS> (the plane form) has the same prologue and
then scans rows that start at any byte alignment.  Everything is mod 256.

The sizes put heads into every lane (width 4), at every hk into lanes 0 and 63 and into the last thread of either workgroup size
(odd widths with enough rows), leave whole wavefronts without a head (widths above 256 and above 1024), make the prologue and the
walk take one and several iterations in both forms, and end tiles at every n mod 4.  The alpha kinds put wrapping sums, the
largest deltas, hidden heads, hidden row ends and visible-only heads onto those geometries.  tests/test_alpha_heads.py proves
from the oracle that every raster is one coded tile, takes a census of what the catalogue holds, and runs it on the GPU.

The rules here are written from the format (libxpng.c:798-800: alpha is predicted from the left neighbour, in column 0 from the
pixel above), not from the kernels.  No RNG library: every value is the integer hash of xpng_amd/synth.py, keyed by the raster's name."""
import zlib

import numpy as np

from xpng_amd.synth import _hash_np

THREADS = (256, 1024)                         # the two workgroup sizes of k_dec_resid and k_dec_alpha
SPT = 10                                      # (tile, stream) items of an RGBA tile at level 1

# (w, h): n = 4400 5155 2058 4193 4410 1088 4355 1285 1290 1295 1300 9243 16396; n mod 4 = 0 3 2 1 2 0 3 1 2 3 0 3 0
SIZES = [(4, 1100), (5, 1031), (6, 343), (7, 599), (63, 70), (64, 17), (65, 67), (257, 5), (258, 5), (259, 5), (260, 5), (1027, 9),
         (4099, 4)]
BATCH_SIZES = [(5, 1031), (1027, 9)]          # narrow and tall, wide and flat: the uniform batches of the GPU tests
KINDS = ("rand", "zeros", "col0_wrap", "row_wrap", "extremes", "hidden_heads", "only_heads", "hidden_row_ends", "tail")
# only_heads is visible in column 0 alone.  The third wrong rule (below) shows only where a visible pixel stands in front of a
# multiple of 4 * THREADS that is no row start: in column 0, that is where w divides 1024 k - 1 (4095 = 5 * 819 = 7 * 585 = 63 * 65).
# At widths 4 and 64 every multiple of 1024 is a row start and the rule cannot show on any plane.
ONLY_HEADS_WIDTHS = (4, 5, 7, 63, 64, 65)
EXTREME_DELTAS = (-128, 127, -1)              # zig-zag symbols 0xFF, 0xFE, 1


def _seed(name):
    return zlib.crc32(name.encode()) & 0xFFFFF


def _noise(name, w, h, c):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    return (_hash_np(xs, ys, c, _seed(name)) >> np.uint64(8)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the alpha planes
def alpha_plane(kind, w, h, name):
    """(h, w) int64 alpha of a kind; pixel 0 is visible in every kind"""
    n = w * h
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    i = ys * w + xs
    rand = 1 + _noise(name, w, h, 3) % 255                                         # 1 .. 255
    if kind == "rand":
        a = rand
    elif kind == "zeros":                                                           # 0 .. 255, about 30 % forced to 0 ...
        a = np.where(_noise(name, w, h, 4) % 10 < 3, 0, _noise(name, w, h, 3) % 256)
        a = np.where((i % 1024 == 1023) | (i == 0), a | 1, a)                       # ... but the pixel in front of an iteration stays visible
    elif kind == "col0_wrap":
        # column 0 climbs by 101 a row; the row is flat behind one step of 64 at column 1.  (Entirely flat rows would end on the value
        # they begin with, and taking column 0 from the end of the row above would then give the right plane.)
        c = 200 + 101 * ys
        a = np.where(xs == 0, c, c + 64) & 255
    elif kind == "row_wrap":                                                        # every row climbs by 97 a pixel: 3 steps pass 256
        a = (1 + 53 * ys + 97 * xs) & 255
    elif kind == "extremes":                                                        # in raster order: -128, +127, -1, ...
        d = np.array(EXTREME_DELTAS)[(np.arange(n) - 1) % 3]
        d[0] = 0
        a = ((255 + np.cumsum(d)) & 255).reshape(h, w)
    elif kind == "hidden_heads":                                                    # alpha 0 exactly in column 0 from row 1 on
        a = np.where((xs == 0) & (ys > 0), 0, rand)
    elif kind == "only_heads":                                                      # visible in column 0 alone
        a = np.where(xs == 0, rand, 0)
    elif kind == "hidden_row_ends":                                                 # alpha 0 in the last w mod 4 + 1 pixels of every row
        a = np.where(xs >= w - (w % 4 + 1), 0, rand)
    elif kind == "tail":                                                            # flat, and a varying last row
        a = np.where(ys == h - 1, rand, 200)
    else:
        raise KeyError(kind)
    a = a.astype(np.int64)
    assert a[0, 0] != 0
    return a


def kinds_of(w, h):
    return [k for k in KINDS if k != "only_heads" or w in ONLY_HEADS_WIDTHS]


def names():
    """every raster, in catalogue order"""
    return [f"{kind}_{w}x{h}" for (w, h) in SIZES for kind in kinds_of(w, h)]


def parse(name):
    kind, size = name.rsplit("_", 1)
    w, h = (int(v) for v in size.split("x"))
    return kind, w, h


def of_size(w, h):
    return [nm for nm in names() if nm.endswith(f"_{w}x{h}")]


def mixed_names():
    """the catalogue repeated cyclically until its tiles are more than 2048 (tile, stream) items: a launch of them selects the wide
    chains and the 256-thread kernels by itself"""
    nm = names()
    count = max(len(nm), 2048 // SPT + 1)
    return [nm[j % len(nm)] for j in range(count)]


_cache = {}


def raster(name):
    """The named (h, w, 4) raster (read-only, shared between tests): colour 100 plus two bits of noise, zero under alpha 0, so the
    raster is its own normalize_rgba."""
    if name not in _cache:
        kind, w, h = parse(name)
        a = alpha_plane(kind, w, h, name)
        r = np.zeros((h, w, 4), dtype=np.uint8)
        for c in range(3):
            r[..., c] = np.where(a != 0, 100 + (_noise(name, w, h, c) & 3), 0)
        r[..., 3] = a
        r.setflags(write=False)
        _cache[name] = r
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the plain rules
def zz_dec(s):
    s = np.asarray(s).astype(np.int64)
    return (s >> 1) ^ -(s & 1)


def _deltas(syms, w, h):
    """(h, w) the alpha differences as bytes (0 .. 255); 0 at pixel 0.  syms[i - 1] is the symbol of pixel i."""
    assert len(syms) == w * h - 1
    return np.concatenate([[0], zz_dec(syms) & 255]).reshape(h, w)


def alpha_from_symbols(a0, syms, w, h):
    """(h, w) uint8: every pixel its left neighbour plus its difference, in column 0 the pixel above plus its difference, mod 256"""
    D = _deltas(syms, w, h)
    col = a0 + np.cumsum(D[:, 0])
    row = np.concatenate([np.zeros((h, 1), np.int64), np.cumsum(D[:, 1:], axis=1)], axis=1)
    return ((col[:, None] + row) & 255).astype(np.uint8)


def heads(w, h, threads):
    """The row starts of a w x h tile as the walk of k_dec_resid<4, threads> meets them: per head its row y, its pixel p = y w, the
    iteration, and the thread, wavefront, lane and position hk (0 .. 3) of the lane that owns the pixel."""
    y = np.arange(h)
    p = y * w
    tid = p % (4 * threads) // 4
    return {"y": y, "p": p, "it": p // (4 * threads), "tid": tid, "wave": tid // 64, "lane": tid % 64, "hk": p % 4}


def owner(p, w, threads):
    """(iteration, wave, lane, position in the lane) of pixel p, and the same with hk for the head of its row: for a failure report"""
    def place(q):
        tid = q % (4 * threads) // 4
        return (q // (4 * threads), tid // 64, tid % 64, q % 4)
    return place(p), place(p // w * w)


def restarts(w, h, threads):
    """the multiples of 4 * threads inside the tile that are no row starts: where the walk hands its running sum to the next iteration"""
    r = np.arange(4 * threads, w * h, 4 * threads)
    return r[r % w != 0]


# Three deliberately wrong decoders.  They are here to show that the catalogue can tell them from the right one; nothing decodes with them.
def wrong_col0_from_left(a0, syms, w, h):
    """column 0 takes the pixel in front of it in raster order (the end of the row above) for its neighbour"""
    D = _deltas(syms, w, h)
    return ((a0 + np.cumsum(D.reshape(-1))) & 255).astype(np.uint8).reshape(h, w)


def wrong_saturated(a0, syms, w, h):
    """every sum stops at 255"""
    D = _deltas(syms, w, h)
    out = np.zeros((h, w), np.int64)
    out[0, 0] = a0
    for y in range(1, h):
        out[y, 0] = min(out[y - 1, 0] + D[y, 0], 255)
    for x in range(1, w):
        out[:, x] = np.minimum(out[:, x - 1] + D[:, x], 255)
    return out.astype(np.uint8)


def wrong_restarted(a0, syms, w, h, threads):
    """the running sum starts again from 0 at every multiple of 4 * threads pixels, until the next row start sets it right"""
    T = alpha_from_symbols(a0, syms, w, h).astype(np.int64).reshape(-1)
    off = np.zeros(w * h, np.int64)
    for r in restarts(w, h, threads):
        off[r:(r // w + 1) * w] = T[r - 1]
    return ((T - off) & 255).astype(np.uint8).reshape(h, w)
