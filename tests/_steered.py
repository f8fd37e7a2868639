"""Deterministic rasters that steer the encoder into a chosen branch of the format (test infrastructure).

The level-1 / level-2 colour chooser (libxpng.c:92-140) looks only at pixels (4i+3, 4j+3) of a tile and at their left, upper and
upper-left neighbours, so the 2x2 blocks at x % 4 in {2,3}, y % 4 in {2,3} (tile-local) decide the predictor and the other 12 of
every 16 pixels are free.  `steered` builds the sampled blocks so that one wanted predictor wins on every tile, and fills the free
pixels with a compressible background plus sparse outliers that put every (L, U, UL) combination of
{0, 1, 2, 127, 128, 129, 253, 254, 255} in front of some coded interior pixel, in every channel.  `tie` builds sampled blocks whose
costs tie exactly, `gray` builds R == G == B rasters for every level-2 gray mode and block form, and `l2_form` / `alpha_form`
build the rarely written rANS block forms.

No RNG library: every value is the integer hash of xpng_amd/synth.py, so the bytes do not depend on the numpy version.
Everything is tile-local: the tile table below restates libxpng.c:51-83 (the CPU test pins it to the oracle's).
"""
import numpy as np

from xpng_amd.synth import _hash_np

EDGE = np.array([0, 1, 2, 127, 128, 129, 253, 254, 255], dtype=np.int64)
TILE_AREA = 444 * 444


def _split(n, base):
    rem, count, first, second = n % base, n // base, base + n % base, base
    if rem > base // 2:
        count += 1
        second = first // 2
        first = second + (first & 1)
    return count, first, second


def tile_table(W, H):
    """[(x, y, w, h)] in file order (libxpng.c:51-83)."""
    if W * H <= TILE_AREA:
        return [(0, 0, W, H)]
    if W < 444:
        bw, bh = W, TILE_AREA // W
    elif H < 444:
        bh, bw = H, TILE_AREA // H
    else:
        bw = bh = 444
    nx, w0, w1 = _split(W, bw)
    ny, h0, h1 = _split(H, bh)
    xs = [(0, w0)] + [(w0 + (i - 1) * w1 if i == 1 else w0 + w1 + (i - 2) * bw, w1 if i == 1 else bw) for i in range(1, nx)]
    ys = [(0, h0)] + [(h0 + (j - 1) * h1 if j == 1 else h0 + h1 + (j - 2) * bh, h1 if j == 1 else bh) for j in range(1, ny)]
    return [(x, y, w, h) for (y, h) in ys for (x, w) in xs]


def _avg(L, U):
    return (L + U + 1) >> 1


def _grad(L, U, UL):
    return (3 * L + 3 * U - 2 * UL + 2) >> 2


def _h(x, y, c, seed):
    return _hash_np(x, y, c, seed).astype(np.int64)


# (x % 4, y % 4) of the three free pixels that form (L, U, UL) of a free pixel, three such triples per 4x4 cell:
#   slot 0: pixel (1,1): L (0,1)  U (1,0)  UL (0,0)      slot 1: pixel (1,3): L (0,3)  U (1,2)  UL (0,2)
#   slot 2: pixel (3,1): L (2,1)  U (3,0)  UL (2,0)
_ROLE = {(0, 1): (0, 0), (1, 0): (0, 1), (0, 0): (0, 2), (0, 3): (1, 0), (1, 2): (1, 1), (0, 2): (1, 2),
         (2, 1): (2, 0), (3, 0): (2, 1), (2, 0): (2, 2), (1, 1): (0, 3), (1, 3): (1, 3), (3, 1): (2, 3)}  # role 3 = the pixel itself


def _colour(w, h, alpha, seed, block):
    """Common body of `steered` and `tie`: block(a, bi, bj, c) -> (UL, L, U, cur) of the sampled 2x2 blocks, channel c, where a is
    the background level at the block and (bi, bj) its cell."""
    ch = 3 + int(alpha)
    out = np.zeros((h, w, ch), dtype=np.uint8)
    tiles = tile_table(w, h)
    n_slots = 3 * sum((tw // 4) * (th // 4) for (_, _, tw, th) in tiles)
    stride = max(8, n_slots // 2200)          # about three rounds of the 729 combinations; at most 1 triple in 8 slots
    if stride % 3 == 0:
        stride += 1                           # (a multiple of 3 would use slot 0 of the cells only)
    base = 0
    for ti, (tx, ty, tw, th) in enumerate(tiles):
        sd = seed * 977 + ti * 131
        ly, lx = np.meshgrid(np.arange(th, dtype=np.int64), np.arange(tw, dtype=np.int64), indexing="ij")
        ux, uy = lx.astype(np.uint64), ly.astype(np.uint64)
        bi, bj = lx >> 2, ly >> 2
        ncx, ncy = tw // 4, th // 4
        incell = (bi < ncx) & (bj < ncy)
        mx, my = lx & 3, ly & 3
        sampled = incell & (mx >= 2) & (my >= 2)
        # free pixels: which slot of their cell they belong to, and in which role
        k = np.full(lx.shape, -1, dtype=np.int64)
        role = np.zeros(lx.shape, dtype=np.int64)
        for (ax, ay), (kk, rr) in _ROLE.items():
            m = (mx == ax) & (my == ay)
            k[m], role[m] = kk, rr
        slot = (base + bj * ncx + bi) * 3 + k
        used = incell & (k >= 0) & (slot % stride == stride // 2)
        u = slot // stride
        keep = sampled | used                 # pixels whose colour must survive an alpha of zero
        single = (_h(ux, uy, 5, sd) % 97 == 0) & ~sampled & ~used
        tile = np.zeros((th, tw, ch), dtype=np.int64)
        for c in range(3):
            def bg(x, y, noise):
                t = (x * (c + 1) + y * (3 - c)) >> 4
                return 96 + 8 * c + np.abs((t % 128) - 64) + noise
            v = bg(lx, ly, _h(ux, uy, c, sd) & 1)
            q = (u + 243 * c) % 729
            trip = np.where(role == 0, EDGE[q // 81], np.where(role == 1, EDGE[(q // 9) % 9], EDGE[q % 9]))
            v = np.where(single, EDGE[(_h(ux, uy, 6, sd) >> 8) % 9], v)
            v = np.where(used & (role < 3), trip, v)
            a = bg(4 * bi + 2, 4 * bj + 2, 0)
            UL, L, U, cur = block(a, bi.astype(np.uint64), bj.astype(np.uint64), c, sd)
            blk = np.where(my == 2, np.where(mx == 2, UL, U), np.where(mx == 2, L, cur))
            tile[..., c] = np.where(sampled, blk, v)
        if alpha:
            t = _h(ux >> np.uint64(5), uy >> np.uint64(5), 7, sd) & 3
            al = np.where(t == 0, 0, np.where(t == 1, ((lx + ly) & 255) | 1, 255))
            al = np.where((ly & 31) >> 1 == 2, 0, al)              # rows 4, 5 of every 32: a transparent run across the row end
            al[0, max(0, tw - 5):] = 0                             # ... and on rows 0 / 1, for tiles of fewer than six rows
            al[1, :3] = 0
            al = np.where(keep, np.maximum(al, 1), al)
            tile[..., 3] = al
            tile[al == 0] = 0
        assert tile.min() >= 0 and tile.max() <= 255
        out[ty:ty + th, tx:tx + tw] = tile.astype(np.uint8)
        base += ncx * ncy
    return out


def _block_for(pr):
    """Sampled block that makes predictor pr the strict minimum: UL = a - 64 puts avg and gradient 32 apart; the residual is
    -1..1 per channel (no green) or a shared -1 / +1 on green with -2 / +2 on red and blue (green-subtract one bit cheaper)."""
    def block(a, bi, bj, c, sd):
        UL = a - 64
        L = a + (_h(bi, bj, c, sd + 11) & 1)
        U = a + (_h(bi, bj, c, sd + 12) & 1)
        pred = _grad(L, U, UL) if pr & 2 else _avg(L, U)
        hh = _h(bi, bj, 9, sd)
        if pr & 1:
            neg = np.where(c == 1, -1, np.where((c == 2) & ((hh >> 1) & 1 == 1), -1, -2))
            pos = 1 if c == 1 else 2
            d = np.where(hh & 1 == 1, neg, pos)
        else:
            fixed = (1, -1, 0)[c] if c < 2 else ((hh >> 1) % 3) - 1
            d = np.where(hh & 1 == 1, fixed, (_h(bi, bj, c, sd + 13) % 3) - 1)
        return UL, L, U, pred + d
    return block


def steered(pr, w, h, alpha, seed=1):
    """(h, w, 3|4) uint8 raster on which the chooser returns predictor pr (0 avg, 1 avg+green, 2 gradient, 3 gradient+green)
    for every tile."""
    return _colour(w, h, alpha, seed, _block_for(pr))


TIES = {"all": 0, "avg": 0, "grad": 2, "green": 1}   # kind -> the predictor that must win (first minimum)


def tie(kind, w, h, alpha, seed=1):
    """Sampled blocks whose costs tie exactly:  all: 0 = 1 = 2 = 3 (flat blocks);  avg: 0 = 1 < 2 = 3 (the pixel is its average
    prediction, the gradient is 32 off);  grad: 2 = 3 < 0 = 1;  green: 1 = 3 < 0 = 2 (flat neighbourhood, so both predictions
    agree, residual (-2, -1, -2))."""
    def block(a, bi, bj, c, sd):
        if kind == "all":
            return a, a, a, a
        if kind == "green":
            return a, a, a, a + (-2, -1, -2)[c]
        UL = a - 64
        L = a + (_h(bi, bj, c, sd + 11) & 1)
        U = a + (_h(bi, bj, c, sd + 12) & 1)
        return UL, L, U, (_avg(L, U) if kind == "avg" else _grad(L, U, UL))
    return _colour(w, h, alpha, seed, block)


def edge_combinations(raster):
    """Per channel, the set of (L, U, UL) triples drawn from EDGE that stand in front of a CODED tile-interior pixel."""
    h, w, ch = raster.shape
    r = raster.astype(np.int64)
    code = np.full(256, -1, dtype=np.int64)
    code[EDGE] = np.arange(9)
    found = [set(), set(), set()]
    for (tx, ty, tw, th) in tile_table(w, h):
        t = r[ty:ty + th, tx:tx + tw]
        coded = t[1:, 1:, 3] != 0 if ch == 4 else np.ones((th - 1, tw - 1), dtype=bool)
        for c in range(3):
            L, U, UL = code[t[1:, :-1, c]], code[t[:-1, 1:, c]], code[t[:-1, :-1, c]]
            m = coded & (L >= 0) & (U >= 0) & (UL >= 0)
            found[c].update(np.unique(L[m] * 81 + U[m] * 9 + UL[m]).tolist())
    return found


# ------------------------------------------------------------------------------------------------ gray (level 2)
# kind -> the tile type byte the encoder must write.
#   left / up / avg / grad / raw : the five gray modes.
#   one  : v = x + y.  "left" leaves the residual 1 everywhere (row 0 and column 0 too): a one-symbol (type 1) block.
#   tie_lua : v = f(x + y), so L == U at every interior pixel: the left, up and average candidates are the SAME symbol stream
#             (avg(L, L) = L) and tie exactly; the gradient candidate is larger.  First minimum: left (0x20).
#   tie_ug  : every column constant, neighbouring columns -2..+1 apart (L - U in -2..1): the gradient prediction
#             (3L + 3U - 2L + 2) >> 2 equals U there, so the up and gradient candidates are the SAME stream and tie exactly;
#             left and average are larger.  First minimum: up (0x21).
#   Row 0 and column 0 carry the same symbol in all four candidates, so "same interior" means "same stream".
GRAY = {"left": 0x20, "up": 0x21, "avg": 0x22, "grad": 0x23, "raw": 0x28, "one": 0x20, "tie_lua": 0x20, "tie_ug": 0x21}
GRAY_TIES = {"tie_lua": (0, 1, 2), "tie_ug": (1, 3)}   # the candidates that tie


def gray(kind, w, h, seed=1):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    x, y = xs.astype(np.int64), ys.astype(np.int64)
    z = np.zeros_like(xs)
    if kind in ("left", "up"):
        line = ys if kind == "left" else xs
        v = _h(z, line, 0, seed) >> 24
        v = np.where(_h(xs, ys, 1, seed) % 50 == 0, _h(xs, ys, 2, seed) >> 24, v)
    elif kind == "avg":
        v = 100 + (_h(xs, ys, 0, seed) & 7)
    elif kind == "grad":
        if w >= 32:
            v = ((x * y) // 97 + (_h(xs, ys, 0, seed) & 1)) & 255
        else:  # a few columns only: v = x s(y) + B(y).  left leaves s (0..31), up leaves B' (-23..23), the damped gradient (B' + s) / 4
            v = x * np.abs(((y // 4) % 62) - 31) + _h(z, ys, 0, seed) % 24
    elif kind == "raw":
        v = _h(xs, ys, 0, seed) >> 24
    elif kind == "one":
        v = (x + y) & 255
    elif kind == "tie_lua":
        t = xs + ys
        v = (t.astype(np.int64) * 3 + (_h(t, z, 0, seed) & 7)) & 255
    elif kind == "tie_ug":
        col, c = np.empty(w, dtype=np.int64), 128
        hs = _h(np.arange(w, dtype=np.uint64), np.zeros(w, dtype=np.uint64), 0, seed)
        down = False
        for i in range(w):
            step = -1 if down else int(hs[i] % 4) - 1  # L - U = c(x-1) - c(x) must lie in -2..1: steps of -1..2 only
            c += step
            down = c > 240 or (down and c > 16)        # (the hashed steps drift upwards; walk back down before the byte wraps)
            col[i] = c
        v = np.broadcast_to(col[None, :], (h, w))
    else:
        raise ValueError(kind)
    return np.repeat(np.asarray(v, dtype=np.int64).astype(np.uint8)[..., None], 3, axis=2)


def gray_candidates(raster):
    """The four candidate symbol streams (left, up, average, gradient) of a one-tile gray raster (libxpng.c:583-604)."""
    v = raster[..., 0].astype(np.int64)
    L, U, UL = v[1:, :-1], v[:-1, 1:], v[:-1, :-1]
    out = []
    for pred in (L, U, _avg(L, U), _grad(L, U, UL)):
        d = np.zeros_like(v)
        d[0, 1:] = v[0, 1:] - v[0, :-1]
        d[1:, 0] = v[1:, 0] - v[:-1, 0]
        d[1:, 1:] = v[1:, 1:] - pred
        d = ((d + 128) & 255) - 128
        out.append(np.where(d < 0, -2 * d - 1, 2 * d).astype(np.uint8).ravel()[1:])
    return out


def mixed_gray(seed=1):
    """1000 x 900 RGB, four tiles: gray "left", steered colour (predictor 3), gray "gradient", one colour."""
    r = steered(3, 1000, 900, False, seed)
    t = tile_table(1000, 900)
    for ti, kind in ((0, "left"), (2, "grad")):
        x, y, w, h = t[ti]
        r[y:y + h, x:x + w] = gray(kind, w, h, seed)
    x, y, w, h = t[3]
    r[y:y + h, x:x + w] = 77
    return r


# ------------------------------------------------------------------------------------------------ level-2 block forms
def l2_form(kind, w=420, h=300, seed=1):
    """RGB rasters for the forms of the 17 level-2 blocks.
    outliers : one colour with single one-pixel outliers of every magnitude class 1..8 (the same step on the three channels): every
               class stream holds a handful of equal symbols - one-symbol (type 1) blocks - or so few that raw (type 2) wins.
    noise1   : 1-bit noise, skewed: class 1 carries nearly every pixel, all 7 of its symbols in use.
    noise2   : 2-bit noise, skewed: class 2 with all 56 of its symbols in use.
    noise3   : 3-bit noise: class 3 with all 8 symbols (a dense, type 3, table), classes 1 and 2 beside it."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    out = np.empty((h, w, 3), dtype=np.uint8)
    if kind == "outliers":
        out[...] = (90, 120, 150)
        steps = [-1, 1, 2, 4, 8, 16, 32, 64]      # zig-zag 1, 2, 4, 8, ..., 128: classes 1..8
        for i, s in enumerate(steps):
            for rep in range(2):
                out[21 + 16 * i, 33 + 40 * rep + 8 * i] = (90 + s, 120 + s, 150 + s)
        return out
    bits = {"noise1": 1, "noise2": 2, "noise3": 3}[kind]
    for c in range(3):
        hh = _h(xs, ys, c, seed)
        n = (hh >> 8) & ((1 << bits) - 1)
        n = np.where(hh % 5 < 3, 0, n)            # skew: three pixels in five stay on the level
        out[..., c] = (100 + 20 * c + n).astype(np.uint8)
    return out


def alpha_form(kind, w=128, h=96, seed=1):
    """RGBA rasters for the forms of the level-1 alpha block: const (one symbol, type 1), raw (noise: type 2), dense (half the
    steps zero, the others cycling through every value: more than 238 of 256 table entries in use, type 3)."""
    r = steered(0, w, h, False, seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    if kind == "const":
        a = np.full((h, w), 200, dtype=np.int64)
    elif kind == "raw":
        a = 1 + _h(xs, ys, 3, seed) % 255
    elif kind == "dense":
        i = (ys * np.uint64(w) + xs).astype(np.int64)
        step = np.where(i & 1 == 1, (i >> 1) % 256, 0)
        a = np.cumsum(step.reshape(-1)).reshape(h, w) & 255
    else:
        raise ValueError(kind)
    out = np.concatenate([r, a.astype(np.uint8)[..., None]], axis=2)
    out[out[..., 3] == 0] = 0
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------ the named set
SIZES = [(900, 460), (64, 64), (30000, 4), (7, 9000)]          # two ordinary tiles / one small / one 30000 wide / one 9000 tall
BAND_SIZES = [(453, 130), (1003, 777), (2500, 70)]              # band reconstruction geometries; a tile wider than its seam buffer
GRAY_SIZES = [(420, 300), (7, 9000)]


def _fmt(alpha):
    return "rgba" if alpha else "rgb"


def named():
    """name -> (thunk, meta): every raster pinned in tests/golden/steered.json.  meta: what the encoder must do with it."""
    out = {}
    for pr in range(4):
        for alpha in (False, True):
            for (w, h) in SIZES + (BAND_SIZES if pr >= 2 else []):
                out[f"pr{pr}_{_fmt(alpha)}_{w}x{h}"] = (lambda pr=pr, w=w, h=h, alpha=alpha: steered(pr, w, h, alpha), {"pr": pr})
    for kind, want in TIES.items():
        for alpha in (False, True):
            out[f"tie_{kind}_{_fmt(alpha)}_900x460"] = (lambda kind=kind, alpha=alpha: tie(kind, 900, 460, alpha), {"pr": want, "tie": kind})
    for kind, mode in GRAY.items():
        for (w, h) in GRAY_SIZES + ([(100, 100)] if kind == "one" else []):
            out[f"gray_{kind}_{w}x{h}"] = (lambda kind=kind, w=w, h=h: gray(kind, w, h), {"gray": mode, "kind": kind})
    out["mixed_gray_1000x900"] = (mixed_gray, {})
    for kind in ("outliers", "noise1", "noise2", "noise3"):
        out[f"l2_{kind}_420x300"] = (lambda kind=kind: l2_form(kind), {"coded": True})
    for kind in ("const", "raw", "dense"):
        out[f"alpha_{kind}_128x96"] = (lambda kind=kind: alpha_form(kind), {"coded": True})
    return out


_cache = {}


def raster(name):
    """The named raster (read-only, shared between tests)."""
    if name not in _cache:
        r = np.ascontiguousarray(named()[name][0]())
        r.setflags(write=False)
        _cache[name] = r
    return _cache[name]
