"""Frequency-table tools for the rANS decode tests (test infrastructure, imported by test modules; not a conftest).

- parse_v2_block / gray_table: the frequency tables of v2 blocks (level 1) and of level-2 gray tiles, read as the reference
  decoder reads them (libxpng.c:429-493; MSB-first bit fields out of little-endian 32-bit words).
- lookup_profile / gray_profile: which symbol-lookup route of the wide decode chains (xpng_amd/csrc/rans2_wide_dec.hpp,
  rans1_wide_dec.hpp; table layouts and wd_store_tables in rans_dec.hpp) a stream with a given table can take, by the rules of
  their prep kernels.
- recode_tiles: rewrite chosen v2 blocks of mode-1 tile blobs (crafted, decode-only files).
- alpha_plane / symbol helpers: RGBA rasters whose alpha stream has a chosen symbol histogram.
"""
from __future__ import annotations

import numpy as np

COARSE_BITS_ALPHA = 9   # WdLayoutA::CBITS: 512 coarse bytes indexed by cold rank >> rsh
COARSE_BITS_GRAY = 9    # W1dLayoutA::CBITS: slot >> (pb - 9), 64-slot buckets at pb 15
SMALL_MAX_PB, SMALL_MAX_N = 12, 9   # WdLayout<false>: the register-searched context layout


class BitReader:
    """bitr of the oracle: 32 bits at a time, little-endian words, fields read from the top."""

    def __init__(self, data: bytes, pos: int = 0, end: int = None):
        self.d, self.p, self.end = data, pos, len(data) if end is None else end
        self.acc, self.have = 0, 0

    def get(self, c: int) -> int:
        if self.have < 32:
            self.acc = (self.acc << 32) & ((1 << 96) - 1)
            self.have += 32
            if self.p < self.end:
                self.acc += int.from_bytes(self.d[self.p:self.p + 4], "little")
                self.p += 4
        self.have -= c
        return (self.acc >> self.have) & ((1 << c) - 1)


def _read_table(rd: BitReader, btype: int, N: int, pb: int) -> np.ndarray:
    F = np.zeros(N, dtype=np.int64)
    for i in range(N):
        F[i] = rd.get(pb) if btype == 3 else (rd.get(pb) if rd.get(1) else 0)
    return F


def parse_v2_block(blk: bytes):
    """-> (type, n, pb, F): type 0 (empty), 1 (one symbol), 2 (raw) carry pb = F = None; types 3 / 4 the table as read."""
    h0 = int.from_bytes(blk[0:4], "little")
    btype = h0 >> 24
    if btype == 0:
        return 0, 0, None, None
    h1 = int.from_bytes(blk[4:8], "little")
    n, v2 = h1 & 0xFFFFFF, h1 >> 24
    if btype in (1, 2):
        return btype, n, None, None
    h2 = int.from_bytes(blk[8:12], "little")
    pb = h2 >> 24
    rd = BitReader(blk, 8 + 4 * (h2 & 0xFFFFFF), h0 & 0xFFFFFF)
    return btype, n, pb, _read_table(rd, btype, v2 + 2, pb)


def _owner(cum: np.ndarray, F: np.ndarray, slots: np.ndarray) -> np.ndarray:
    """Largest index with cum <= slot, stepped back over zero-frequency entries (the prep's binary search)."""
    o = np.searchsorted(cum[:len(F)], slots, side="right") - 1
    for _ in range(len(F)):  # (only reachable on tables that leave slots unowned)
        back = (o > 0) & (F[np.maximum(o, 0)] == 0)
        if not back.any():
            break
        o = np.where(back, o - 1, o)
    return o


def lookup_profile(pb: int, F, alpha: bool = True) -> dict:
    """How the wide v2 decode resolves slots of a stream with table F (k_rans2_dec_prep / k_rans2_dec_chain<true>).

    hot0 / hot1: the two symbols of largest (F << 8 | sym) (ties go to the higher index; hot1 = hot0 when one symbol is used);
    cold: 2^pb minus their ranges; rsh: coarse bytes are indexed by cold rank >> rsh (2^9 of them); max_bound: the most symbol
    boundaries past the coarse symbol inside one bucket (hot ranges and zero-frequency entries count: count8 steps over them).
    route: "exact" (rsh == 0: the coarse byte is the symbol), "round1" (<= 7 boundaries), "round2" (8..15), "scan" (>= 16).
    single: one used symbol (hot1 == hot0).  layout: "alpha" for the alpha stream; for a context stream "small" (register
    search, pb <= 12 and N <= 9) or "rest" (left to k_rans2_decode_rest)."""
    F = np.asarray(F, dtype=np.int64)
    N = len(F)
    keys = (F << 8) | np.arange(N)
    hot0 = int(keys.max())
    rest = np.where(keys == hot0, 0, keys)
    hot1 = int(rest.max())
    if (hot1 >> 8) == 0:
        hot1 = hot0
    s0, s1 = hot0 & 255, hot1 & 255
    cum = np.concatenate([[0], np.cumsum(F)])
    Ca, Fa = int(cum[s0]), int(F[s0])
    Cb, Fb = (int(cum[s1]), int(F[s1])) if s1 != s0 else (0, 0)
    if Fb and Cb < Ca:
        Ca, Fa, Cb, Fb = Cb, Fb, Ca, Fa
    cold = (1 << pb) - Fa - Fb
    rsh = 0
    while (cold >> rsh) > (1 << COARSE_BITS_ALPHA):
        rsh += 1
    max_bound, straddles = 0, 0
    if cold > 0:
        ranks = np.arange(cold, dtype=np.int64)
        slots = ranks + np.where(ranks >= Ca, Fa, 0)
        if Fb:
            slots = slots + np.where(slots >= Cb, Fb, 0)
        slots = np.minimum(slots, (1 << pb) - 1)
        own = _owner(cum, F, slots)
        starts = np.arange(0, cold, 1 << rsh)
        first, last = own[starts], own[np.minimum(starts + (1 << rsh), cold) - 1]
        max_bound = int((last - first).max())
        sfirst, slast = slots[starts], slots[np.minimum(starts + (1 << rsh), cold) - 1]
        for C, Fh in ((Ca, Fa), (Cb, Fb)):
            if Fh:
                straddles += int(((sfirst < C) & (slast >= C + Fh)).sum())
    if rsh == 0:
        route = "exact"
    else:
        route = "round1" if max_bound < 8 else ("round2" if max_bound < 16 else "scan")
    layout = "alpha" if alpha else ("small" if pb <= SMALL_MAX_PB and N <= SMALL_MAX_N else "rest")
    return dict(pb=pb, N=N, hot0=s0, hot1=s1, F0=int(F[s0]), F1=int(F[s1]), cold=cold, rsh=rsh, max_bound=max_bound,
                route=route, straddles=straddles, single=s0 == s1, layout=layout, used=int((F > 0).sum()))


def gray_profile(F, pb: int = 15) -> dict:
    """Level-2 gray slot (k_rans1_dec_chain<true>): the coarse byte names the owner of the bucket's first slot, then a forward
    scan; max_bound = the longest scan (boundaries inside one 2^(pb - 9)-slot bucket)."""
    F = np.asarray(F, dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(F)])
    total = int(cum[-1])
    sh = pb - COARSE_BITS_GRAY if pb > COARSE_BITS_GRAY else 0
    starts = np.arange(0, total, 1 << sh)
    own_first = _owner(cum, F, starts)
    own_last = _owner(cum, F, np.minimum(starts + (1 << sh), total) - 1)
    return dict(pb=pb, bucket=1 << sh, max_bound=int((own_last - own_first).max()), used=int((F > 0).sum()))


def tile_blobs(blobs: bytes, n_tiles: int):
    """Split concatenated tile blobs by their 24-bit size words."""
    out, o = [], 0
    for _ in range(n_tiles):
        L = int.from_bytes(blobs[o:o + 3], "little")
        out.append(blobs[o:o + L])
        o += L
    assert o == len(blobs)
    return out


def m1_blocks(tile: bytes, ch: int):
    """Mode-1 coded tile -> (prefix bytes up to the first v2 block, [the 9 (+1 alpha) v2 blocks])."""
    ksz = int.from_bytes(tile[4:8], "little")
    q, blocks = 4 + ksz, []
    for _ in range(9 + (ch == 4)):
        b0 = int.from_bytes(tile[q:q + 4], "little")
        sz = 4 if (b0 >> 24) == 0 else b0 & 0xFFFFFF
        blocks.append(bytes(tile[q:q + sz]))
        q += sz
    assert q == len(tile)
    return bytes(tile[:4 + ksz]), blocks


def recode_tiles(blobs: bytes, W: int, H: int, ch: int, fn) -> bytes:
    """Rewrite v2 blocks of mode-1 tile blobs: fn(tile index, stream c (0..8 context, 9 alpha), block bytes) returns a
    replacement block or None (kept).  Raw tiles pass unchanged; each tile's size word follows its new length."""
    from oracle import pyoracle as po
    out = bytearray()
    for ti, tile in enumerate(tile_blobs(blobs, len(po.tile_table(W, H, ch)))):
        if tile[3] == 0:
            out += tile
            continue
        head, blocks = m1_blocks(tile, ch)
        for c, blk in enumerate(blocks):
            new = fn(ti, c, blk)
            if new is not None:
                blocks[c] = new
        body = head + b"".join(blocks)
        out += len(body).to_bytes(3, "little") + bytes([tile[3]]) + body[4:]
    return bytes(out)


def gray_table(tile: bytes):
    """Level-2 tile -> (block type, F[256]) of its gray rANS v1 stream (pb 15), or None for any other tile kind.  The table
    follows the first pixel's 8 bits in the tile bit stream; the block type sits in the block behind that stream."""
    ttype = tile[3]
    if ttype >> 4 != 2 or ttype & 8:
        return None
    bsz = int.from_bytes(tile[4:8], "little")
    btype = tile[4 + bsz + 3]
    if btype not in (3, 4):
        return None
    rd = BitReader(tile, 8, 4 + bsz)
    rd.get(8)
    return btype, _read_table(rd, btype, 256, 15)


def sym_of_delta(d: int) -> int:
    """Alpha symbol of an alpha difference (pix_toU: wrap to int8, zig-zag)."""
    v = ((d + 128) & 255) - 128
    return (2 * v if v >= 0 else -2 * v - 1) & 255


def delta_of_sym(s: int) -> int:
    return (s >> 1) if s % 2 == 0 else (256 - ((s + 1) >> 1)) & 255


def symbols_from_counts(counts: dict, rng) -> np.ndarray:
    """A shuffled symbol sequence with exactly counts[sym] copies of each symbol."""
    seq = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in sorted(counts.items()) if c])
    rng.shuffle(seq)
    return seq


def alpha_plane(syms: np.ndarray, w: int, h: int, a0: int = 200) -> np.ndarray:
    """(h, w) alpha plane whose mode-1 alpha stream (pixels 1 .. w*h - 1 in raster order; left neighbour as predictor, the
    pixel above in column 0) is exactly syms."""
    assert len(syms) == w * h - 1
    lut = np.array([delta_of_sym(s) for s in range(256)], dtype=np.int64)
    d = np.concatenate([[a0], lut[syms]]).reshape(h, w)
    col = np.cumsum(d[:, 0])
    plane = col[:, None] + np.concatenate([np.zeros((h, 1), np.int64), np.cumsum(d[:, 1:], axis=1)], axis=1)
    return (plane & 255).astype(np.uint8)


# ---------------------------------------------------------------- table catalogue and crafted files

def _spread(counts: np.ndarray, total: int, floor: np.ndarray) -> np.ndarray:
    """Integer table proportional to counts, at least floor[i] per entry, summing to total (largest entry takes the rest)."""
    counts = np.asarray(counts, dtype=np.float64)
    F = np.maximum(np.floor(counts * (total - floor.sum()) / max(counts.sum(), 1.0)).astype(np.int64), 0) + floor
    F[int(np.argmax(F))] += total - int(F.sum())
    return F


def ctx_table(shape: str, hist: np.ndarray, pb: int) -> np.ndarray:
    """Context-stream tables (symbols 0..8) the reference encoder never writes:
    sym8: N = 9, every entry >= 1 (symbol 8 in the table even if unused);  holes: N = last used + 1, unused entries 0;
    skew: the most frequent used symbol at 2^pb - (N - 1), every other entry 1;  wide: N > 9, trailing zero entries."""
    hist = np.asarray(hist, dtype=np.int64)
    used = hist > 0
    top = int(np.nonzero(used)[0].max())
    if shape == "sym8":
        return _spread(hist[:9] if len(hist) >= 9 else np.pad(hist, (0, 9 - len(hist))), 1 << pb, np.ones(9, np.int64))
    if shape == "holes":
        return _spread(hist[:top + 1], 1 << pb, used[:top + 1].astype(np.int64))
    if shape == "skew":
        F = np.ones(max(top + 1, 2), np.int64)
        F[int(np.argmax(hist))] = (1 << pb) - (len(F) - 1)
        return F
    if shape == "wide":
        F = np.zeros(9 + 7 + 3 * (pb - 9), np.int64)
        F[:top + 1] = _spread(hist[:top + 1], 1 << pb, used[:top + 1].astype(np.int64))
        return F
    raise ValueError(shape)


def alpha_table(shape: str, hist: np.ndarray, pb: int) -> np.ndarray:
    """Alpha-stream tables at pb < 15: dense: every cold symbol at F = 1 but three that fill 57 % of the slots, unused entries 0
    (zero-frequency holes count as boundaries: a bucket of a few ranks holds many), the hot pair shares the rest;  flat: every used symbol about the same share;
    lone: one used symbol at 2^pb - 1 (a pb-bit field cannot hold 2^pb), the table sums to 2^pb - 1."""
    hist = np.asarray(hist, dtype=np.int64)
    used = hist > 0
    N = int(np.nonzero(used)[0].max()) + 1
    if shape == "lone":
        assert used.sum() == 1
        F = np.zeros(max(N, 2), np.int64)
        F[int(np.argmax(hist))] = (1 << pb) - 1
        return F
    if shape == "dense":
        F = used[:N].astype(np.int64)
        h = np.argsort(-hist[:N], kind="stable")[:5]
        extra = (57 << pb) // 100 - int(F.sum()) + 2          # cold ranks: 57 % of the slots (rsh > 0), three bulk symbols
        for q in range(3):
            F[h[2 + q]] += extra // 3 + (extra % 3 if q == 0 else 0)
        spare = (1 << pb) - int(F.sum())                      # the hot pair: about 21.5 % each
        F[h[0]] += spare - spare // 2
        F[h[1]] += spare // 2
        return F
    if shape == "flat":
        return _spread(used[:N].astype(np.float64), 1 << pb, used[:N].astype(np.int64))
    raise ValueError(shape)


CTX_SHAPES = ("sym8", "holes", "skew", "wide")


def craft_m1_variants(W: int = 600, H: int = 300):
    """Decode-only mode-1 RGBA files: (name, raster, tile blobs, [lookup_profile of every re-coded block]).

    Photo rasters whose alpha differences are 0, 1 or one of 2, 5, 8, .. 119 (alpha symbols with gaps between them); in each variant every context block is re-coded with a table shape of CTX_SHAPES
    at pb 10..12 (shape and pb rotate over the nine streams and the variants) and the alpha block at pb 10..14 with a dense
    or a flat table, all in dense (type 3) or sparse (type 4) form.  Two more rasters carry one alpha symbol (type 1 as the
    reference writes it): re-coded as a type 3 / 4 block whose table holds that symbol alone, first and last in the table."""
    from oracle import pyoracle as po
    from xpng_amd.synth import synth_raster
    rng = np.random.default_rng(5)
    base = synth_raster("photo", W, H, True, seed=7).copy()
    d = np.where(rng.random((H, W)) < 0.5, 0, np.where(rng.random((H, W)) < 0.5, 1, rng.choice(np.arange(2, 120, 3), (H, W))))
    base[..., 3] = ((np.cumsum(d, axis=1) + 1) & 255).astype(np.uint8)
    base[base[..., 3] == 0] = 0
    lone0 = synth_raster("photo", W, H, True, seed=8).copy()
    lone0[..., 3] = 200                                         # alpha differences all 0: symbol 0 alone
    lone2 = synth_raster("photo", W, H, True, seed=9).copy()
    yy, xx = np.mgrid[0:H, 0:W]
    lone2[..., 3] = ((xx + yy + 1) & 255).astype(np.uint8)      # all +1: symbol 2 alone (the last entry of its table)
    lone2[lone2[..., 3] == 0] = 0
    out = []
    k = 0
    for pb_a in (10, 11, 12, 13, 14):
        for ashape in ("dense", "flat"):
            for sparse in (False, True):
                prof = []

                def fn(ti, c, blk, k=k, pb_a=pb_a, ashape=ashape, sparse=sparse, prof=prof):
                    if blk[3] == 0:
                        return None
                    n = int.from_bytes(blk[4:7], "little")
                    syms, _ = po.rans2_decode(blk, n)
                    hist = np.bincount(syms, minlength=256)
                    if (hist > 0).sum() < 2:
                        return None
                    if c < 9:
                        pb = 10 + (c + k) % 3
                        F = ctx_table(CTX_SHAPES[(c + k) % 4], hist[:9], pb)
                    else:
                        pb, F = pb_a, alpha_table(ashape, hist, pb_a)
                    prof.append(lookup_profile(pb, F, alpha=c == 9))
                    return po.rans2_encode_table(F, syms, pb, sparse)

                blobs = recode_tiles(po.encode_tiles(1, base), W, H, 4, fn)
                out.append((f"ctx{k}-alpha-{ashape}-pb{pb_a}-{'sparse' if sparse else 'dense'}", base, blobs, prof))
                k += 1
    for name, r in (("lone-first", lone0), ("lone-last", lone2)):
        for sparse in (False, True):
            prof = []

            def fn(ti, c, blk, sparse=sparse, prof=prof):
                if c != 9:
                    return None
                assert blk[3] == 1
                n = int.from_bytes(blk[4:7], "little")
                syms, _ = po.rans2_decode(blk, n)
                F = alpha_table("lone", np.bincount(syms, minlength=256), 15)
                prof.append(lookup_profile(15, F))
                return po.rans2_encode_table(F, syms, 15, sparse)

            out.append((f"alpha-{name}-{'sparse' if sparse else 'dense'}", r, recode_tiles(po.encode_tiles(1, r), W, H, 4, fn), prof))
    return out


def scan_recipe_raster(W: int = 888, H: int = 444, seed: int = 5) -> np.ndarray:
    """Smooth alpha with sparse sharp edges: alpha differences 0 (40 %), 1 (25 %), else 2..11, and every value 0..255 at six
    random pixels.  The reference's own table for it puts 32 boundaries in one 32-rank bucket (rsh = 5): the plain scan."""
    from xpng_amd.synth import synth_raster
    rng = np.random.default_rng(seed)
    r = synth_raster("photo", W, H, True, seed=5).copy()
    u = rng.random((H, W))
    d = np.where(u < 0.40, 0, np.where(u < 0.65, 1, rng.integers(2, 12, (H, W))))
    d.flat[rng.choice(W * H, 256 * 6, replace=False)] = np.repeat(np.arange(256), 6)
    r[..., 3] = ((np.cumsum(d, axis=1) + 1) & 255).astype(np.uint8)
    r[r[..., 3] == 0] = 0
    return r


# single-tile RGBA rasters of 331 x 99 px: the alpha stream has 2^15 symbols, so the reference's pb-15 table IS the histogram
SHAPE_W, SHAPE_H = 331, 99


def _counts(hot: dict, fill: int = None, ones: bool = True) -> dict:
    c = {s: 1 for s in range(256)} if ones else {}
    c.update(hot)
    rest = (1 << 15) - sum(c.values())
    if rest:
        assert fill is not None and rest > 0
        c[fill] = c.get(fill, 0) + rest
    return c


ALPHA_SHAPES = {
    # name: (symbol counts, route the wide chain must take, extra check)
    "exact": _counts({0: 20000, 2: 12256}, fill=4),            # cold = 512 exactly: rsh 0, 254 symbols at F = 1
    "round1": _counts({0: 16000, 2: 13000}, fill=4),           # cold 3768: rsh 3, <= 7 boundaries per bucket
    "round2": _counts({0: 16000, 2: 10000, 6: 3000}, fill=4),  # cold 6768: rsh 4, 15 boundaries in a bucket
    "scan": _counts({0: 12000, 2: 8000}, fill=4),              # symbol 4 takes the rest (hot0): cold 8253, rsh 5, 31+ boundaries
    "two": _counts({0: 20000, 2: 12768}, ones=False),          # two symbols (and a hole between): cold = 0
    "tied": _counts({0: 14884, 2: 14884}, fill=4),             # equal hot pair: hot0 is the higher index
    "hot_inside": _counts({100: 16000, 102: 14000}, fill=0),   # hot symbols with cold neighbours on both sides
}
ALPHA_ROUTES = {"exact": "exact", "round1": "round1", "round2": "round2", "scan": "scan", "two": "exact", "tied": "round1",
                "hot_inside": "round2"}


def shape_raster(name: str, seed: int = 0) -> np.ndarray:
    from xpng_amd.synth import synth_raster
    rng = np.random.default_rng(1000 + seed)
    r = synth_raster("photo", SHAPE_W, SHAPE_H, True, seed=3 + seed).copy()
    r[..., 3] = alpha_plane(symbols_from_counts(ALPHA_SHAPES[name], rng), SHAPE_W, SHAPE_H)
    r[r[..., 3] == 0] = 0
    return r


def alpha_block_tables(blobs: bytes, W: int, H: int):
    """The (pb, F) of every coded tile's alpha block that has a table (types 3 / 4)."""
    from oracle import pyoracle as po
    out = []
    for tile in tile_blobs(blobs, len(po.tile_table(W, H, 4))):
        if tile[3] == 0:
            continue
        t, n, pb, F = parse_v2_block(m1_blocks(tile, 4)[1][9])
        if t >= 3:
            out.append((pb, F))
    return out


def file_header(W: int, H: int, level: int, alpha: bool) -> bytes:
    return (((W - 1) | (level << 24)).to_bytes(4, "little") + ((H - 1) | (int(alpha) << 24)).to_bytes(4, "little"))


def gray_scan_raster(W: int = 600, H: int = 300, seed: int = 3) -> np.ndarray:
    """Level-2 gray tile (R = G = B) of a smooth ramp with a few hundred isolated spikes: the residuals of the spikes spread over
    most of the 256 symbols at F of 1 or 2, so a 64-slot coarse bucket of the gray slot holds dozens of boundaries."""
    from xpng_amd.synth import synth_raster
    rng = np.random.default_rng(seed)
    g = synth_raster("gray", W, H, False, seed=seed)[..., 0].copy()
    g.flat[rng.choice(W * H, 600, replace=False)] = rng.integers(0, 256, 600)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))
