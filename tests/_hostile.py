"""Hostile tile headers and the verdict each one must get - TEST INFRASTRUCTURE, shared by tests/test_dec_parse_host.py (the four
validators of the decode run on the host) and tests/test_hostile_tiles.py (the rejections on the device).

A case is a tile blob, the tile's n / pxsz, the bytes that exist behind the tile's offset (`avail`), a name `<tile>/<field>=<value>`
and the verdict `accept` or `reject`.  The blobs are tiles of oracle.pyoracle.encode_tiles on tiny one-tile rasters, and tiles put
together here from hand-made blocks where a condition needs a block the encoder does not write for so few pixels; the edits are
systematic: every header field of the tile and of each of its blocks set to 0, 1, its legal minimum - 1, its minimum, its value - 1,
its value, its value + 1, its legal maximum, that + 1, and all ones.  compound() adds what one edit cannot reach.

THE RULES (judge_m1, judge_m2) are written from the format as DESIGN.md 3-5 and oracle/xpng_oracle.c (decode_tile_m1, decode_tile_m2,
xo_rans2_decode, rans1_decode) state it, not from the kernels.  A tile is acceptable when a decoder that follows the format reads every
header word, the k / b words, every block, its word range, its two states and its table inside [0, L) with L <= avail, and writes no
stream beyond its quota.  Each rule has a name (the `rule` of a rejected case); where the format leaves a question open the decision
and its reason stand beside the rule:

  m1 tile type    raw (0) or high nibble 1.  The encoder writes 0x10 | predictor (0..3); the reference decoder reads bits 0 and 1 and
                  ignores bits 2 and 3, so 0x14..0x1F are accepted like it does.  Any other high nibble is no tile of this format.
  block sizes % 4 MODE 1 REQUIRES a multiple of 4, MODE 2 DOES NOT, and both are right.  A v2 block (mode 1) is read in whole dwords up
                  to its end: the table reader (BitR in rans2_dec_freqs) and the second word of a raw symbol (rans2_dec_plain) test
                  `p < end` and then load 4 bytes, so an end that is no multiple of 4 lets them read up to 3 bytes behind the block,
                  and behind L for the last block.  A v1 block (mode 2) holds only words: its consumers take nw = (size - 24) >> 2 of
                  them, rounding DOWN, and its table lies in b, whose own size must be a multiple of 4 for the same dword reads.
  pb 10..15       the encoder writes 12 and 15.  The consumers' tables need pb <= 15 (2^15 slots, 16-bit cumulative counts) and
                  pb >= 8 (the coarse tables drop pb - 8 bits); the oracle's own table writer takes 10..15 and so do the rules: no
                  file of the reference has another value.
  v2 (raw bits)   1..8: a symbol is a byte, and 0 bits make the extraction shift by 64.
  gray stream     at most n symbols (the encoder writes n - 1): the stream region holds n, the consumer reads n - 1 of them.
  class streams   at most 3 n symbols (classes 1 and 2: n), and every stream in the room its length needs inside
                  m2_streams_region(n): the caps of the decode workspace (m2_encode.hpp), beyond anything the format produces.
  fewer symbols   context streams that hold fewer than n - 1 symbols are accepted: the reference would read stale memory of its own
                  pool, the device reads stale bytes of its own plane, neither leaves its buffers.
  m2 table bits   may run past the end of b: they read as 0 there (BITSTREAM_FILL past the end), the table entries behind it are 0.
"""
import struct

import numpy as np

ACCEPT, REJECT = 1, 0


def rup(a, b):
    return (a + b - 1) // b * b


def m2_slot(m):
    return rup(m + 32, 64)


def m2_streams_region(n):
    return rup(4 * n + 21 * 96, 256)


def m2_nominal(s):
    if s < 9:
        return 9
    if s >= 17:
        return 256
    v = s - 8
    return 1 << (3 * v) if v < 3 else 1 << v


def u32(b, o):
    return int.from_bytes(b[o:o + 4], "little")


class Reject(Exception):
    pass


def need(cond, rule):
    if not cond:
        raise Reject(rule)


# ---- the rules -----------------------------------------------------------------------------------------------------------
def _judge_m1(b, avail, n, pxsz):
    b = b[:avail]
    need(avail >= 4, "no tile word")
    ty, L = b[3], u32(b, 0) & 0xFFFFFF
    need(L <= avail, "L > avail")
    if ty == 0:
        need(L == n * pxsz + 4, "raw L")                            # the raw rows are n * pxsz bytes behind the word
        return
    need(ty >> 4 == 1, "tile type")
    need(L >= 8, "no ksz word")
    ksz = u32(b, 4)
    need(ksz >= 8, "ksz < 8")                                       # the first pixel is read from k's first word
    need(ksz % 4 == 0, "ksz % 4")                                   # k is words
    need(4 + ksz <= L, "k > L")
    o, coded = 4 + ksz, 0
    for c in range(9 + (pxsz == 4)):
        need(o + 4 <= L, "no block word")
        bt, sz = b[o + 3], u32(b, o) & 0xFFFFFF
        need(bt <= 4, "block type")
        if bt == 0:
            o += 4                                                  # an empty block is its word (xo_rans2_decode returns 4)
            continue
        need(sz >= 8, "block size < 8")
        need(sz % 4 == 0, "block size % 4")
        need(o + sz <= L, "block > L")
        m, v2 = u32(b, o + 4) & 0xFFFFFF, b[o + 7]
        if bt == 2:
            need(1 <= v2 <= 8, "raw bits")
            need(8 + 4 * ((m * v2 + 31) // 32) <= sz, "raw symbols > block")
        if bt >= 3:
            need(v2 <= 254, "alphabet > 256")                       # N = v2 + 2 symbols of a byte
            need(sz >= 12, "no table word")
            toff, pb = u32(b, o + 8) & 0xFFFFFF, b[o + 11]
            need(10 <= pb <= 15, "pb")
            need(toff >= 5, "states < words")                       # the two states lie at table - 16 >= the first word at 12
            need(8 + 4 * toff < sz, "table >= block end")
        if c < 9:
            coded += m
            need(coded <= n - 1, "context symbols > n - 1")
        else:
            need(m <= n - 1, "alpha symbols > n - 1")
        o += sz


def _judge_m2(b, avail, n):
    b = b[:avail]
    need(avail >= 4, "no tile word")
    ty, L = b[3], u32(b, 0) & 0xFFFFFF
    need(L <= avail, "L > avail")
    if ty == 0:
        need(L == 3 * n + 4, "raw L")
        return
    if ty == 255:
        need(L == 8, "single colour L")                             # the encoder writes (255 << 24) | 8 and one pixel
        return
    need(ty >> 4 in (1, 2), "tile type")
    gray = ty >> 4 == 2
    if gray and ty & 8:
        need(L == n + 4, "raw gray L")
        return
    need(L >= 8, "no bsz word")
    bsz = u32(b, 4)
    need(bsz >= 8, "bsz < 8")                                       # the first pixel is read from b's first word
    need(bsz % 4 == 0, "bsz % 4")
    need(4 + bsz <= L, "b > L")
    o, coded, room = 4 + bsz, 0, 0
    for s in ([17] if gray else range(17)):
        need(o + 4 <= L, "no block word")
        bt, sz = b[o + 3], u32(b, o) & 0xFFFFFF
        need(bt <= 4, "block type")
        need(sz >= (4 if bt == 0 else 8), "block size < 8")
        need(o + sz <= L, "block > L")
        if bt >= 3:
            need(sz >= 24, "no states")                             # the word, n and the two states
        m = 0 if bt == 0 else (u32(b, o + 4) & 0xFFFFFF if bt == 1 else u32(b, o + 4))
        need(m <= (3 * n if 11 <= s < 17 else n), "stream > cap")
        room += m2_slot(m)
        need(room <= m2_streams_region(n), "streams > region")
        if s < 9:
            coded += m
        o += sz
    need(coded <= n - 1, "context symbols > n - 1")


def judge(mode, b, avail, n, pxsz):
    """-> (ACCEPT | REJECT, the rule that rejects it or '')"""
    try:
        _judge_m1(b, avail, n, pxsz) if mode == 1 else _judge_m2(b, avail, n)
    except Reject as r:
        return REJECT, str(r)
    return ACCEPT, ""


# ---- fields of a tile the oracle (or craft below) wrote ------------------------------------------------------------------
def fields(mode, b, n, pxsz):
    """[(field, label, byte offset of its word, shift, bits, legal minimum, legal maximum)] of a well-formed tile"""
    ty, L = b[3], u32(b, 0) & 0xFFFFFF
    f = [("L", "L", 0, 0, 24, 5 if mode == 2 else 12, len(b))]
    if mode == 1:
        f.append(("type", "type", 0, 24, 8, 0x10, 0x1F))
        if ty == 0:
            return f
        ksz = u32(b, 4)
        f.append(("ksz", "ksz", 4, 0, 32, 8, L - 4))
        o = 4 + ksz
        for c in range(9 + (pxsz == 4)):
            bt, sz = b[o + 3], u32(b, o) & 0xFFFFFF
            who = "alpha" if c == 9 else "blk"
            f.append((who + ".type", "%s%d.type" % (who, c), o, 24, 8, 0, 4))
            f.append((who + ".size", "%s%d.size" % (who, c), o, 0, 24, 32 if bt >= 3 else 8, L - o))
            if bt:
                f.append((who + ".n", "%s%d.n" % (who, c), o + 4, 0, 24, 0, n - 1))
                f.append((who + ".v2", "%s%d.v2" % (who, c), o + 4, 24, 8, 1 if bt == 2 else 0, 255 if bt == 1 else 8 if bt == 2 else 254))
            if bt >= 3:
                f.append((who + ".toff", "%s%d.toff" % (who, c), o + 8, 0, 24, 5, (sz - 8) // 4 - 1))
                f.append((who + ".pb", "%s%d.pb" % (who, c), o + 8, 24, 8, 10, 15))
            o += sz if bt else 4
        return f
    f.append(("kind", "kind", 0, 24, 8, 0x10, 0x2B))
    if ty in (0, 255) or (ty >> 4 == 2 and ty & 8):
        return f
    bsz = u32(b, 4)
    f.append(("bsz", "bsz", 4, 0, 32, 8, L - 8))
    o = 4 + bsz
    for s in ([17] if ty >> 4 == 2 else range(17)):
        bt, sz = b[o + 3], u32(b, o) & 0xFFFFFF
        f.append(("blk.type", "blk%d.type" % s, o, 24, 8, 0, 4))
        f.append(("blk.size", "blk%d.size" % s, o, 0, 24, 24 if bt >= 3 else 8 if bt else 4, L - o))
        if bt == 1:
            f.append(("blk.nsym", "blk%d.nsym" % s, o + 4, 0, 24, 0, 3 * n if 11 <= s < 17 else n))
            f.append(("blk.sym", "blk%d.sym" % s, o + 4, 24, 8, 0, 255))
        elif bt:
            f.append(("blk.nsym", "blk%d.nsym" % s, o + 4, 0, 32, 0, 3 * n if 11 <= s < 17 else n))
        o += sz
    return f


def edit_values(exact, lo, hi, bits):
    top = (1 << bits) - 1
    return sorted({v for v in (0, 1, lo - 1, lo, exact - 1, exact, exact + 1, hi, hi + 1, top) if 0 <= v <= top})


def put(b, off, shift, bits, v):
    """b with the field at (off, shift, bits) set to v"""
    w = (u32(b, off) & ~(((1 << bits) - 1) << shift)) | (v << shift)
    return b[:off] + struct.pack("<I", w & 0xFFFFFFFF) + b[off + 4:]


class Case:
    __slots__ = ("name", "field", "mode", "pxsz", "n", "w", "avail", "blob", "verdict", "rule", "base", "patches")

    def __init__(self, name, field, mode, pxsz, n, w, blob, avail=None, base=None, patches=()):
        """blob: the bytes behind the tile's offset (avail of them; a shorter blob is followed by 0x5A bytes).  base / patches: the
        same bytes as (a blob many cases share, [(offset, bytes)]): how the case file stores them"""
        self.name, self.field, self.mode, self.pxsz, self.n, self.w = name, field, mode, pxsz, n, w
        self.avail = len(blob) if avail is None else avail
        self.blob = (blob + b"\x5A" * max(0, self.avail - len(blob)))[:self.avail]
        self.verdict, self.rule = judge(mode, self.blob, self.avail, n, pxsz)
        self.base, self.patches = self.blob if base is None else base, list(patches)


class Cases:
    def __init__(self):
        self.cases = []

    def systematic(self, tile, mode, pxsz, n, w, blob):
        """every field of `blob` at every edit value, in front of exactly len(blob) bytes"""
        for field, label, off, shift, bits, lo, hi in fields(mode, blob, n, pxsz):
            exact = (u32(blob, off) >> shift) & ((1 << bits) - 1)
            for v in edit_values(exact, lo, hi, bits):
                e = put(blob, off, shift, bits, v)
                self.cases.append(Case("%s/%s=%d" % (tile, label, v), "m%d.%s" % (mode, field), mode, pxsz, n, w, e,
                                       base=blob, patches=[(off, e[off:off + 4])]))

    def whole(self, name, field, mode, pxsz, n, w, blob, avail=None):
        c = Case(name, field, mode, pxsz, n, w, blob, avail)
        self.cases.append(c)
        return c

    def write(self, path, cases=None):
        """the flat binary file the host program reads: u32 bases, {u32 len, bytes}, u32 cases, {u32 base, mode, pxsz, n, w, avail,
        verdict, patches, {u32 offset, len, bytes}, u32 name length, name}"""
        cases = self.cases if cases is None else cases
        used, renum = [], {}
        for c in cases:
            if id(c.base) not in renum:
                renum[id(c.base)] = len(used)
                used.append(c.base)
        out = [struct.pack("<I", len(used))]
        for b in used:
            out += [struct.pack("<I", len(b)), b]
        out.append(struct.pack("<I", len(cases)))
        for c in cases:
            patches = [(o, p) for o, p in c.patches if o < c.avail]
            out.append(struct.pack("<8I", renum[id(c.base)], c.mode, c.pxsz, c.n, c.w, c.avail, c.verdict, len(patches)))
            for o, p in patches:
                p = p[:c.avail - o]
                out += [struct.pack("<2I", o, len(p)), p]
            nm = c.name.encode()
            out += [struct.pack("<I", len(nm)), nm]
        with open(path, "wb") as f:
            f.write(b"".join(out))
        return len(cases)


# ---- hand-made blocks and tiles ------------------------------------------------------------------------------------------
def w32(*v):
    return struct.pack("<%dI" % len(v), *[x & 0xFFFFFFFF for x in v])


def v2_blk0():
    return w32(4)


def v2_blk1(m, sym):
    return w32(8 | 1 << 24, m | sym << 24)


def v2_blk2(m, v2, size=None, ty=2):
    words = (m * v2 + 31) // 32
    size = 8 + 4 * words if size is None else size
    return w32(size | ty << 24, m | v2 << 24) + b"\x33" * max(0, size - 8)


def v2_blk34(ty, m, v2, pb, toff, size):
    """12 bytes of header, then `size - 12` bytes: the words, the states and the table wherever toff says"""
    return (w32(size | ty << 24, m | v2 << 24, toff | pb << 24) + b"\x11" * max(0, size - 12))[:max(size, 12)]


def tile_m1(ty, blocks, kwords=1, L=None):
    body = w32(4 + 4 * kwords) + b"\x77" * (4 * kwords) + b"".join(blocks)
    return w32((len(body) + 4 if L is None else L) | ty << 24) + body


def v1_blk(bt, size, m=None, sym=0):
    if bt == 0:
        return (w32(size) + b"\x22" * max(0, size - 4))[:max(size, 4)]
    h1 = (m | sym << 24) if bt == 1 else m
    return (w32(size | bt << 24, h1) + b"\x22" * max(0, size - 8))[:max(size, 8)]


def tile_m2(ty, blocks, bwords=1, L=None, bbytes=None):
    """bbytes: the bytes of b behind its size word where they are no whole words"""
    bbytes = 4 * bwords if bbytes is None else bbytes
    body = w32(4 + bbytes) + b"\x66" * bbytes + b"".join(blocks)
    return w32((len(body) + 4 if L is None else L) | ty << 24) + body


FORMATS = [(1, 3), (1, 4), (2, 3)]                                   # (mode, pxsz): mode 1 RGB, mode 1 RGBA, mode 2


def base_tiles(po, mode, pxsz):
    """[(name, n, w, blob)]: one-tile rasters through the oracle's encoder.  Block types 0, 1, 2, 3 and 4 all occur in every
    format (asserted in build())"""
    from xpng_amd.synth import synth_raster
    import _steered as S
    out = []
    shapes = [(4, 4), (64, 64), (97, 31)] + ([(16, 3), (5, 3)] if pxsz == 3 else [(16, 4)])  # (no RGBA tile is narrower than 4)
    for kind in ("photo", "flat", "gray", "noise"):
        for (w, h) in shapes:
            if kind == "noise" and w * h > 64:
                continue                                             # (raw tiles: the small ones say all there is to say)
            r = synth_raster(kind, w, h, pxsz == 4, seed=3)
            out.append(("%s%dx%d" % (kind, w, h), w * h, w, po.encode_tiles(mode, r)))
    r = np.zeros((12, 20, pxsz), np.uint8)                           # a ramp along the rows: streams of one distinct symbol (type 1)
    r[..., 0], r[..., 1] = np.arange(20)[None, :] * 3, 7
    if pxsz == 4:
        r[..., 3] = 200
    out.append(("ramp20x12", 240, 20, po.encode_tiles(mode, r)))
    if mode == 1:
        r = S.steered(2, 64, 64, pxsz == 4)                          # a steered predictor: another type byte
        out.append(("steered64x64", 64 * 64, 64, po.encode_tiles(1, r)))
    else:
        r = S.gray("left", 20, 12)
        out.append(("grayleft20x12", 240, 20, po.encode_tiles(2, r)))
    return out


def block_types(mode, blob, pxsz):
    ty = blob[3]
    if ty == 0 or (mode == 2 and (ty == 255 or (ty >> 4 == 2 and ty & 8))):
        return set()
    o, out = 4 + u32(blob, 4), set()
    for _ in (range(9 + (pxsz == 4)) if mode == 1 else [17] if ty >> 4 == 2 else range(17)):
        bt = blob[o + 3]
        out.add(bt)
        o += (u32(blob, o) & 0xFFFFFF) if (bt or mode == 2) else 4
    return out


def compound(cs, mode, pxsz, tiles):
    """what one edit cannot reach"""
    add = cs.whole
    fm = "m%d." % mode
    for name, n, w, blob in tiles:                                   # avail of 0, 3, 4, L - 1, L (and behind L)
        L = len(blob)
        for a in (0, 3, 4, L - 1, L, L + 5):
            add("%s/avail=%d" % (name, a), fm + "avail", mode, pxsz, n, w, blob, a)
        for v in (L - 4, L - 1, L + 1, L + 4, L + 8, L + 9):       # the L edits again, in front of 8 bytes that exist
            add("%s/L=%d in front of 8 more bytes" % (name, v), fm + "L", mode, pxsz, n, w, put(blob, 0, 0, 24, v), L + 8)
    n, w = 16, 4
    if mode == 1:
        spt = 9 + (pxsz == 4)
        rest = lambda k: [v2_blk0()] * (spt - k)
        # the last block ends exactly at L, and one byte past it
        t = tile_m1(0x10, [v2_blk1(15, 3)] + rest(1))
        add("last block ends at L", fm + "L", 1, pxsz, n, w, t)
        add("last block ends one byte past L", fm + "L", 1, pxsz, n, w, put(t, 0, 0, 24, len(t) - 1), len(t))
        last = [v2_blk0()] * (spt - 1) + [v2_blk1(15, 3)]
        t = tile_m1(0x10, last)
        add("last 8-byte block ends at L", fm + "L", 1, pxsz, n, w, t)
        add("last 8-byte block one byte past L", fm + "L", 1, pxsz, n, w, put(t, 0, 0, 24, len(t) - 1), len(t))
        # a tile that ends inside its last block's word, inside its ksz word, behind it: the buffer ends where the tile does
        t = tile_m1(0x10, [v2_blk0()] * spt)
        for d in (1, 2, 3, 4):
            add("tile and buffer end %d bytes inside the last block word" % d, fm + "L", 1, pxsz, n, w, put(t, 0, 0, 24, len(t) - d)[:len(t) - d])
        for L in (4, 5, 6, 7, 8, 11, 12):
            add("coded tile L=%d in %d bytes" % (L, L), fm + "L", 1, pxsz, n, w, put(t, 0, 0, 24, L)[:L])
        add("ksz=4: no k word", fm + "ksz", 1, pxsz, n, w, tile_m1(0x10, [v2_blk0()] * spt, kwords=0))
        add("ksz=4: no k word, symbols", fm + "ksz", 1, pxsz, n, w, tile_m1(0x10, [v2_blk1(15, 3)] + rest(1), kwords=0))
        # a type 3 / 4 block of 8 bytes at the very end of the buffer: its third word does not exist
        for bt in (3, 4):
            t = tile_m1(0x10, [v2_blk0()] * (spt - 1) + [w32(8 | bt << 24, 3 | 7 << 24)])
            add("last block type %d of 8 bytes" % bt, fm + "blk.size", 1, pxsz, n, w, t)
        # context counts that sum to n - 1 and to n, over one block and over nine
        for total in (n - 1, n):
            add("one context block of %d" % total, fm + "blk.n", 1, pxsz, n, w, tile_m1(0x10, [v2_blk1(total, 0)] + rest(1)))
            nine = [v2_blk1(1, 0)] * 8 + [v2_blk1(total - 8, 1)]
            add("nine context blocks of %d" % total, fm + "blk.n", 1, pxsz, n, w, tile_m1(0x11, nine + rest(9)))
        if pxsz == 4:                                                # an alpha n of n - 1 and of n
            for m in (n - 1, n):
                add("alpha of %d" % m, fm + "alpha.n", 1, 4, n, w, tile_m1(0x10, [v2_blk1(3, 0)] + [v2_blk0()] * 8 + [v2_blk1(m, 9)]))
                add("raw alpha of %d" % m, fm + "alpha.n", 1, 4, n, w, tile_m1(0x10, [v2_blk0()] * 9 + [v2_blk2(m, 8)]))
        # type 2: v2 of 0, 1, 8, 9, and a size one word short of 8 + 4 ceil(n v2 / 32)
        for v2 in (0, 1, 8, 9):
            for m in (15, 8, 1):
                full = 8 + 4 * ((m * max(v2, 1) + 31) // 32)
                for size in (full - 4, full, full + 4):
                    add("raw block v2=%d m=%d size=%d" % (v2, m, size), fm + "blk.v2", 1, pxsz, n, w,
                        tile_m1(0x10, [v2_blk2(m, v2, size)] + rest(1)))
        # type >= 3: sz of 28 and 32; toff of 4 and 5; 8 + 4 toff equal to sz - 4, sz, sz + 4
        for bt in (3, 4):
            for size, toff in ((28, 5), (32, 5), (32, 4), (32, 6), (36, 5), (36, 6), (36, 7), (36, 8), (64, 13), (64, 14), (64, 15), (24, 5), (12, 5), (16, 5)):
                add("block type %d size=%d toff=%d" % (bt, size, toff), fm + "blk.toff", 1, pxsz, n, w,
                    tile_m1(0x10, [v2_blk34(bt, 7, 7, 12, toff, size)] + rest(1)))
                add("last block type %d size=%d toff=%d" % (bt, size, toff), fm + "blk.toff", 1, pxsz, n, w,
                    tile_m1(0x10, [v2_blk0()] * (spt - 1) + [v2_blk34(bt, 7, 7, 12, toff, size)]))
            for pb in (9, 10, 15, 16):
                add("block type %d pb=%d" % (bt, pb), fm + "blk.pb", 1, pxsz, n, w, tile_m1(0x10, [v2_blk34(bt, 7, 7, pb, 6, 40)] + rest(1)))
            for v2 in (254, 255):
                add("block type %d v2=%d" % (bt, v2), fm + "blk.v2", 1, pxsz, n, w, tile_m1(0x10, [v2_blk34(bt, 7, v2, 12, 6, 40)] + rest(1)))
        # sizes that are no multiple of 4, in front of bytes that exist
        for size in (9, 10, 11, 12):
            add("one-symbol block size=%d" % size, fm + "blk.size", 1, pxsz, n, w,
                tile_m1(0x10, [w32(size | 1 << 24, 5) + b"\0" * (size - 8)] + rest(1)))
        for kw in (1, 2):
            for d in (0, 1, 2, 3):
                t = tile_m1(0x10, [v2_blk1(5, 0)] + rest(1), kwords=kw)
                add("ksz=%d over %d words" % (4 + 4 * kw + d, kw), fm + "ksz", 1, pxsz, n, w, put(t, 4, 0, 32, 4 + 4 * kw + d))
        for npx in (1, 2):                                           # one pixel: no coded symbol at all
            add("n=%d without symbols" % npx, fm + "blk.n", 1, pxsz, npx, npx, tile_m1(0x10, [v2_blk0()] * spt))
            add("n=%d with one symbol" % npx, fm + "blk.n", 1, pxsz, npx, npx, tile_m1(0x10, [v2_blk1(1, 0)] + rest(1)))
            add("n=%d raw" % npx, fm + "L", 1, pxsz, npx, npx, w32(npx * pxsz + 4) + b"\1" * (npx * pxsz))
        return
    # ---- mode 2
    empty17 = [v1_blk(0, 4)] * 17
    for ty in (0x00, 0xFF, 0x10, 0x13, 0x14, 0x1F, 0x20, 0x23, 0x24, 0x28, 0x29, 0x2A, 0x2B, 0x2C, 0x2F, 0x30, 0x0F, 0x01, 0x7F, 0xEE, 0xFE):
        for what, t in (("raw", w32(3 * n + 4) + b"\1" * (3 * n)), ("one", w32(8, 0x01020304)), ("rawgray", w32(n + 4) + b"\1" * n),
                        ("colour", tile_m2(0, empty17)), ("gray", tile_m2(0, [v1_blk(1, 8, n - 1, 2)]))):
            add("kind byte %#04x on a %s tile" % (ty, what), fm + "kind", 2, 3, n, w, put(t, 0, 24, 8, ty))
    for L in (4, 5, 7, 8):                                           # L of 4, 5, 7 and 8 on the short kinds
        for ty in (0xFF, 0x28, 0x00, 0x10, 0x20):
            for npx in (1, 3):
                add("kind %#04x L=%d n=%d" % (ty, L, npx), fm + "L", 2, 3, npx, npx, w32(L | ty << 24) + b"\7" * 4)
                add("kind %#04x L=%d n=%d in %d bytes" % (ty, L, npx, L), fm + "L", 2, 3, npx, npx, (w32(L | ty << 24) + b"\7" * 4)[:L])
    # bsz + 8 equal to L and to L + 4
    t = tile_m2(0x20, [v1_blk(0, 4)])
    add("bsz + 8 == L", fm + "bsz", 2, 3, n, w, t)
    add("bsz + 8 == L + 4", fm + "bsz", 2, 3, n, w, put(t, 4, 0, 32, u32(t, 4) + 4))
    add("bsz + 8 == L + 4 in front of more bytes", fm + "bsz", 2, 3, n, w, put(t, 4, 0, 32, u32(t, 4) + 4), len(t) + 8)
    for bsz in (0xFFFFFFFC, 0xFFFFFFF8, 0x80000000, 0x01000000):
        add("bsz=%#x" % bsz, fm + "bsz", 2, 3, n, w, put(t, 4, 0, 32, bsz))
        add("colour bsz=%#x" % bsz, fm + "bsz", 2, 3, n, w, put(tile_m2(0x10, empty17), 4, 0, 32, bsz))
    for d in (1, 2, 3):
        add("bsz %% 4 == %d" % d, fm + "bsz", 2, 3, n, w, put(tile_m2(0x20, [v1_blk(0, 4)], bwords=2), 4, 0, 32, 8 + d))
        add("gray b of %d bytes, a block behind it" % (4 + d), fm + "bsz", 2, 3, n, w, tile_m2(0x20, [v1_blk(1, 8, 5, 1)], bbytes=4 + d))
        add("colour b of %d bytes, blocks behind it" % (8 + d), fm + "bsz", 2, 3, n, w, tile_m2(0x10, empty17, bbytes=8 + d))
    for bb in (0, 4):                                                # bsz of 4: no word of b, and 8
        add("gray bsz=%d" % (4 + bb), fm + "bsz", 2, 3, n, w, tile_m2(0x20, [v1_blk(1, 8, 5, 1)], bbytes=bb))
        add("colour bsz=%d" % (4 + bb), fm + "bsz", 2, 3, n, w, tile_m2(0x10, empty17, bbytes=bb))
    # a class stream at 3 n and at 3 n + 1 symbols (classes 1 and 2: n), a context stream at n - 1 and n, the gray stream at n and n + 1
    for s, cap in ((9, n), (10, n), (11, 3 * n), (16, 3 * n)):
        for m in (cap, cap + 1):
            for bt in (1, 2):
                blocks = list(empty17)
                blocks[s] = v1_blk(bt, 8, m, 1)
                add("stream %d type %d of %d" % (s, bt, m), fm + "blk.nsym", 2, 3, n, w, tile_m2(0x10, blocks))
    for m in (n - 1, n):
        blocks = list(empty17)
        blocks[0] = v1_blk(1, 8, m, 0)
        add("one context stream of %d" % m, fm + "blk.nsym", 2, 3, n, w, tile_m2(0x11, blocks))
        blocks = [v1_blk(1, 8, 1, 0)] * 8 + [v1_blk(2, 8, m - 8)] + [v1_blk(0, 4)] * 8
        add("nine context streams of %d" % m, fm + "blk.nsym", 2, 3, n, w, tile_m2(0x11, blocks))
    for m in (n - 1, n, n + 1):
        for bt in (1, 2):
            add("gray stream type %d of %d" % (bt, m), fm + "blk.nsym", 2, 3, n, w, tile_m2(0x21, [v1_blk(bt, 8, m, 4)]))
    # streams whose slots sum to exactly m2_streams_region(n), and to one slot more: n = 256, region 3072 = 17 slots of 64 and 31 more
    n2 = 256
    assert m2_streams_region(n2) == 3072
    blocks = list(empty17)
    blocks[11], blocks[12], blocks[13] = v1_blk(1, 8, 736, 1), v1_blk(1, 8, 736, 1), v1_blk(1, 8, 608, 1)
    add("stream slots sum to the region", fm + "blk.nsym", 2, 3, n2, 16, tile_m2(0x10, blocks))
    blocks[14] = v1_blk(1, 8, 33, 1)
    add("stream slots sum to the region and one slot", fm + "blk.nsym", 2, 3, n2, 16, tile_m2(0x10, blocks))
    blocks[14] = v1_blk(1, 8, 32, 1)
    add("stream slots sum to the region, one symbol below the next slot", fm + "blk.nsym", 2, 3, n2, 16, tile_m2(0x10, blocks))
    # a type 3 / 4 block with bsize of 20 and 24 (and of other sizes, last in the tile)
    for bt in (3, 4):
        for size in (8, 20, 23, 24, 25, 27, 28):
            add("gray block type %d size=%d" % (bt, size), fm + "blk.size", 2, 3, n, w, tile_m2(0x20, [v1_blk(bt, size, 7)], bwords=130))
            blocks = list(empty17)
            blocks[16] = v1_blk(bt, size, 7)
            add("last colour block type %d size=%d" % (bt, size), fm + "blk.size", 2, 3, n, w, tile_m2(0x10, blocks, bwords=20))
    for bt, size in ((0, 3), (0, 4), (0, 5), (0, 12), (1, 7), (1, 8), (1, 9), (2, 7), (2, 8), (2, 11), (5, 8), (255, 8)):
        t = tile_m2(0x20, [v1_blk(bt, size, 7)])
        add("gray block type %d size=%d" % (bt, size), fm + "blk.size", 2, 3, n, w, t)
        add("gray block type %d size=%d, one byte past L" % (bt, size), fm + "blk.size", 2, 3, n, w, put(t, 0, 0, 24, len(t) - 1), len(t))
    # frequency-table bit fields that run past endbit: b of one word, a dense table of 256 x 15 bits, a sparse one of set flags
    for bt in (3, 4):
        add("gray table type %d past endbit" % bt, fm + "bsz", 2, 3, n, w, tile_m2(0x20, [v1_blk(bt, 24, 7)], bwords=1))
        blocks = list(empty17)
        blocks[3], blocks[12] = v1_blk(bt, 24, 5), v1_blk(bt, 28, 9)
        add("colour tables type %d past endbit" % bt, fm + "bsz", 2, 3, n, w, tile_m2(0x10, blocks, bwords=2))
    for npx in (1, 2):
        add("n=%d without symbols" % npx, fm + "blk.nsym", 2, 3, npx, npx, tile_m2(0x10, empty17))
        blocks = list(empty17)
        blocks[0] = v1_blk(1, 8, 1, 0)
        add("n=%d with one symbol" % npx, fm + "blk.nsym", 2, 3, npx, npx, tile_m2(0x10, blocks))


_built = {}


def build(po):
    """-> Cases: every systematic and compound case of the three formats (built once per process)"""
    if "all" in _built:
        return _built["all"]
    cs = Cases()
    for mode, pxsz in FORMATS:
        tiles = base_tiles(po, mode, pxsz)
        seen = set()
        for name, n, w, blob in tiles:
            assert judge(mode, blob, len(blob), n, pxsz) == (ACCEPT, ""), (mode, pxsz, name)   # the rules accept what the encoder writes
            seen |= block_types(mode, blob, pxsz)
            cs.systematic("m%d.%d.%s" % (mode, pxsz, name), mode, pxsz, n, w, blob)
        assert seen == {0, 1, 2, 3, 4}, (mode, pxsz, seen)
        pre = len(cs.cases)
        compound(cs, mode, pxsz, tiles)
        for c in cs.cases[pre:]:
            c.name = "m%d.%d.%s" % (mode, pxsz, c.name)
    _built["all"] = cs
    return cs


# ---- the cases of the device test ----------------------------------------------------------------------------------------
def device_raster(po, pxsz):
    """the smallest raster of three tiles (445 rows, the width grown by a tile at a time), and its tile table"""
    w = 889
    while len(po.tile_table(w, 445, pxsz)) < 3:
        w += 444
    return w, 445, po.tile_table(w, 445, pxsz)


def device_cases(po, mode, pxsz, per_mode=15):
    """-> (raster, its file body, tile offsets, Cases, [case]): systematic edits of the MIDDLE tile of a three-tile photo, one
    rejected case per rule.  The tile's own size word is left alone where another edit reaches the rule."""
    key = ("dev", mode, pxsz)
    if key in _built:
        return _built[key]
    from xpng_amd.synth import synth_raster
    W, H, table = device_raster(po, pxsz)
    raster = synth_raster("photo", W, H, pxsz == 4, seed=11)
    body = po.encode_tiles(mode, raster)
    offs, o = [], 0
    for _ in table:
        offs.append(o)
        o += u32(body, o) & 0xFFFFFF
    assert o == len(body)
    t = 1
    n, w = table[t][2] * table[t][3], table[t][2]
    blob = body[offs[t]:offs[t + 1]]
    assert judge(mode, blob, len(blob), n, pxsz) == (ACCEPT, "") and blob[3] != 0
    cs = Cases()
    cs.systematic("dev.m%d.%d" % (mode, pxsz), mode, pxsz, n, w, blob)
    # two passes: the cases that keep the tile's first word, then the others
    picked = {}
    for keep in (True, False):
        for c in cs.cases:
            if c.verdict == REJECT and c.rule not in picked and (c.blob[:3] == blob[:3]) == keep and len(picked) < per_mode:
                picked[c.rule] = c
    _built[key] = (raster, body, offs, cs, list(picked.values()))
    return _built[key]


# ---- the parsers on the host ---------------------------------------------------------------------------------------------
def _kit():
    import _kit                                                     # (imported late: _kit imports the package's ctypes layer)
    return _kit


SANITIZE = ("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan")


def parser_text():
    """the text of the four kernels and of the records and helpers they name, cut out of the product headers"""
    cut = _kit().cut
    parts = [
        cut("common.hpp", "struct TileDesc {", "__host__ __device__ inline uint64_t kw_cap", last=False),       # TileDesc, TileSel, vtile, imglin, rup
        cut("rans_dec.hpp", "struct DecTile {", "struct WDec {", last=False),                                   # DecTile, TILE_BAD
        cut("rans_dec.hpp", "// random-access MSB-first bit read", "// ---- look-up and state update", last=False),  # bits_at
        cut("m2_encode.hpp", "constexpr uint32_t M2_STREAMS", "// Block slots (", last=False),                   # M2_*, m2_nominal, m2_slot, m2_streams_region, m2_off_stream
        cut("m2_encode.hpp", "struct M2Blk {", "\n", last=False) + "\n",
        cut("m2_decode.hpp", "struct M2DecTile {", "// what the reconstruction", last=False),                    # M2DecTile, M2_KIND_BAD
        cut("m1_decode.hpp", "__global__ void k_dec_parse(", "// ----", last=False),
        cut("m2_decode.hpp", "__global__ void k_m2_dec_parse(", "// ----", last=False),
        cut("m1_decode.hpp", "__global__ void k_dec_offsets(", "// One decode job", last=False),
    ]
    text = "\n".join(parts)
    for name in ("void k_dec_parse(", "void k_m2_dec_parse(", "void k_dec_offsets(", "void k_dec_offsets_mixed(", "struct DecTile", "TILE_BAD =",
                 "struct M2DecTile", "struct M2Blk", "M2_KIND_BAD =", "M2_SLOTS =", "m2_nominal(", "m2_slot(", "m2_streams_region(", "m2_off_stream(",
                 "uint32_t bits_at(", "struct TileDesc", "struct TileSel", "uint32_t vtile(", "uint32_t imglin(", "uint64_t rup("):
        assert name in text, name
    assert "asm" not in text and "address_space" not in text
    return text


def run_parsers_on_host(tmp_path, cs, cases=None, flags=(), sanitize=SANITIZE):
    """-> (finished process, {case name: accepted}): the host program over the cases of `cs`"""
    path = tmp_path / "hostile_cases.bin"
    n = cs.write(str(path), cases)
    r = _kit().run_kernels_on_host(tmp_path, "dec_parse_host", {"KERNEL_TEXT": parser_text()}, flags=('-DCASE_FILE="%s"' % path, *flags),
                              sanitize=sanitize, timeout=240)
    verdicts = {}
    for ln in open(str(path) + ".verdicts").read().splitlines():
        v, name = ln.split(" ", 1)
        verdicts[name] = v == "1"
    assert len(verdicts) == len({c.name for c in (cs.cases if cases is None else cases)})
    return r, verdicts, n
