"""Calls in sequence on one context (test infrastructure for tests/test_context_sequences.py): the catalogue of rasters, the
orderings and the CPU census of what changes between consecutive calls.

A context keeps its workspace between calls and clears next to none of it: a call is right only because each of its launches
overwrites what its next reader takes.  A sequence therefore has to put DIFFERENT content through one context call after call, and
the catalogue is built so that consecutive calls leave the most different state behind: every raster of a family has the same
geometry (900 x 460, two tiles of 456 and 444 columns) and is composed tile by tile from `kinds` (below), arranged so that a tile
changes its kind, its predictor, its stream lengths and its block forms from one raster to the next.  `circuit` orders a family so
that every ordered pair (previous raster, current raster) occurs exactly once; `profile` reads what the oracle wrote for a raster,
tile by tile, and `transitions` collects what changed between consecutive calls of a sequence, for the census.

No RNG library: every value comes from tests/_steered.py and xpng_amd/synth.py, so the bytes do not depend on the numpy version."""
import numpy as np

import _steered as S
from xpng_amd.synth import _hash_np, synth_raster

GEOM = (900, 460)            # two tiles, 456 and 444 columns: one context serves a whole family
RANGE_GEOM = (1000, 900)     # four tiles (2 x 2): tile ranges and regions
FORM_GEOM = (1903, 328)      # three tiles in a row, 701 / 601 / 601 columns: tile 0 is wider than TR_MAXW = 672, the others are not
TR_MAXW = 672                # xpng_amd/csrc/m1_encode.hpp


# ------------------------------------------------------------------------------------------------ the kinds a tile can have
def _noise_alpha(w, h, seed):
    """alpha bytes uniform over 1..255: their differences fill the alphabet, so the alpha block is stored raw"""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    a = (_hash_np(xs, ys, 3, seed) >> np.uint64(24)).astype(np.uint8)
    return np.where(a == 0, 1, a).astype(np.uint8)


def _near_flat(w, h, alpha, steps, noisy_alpha):
    """One colour with single outlier pixels `steps` above it.  Everything but the outliers' neighbourhoods falls into context 0; a
    lone outlier leaves one-symbol blocks in the contexts its size selects ([8, 100]: contexts 3, 5, 7, 8) and empty blocks
    elsewhere; the eight steps 1 .. 100 leave a few different symbols in every context from 2 on - raw (type 2) blocks."""
    r = synth_raster("flat", w, h, alpha).copy()
    for i, s in enumerate(steps):
        r[(30 + 50 * i) % h, (20 + 40 * i) % w, :3] = 0x4D + s
    if noisy_alpha:
        r[..., 3] = _noise_alpha(w, h, 9)
    return r


def _tile_kind(kind, w, h, alpha):
    """The (h, w, 3|4) content of one tile of `kind`, for the kinds that are built at the tile's own size."""
    if kind == "flat":                                # empty blocks and one one-symbol block (RGBA: a one-symbol alpha block too)
        return synth_raster("flat", w, h, alpha)
    if kind == "near_one":
        return _near_flat(w, h, alpha, [8, 100], False)
    if kind == "near_raw":                            # RGBA: with a raw alpha block
        return _near_flat(w, h, alpha, [1, 2, 4, 8, 16, 32, 64, 100], alpha)
    if kind == "raw":                                 # noise in every channel: the tile falls back to raw
        r = synth_raster("noise", w, h, alpha).copy()
        if alpha:
            r[..., 3] = _noise_alpha(w, h, 9)
        return r
    if kind == "clear":                               # alpha 0 over the whole tile: it codes no pixel
        assert alpha
        return np.zeros((h, w, 4), np.uint8)
    if kind == "photo":
        return synth_raster("photo", w, h, alpha)
    if kind == "tail":                                # the last third transparent: the last coded pixel lies further up
        assert alpha
        r = synth_raster("photo", w, h, True).copy()
        r[2 * h // 3:] = 0
        r[2 * h // 3 - 1, w // 2:] = 0                # ... and in the middle of a row
        return r
    if kind == "one":                                 # level 2: a single-colour tile
        return np.full((h, w, 3), 77, np.uint8)
    if kind.startswith("gray_"):                      # level 2: every gray mode of S.gray, the raw gray tile included
        assert not alpha
        return S.gray(kind[5:], w, h)
    raise ValueError(kind)


_full = {}


def compose(w, h, alpha, kinds):
    """(h, w, 3|4) raster whose tile i has kinds[i % len(kinds)].  pr0 .. pr3 are S.steered (all nine contexts in use, long k, the
    chooser returns that predictor): it is tile-local, so a tile cut out of the full-size raster keeps its predictor."""
    out = np.zeros((h, w, 3 + int(alpha)), np.uint8)
    for ti, (tx, ty, tw, th) in enumerate(S.tile_table(w, h)):
        kind = kinds[ti % len(kinds)]
        if kind.startswith("pr"):
            key = (kind, w, h, alpha)
            if key not in _full:
                _full[key] = S.steered(int(kind[2:]), w, h, alpha)
            out[ty:ty + th, tx:tx + tw] = _full[key][ty:ty + th, tx:tx + tw]
        else:
            out[ty:ty + th, tx:tx + tw] = _tile_kind(kind, tw, th, alpha)
    return out


# ------------------------------------------------------------------------------------------------ the families
# name -> (the kind of tile 0, the kind of tile 1).  Tile 0 of the level-1 families goes through the four predictors, a raw
# tile and (RGBA) a tile that codes nothing; tile 1 through flat, one-symbol and raw blocks, coded blocks and a raw tile.  RGBA: the
# clear tile stands in tile 1 of one raster and in tile 0 of another (its mirror).
RGBA_L1 = {
    "a_pr0_clear": ("pr0", "clear"),
    "a_pr1_raw": ("pr1", "raw"),
    "a_pr2_nearone": ("pr2", "near_one"),
    "a_pr3_flat": ("pr3", "flat"),
    "a_raw_pr2": ("raw", "pr2"),
    "a_clear_nearraw": ("clear", "near_raw"),
    "a_tail_tail": ("tail", "tail"),
}
RGB_L1 = {
    "b_pr0_flat": ("pr0", "flat"),
    "b_pr1_raw": ("pr1", "raw"),
    "b_pr2_nearone": ("pr2", "near_one"),
    "b_pr3_nearraw": ("pr3", "near_raw"),
    "b_raw_pr1": ("raw", "pr1"),
    "b_flat_photo": ("flat", "photo"),
}
# Level 2: tile 0 goes through the seven kinds {colour, gray left / up / average / gradient, raw gray, single colour} (colour twice,
# with predictors 0 and 2), tile 1 through the same list three places on (colour with predictors 1 and 3): the two tiles swap kinds.
_L2_T0 = ["pr0", "gray_left", "gray_up", "pr2", "gray_avg", "gray_grad", "gray_raw", "one"]
_L2_T1 = ["pr1", "gray_left", "gray_up", "pr3", "gray_avg", "gray_grad", "gray_raw", "one"]
RGB_L2 = {f"c_{_L2_T0[i]}_{_L2_T1[(i + 3) % 8]}".replace("gray_", "g"): (_L2_T0[i], _L2_T1[(i + 3) % 8]) for i in range(8)}
# The geometries of more than two tiles: four steered rasters, one per predictor (tile ranges, regions, the stage entry).
WIDE = {f"{f}_pr{p}_{w}x{h}": ((f"pr{p}",), w, h) for f in ("a", "b") for p in range(4) for (w, h) in (RANGE_GEOM, FORM_GEOM)}
# 64 x 48, one tile: the production pairing (a batch of 230 selects the wide chains and the 256-thread routing by itself)
SMALL = {f"s_{k}": ((k,), 64, 48) for k in ("pr0", "pr1", "pr2", "pr3", "photo", "flat", "raw", "clear", "near_one", "tail")}

FAMILIES = {"rgba_l1": RGBA_L1, "rgb_l1": RGB_L1, "rgb_l2": RGB_L2}

_cache = {}


def raster(name):
    """The named raster (read-only, shared between tests)."""
    if name not in _cache:
        if name in WIDE or name in SMALL:
            kinds, w, h = (WIDE if name in WIDE else SMALL)[name]
        else:
            kinds, (w, h) = next(f[name] for f in FAMILIES.values() if name in f), GEOM
        r = np.ascontiguousarray(compose(w, h, name.startswith(("a_", "s_")), kinds))
        r.setflags(write=False)
        _cache[name] = r
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the orderings
def circuit(k):
    """An Eulerian circuit of the complete directed graph on k nodes (Hierholzer, edges taken in ascending order): k (k - 1) + 1
    nodes from 0 back to 0, every ordered pair (previous, current) of different nodes exactly once."""
    nxt = {v: [u for u in range(k) if u != v][::-1] for v in range(k)}      # (popped from the end: ascending)
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def sequence(family):
    """The names of a family in the order of its circuit."""
    names = list(FAMILIES[family] if isinstance(family, str) else family)
    return [names[i] for i in circuit(len(names))]


# ------------------------------------------------------------------------------------------------ the census
def _u32(b, o):
    return int.from_bytes(b[o:o + 4], "little")


FORMS = {0: "empty", 1: "one", 2: "raw", 3: "coded", 4: "coded"}            # v2 block types (dense and sparse tables: both coded)
GRAY_KINDS = {0x20: "gray_left", 0x21: "gray_up", 0x22: "gray_avg", 0x23: "gray_grad", 0x28: "gray_raw"}


def profile(level, blobs, w, h, ch):
    """What the oracle wrote, tile by tile (tile headers: encode_tile_m1 / encode_tile_m2 / encode_tile_gray in
    oracle/xpng_oracle.c).  Per tile a dict with `off`, `size` and `kind`:
      level 1   kind "raw", or "coded" / "nothing" (a coded tile whose nine context streams are all empty) with `pr`, `k` (the bytes
                of the k words), `ctx_n` (symbols per context stream), `alpha` (bytes of the alpha block, RGBA) and `forms` (the form
                of each of the 9 or 10 blocks)
      level 2   kind "raw", "one", "colour" (with `pr`) or one of GRAY_KINDS"""
    out, o = [], 0
    for _ in S.tile_table(w, h):
        h0 = _u32(blobs, o)
        typ, size = h0 >> 24, h0 & 0xFFFFFF
        t = {"off": o, "size": size}
        if typ == 0:
            t["kind"] = "raw"
        elif typ == 255:
            t["kind"] = "one"
        elif level == 1:
            assert typ >> 4 == 1 and ((typ >> 2) & 1) == (ch == 4)
            p = o + 4
            t["pr"], t["k"] = typ & 3, _u32(blobs, p)
            p += t["k"]
            t["ctx_n"], t["forms"] = [], []
            for c in range(9 + (ch == 4)):
                hdr = _u32(blobs, p)
                t["forms"].append(FORMS[hdr >> 24])
                if c < 9:
                    t["ctx_n"].append(_u32(blobs, p + 4) & 0xFFFFFF if hdr >> 24 else 0)
                else:
                    t["alpha"] = hdr & 0xFFFFFF
                p += hdr & 0xFFFFFF
            assert p == o + size
            t["kind"] = "coded" if any(t["ctx_n"]) else "nothing"
        elif typ >> 4 == 2:
            t["kind"] = GRAY_KINDS[typ]
        else:
            assert typ >> 4 == 1
            t["kind"], t["pr"] = "colour", typ & 3
        out.append(t)
        o += size
    assert o == len(blobs)
    return out


def transitions(profiles):
    """What changes, on some tile, between consecutive entries of `profiles` (a list of (level, profile)).  Members:
      ("ctx", c, "shrink" | "grow")   context stream c of a level-1 tile gets shorter / longer (both calls code the tile)
      ("k", ...), ("alpha", ...)      the same for the k words and the alpha block
      ("form", a, b)                  a level-1 block goes from form a to form b (the same slot of the same tile)
      ("tile", a, b)                  a level-1 tile goes from kind a to kind b
      ("pr", a, b)                    the predictor of a level-1 coded tile changes from a to b
      ("l2", a, b)                    a level-2 tile goes from kind a to kind b
      ("l2_pr", a, b)                 the predictor of a level-2 colour tile changes"""
    out = set()

    def moved(what, a, b):
        if a != b:
            out.add(what + ("shrink" if b < a else "grow",))

    for (la, pa), (lb, pb) in zip(profiles, profiles[1:]):
        if la != lb:
            continue
        for a, b in zip(pa, pb):
            if la == 2:
                out.add(("l2", a["kind"], b["kind"]))
                if "pr" in a and "pr" in b:
                    out.add(("l2_pr", a["pr"], b["pr"]))
                continue
            out.add(("tile", a["kind"], b["kind"]))
            if "pr" not in a or "pr" not in b:
                continue
            out.add(("pr", a["pr"], b["pr"]))
            for c in range(9):
                moved(("ctx", c), a["ctx_n"][c], b["ctx_n"][c])
            moved(("k",), a["k"], b["k"])
            if "alpha" in a:
                moved(("alpha",), a["alpha"], b["alpha"])
            for fa, fb in zip(a["forms"], b["forms"]):
                out.add(("form", fa, fb))
    return out


BLOCK_FORMS = ("empty", "one", "coded", "raw")
L2_KINDS = ("colour", "gray_left", "gray_up", "gray_avg", "gray_grad", "gray_raw", "one")


def wanted(family):
    """The transitions the issue asks a family's sequence for."""
    if family == "rgb_l2":
        return {("l2", a, b) for a in L2_KINDS for b in L2_KINDS if a != b}
    want = {("ctx", c, d) for c in range(9) for d in ("shrink", "grow")} | {("k", d) for d in ("shrink", "grow")}
    want |= {("form", a, b) for a in BLOCK_FORMS for b in BLOCK_FORMS if a != b}
    want |= {("tile", a, b) for a in ("raw", "coded") for b in ("raw", "coded") if a != b}
    want |= {("pr", a, b) for a in range(4) for b in range(4) if a != b}
    if family == "rgba_l1":
        want |= {("alpha", d) for d in ("shrink", "grow")} | {("tile", "nothing", "coded"), ("tile", "coded", "nothing")}
    return want


# Transitions that no raster of a family can reach, each with its reason.  The census asserts that they stay unseen.
UNREACHABLE = {
    ("rgb_l1", ("tile", "nothing", "coded")): "only a transparent pixel is left uncoded, and an RGB raster has none: every RGB tile "
                                              "codes all its pixels",
    ("rgb_l1", ("tile", "coded", "nothing")): "as above",
}
