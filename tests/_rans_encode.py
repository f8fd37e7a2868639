"""Checker and inputs for the rANS ENCODER tables (test infrastructure, imported by tests/test_rans_encode_tables.py; not a conftest).

- normalise_profile: the reference's frequency normalisation (scale the cumulative counts to 2^pb, then the sequential "steal"
  repair) restated on Python integers from the rule itself, with the list of steals it made.
- block_forecast: the block an encoder must write for a symbol stream - empty, one symbol, raw, dense or sparse table - with the
  lengths of the rANS candidate and of the raw block, so that a test can ask how close the choice was.
- the alpha catalogue: single-tile RGBA rasters whose level-1 alpha stream is a chosen symbol sequence (pb 15, alphabet 256).
- ctx_raster / CTX_PARAMS: RGB rasters whose level-1 context streams (pb 12, alphabet 9) reach the steal repair.
- gray_raster / gray_streams: level-2 gray tiles whose left-predictor residual stream is a catalogue stream (pb 15).
"""
from __future__ import annotations

import numpy as np

import _rans_tables as rt

BIG_W, BIG_H = 400, 300                # one tile in RGB and in RGBA; the alpha stream has BIG_N symbols
BIG_N = BIG_W * BIG_H - 1


# ---------------------------------------------------------------- the checker

def normalise_profile(hist, pb: int) -> dict:
    """hist[s] = count of symbol s.  The table the reference writes for it and how it got there:

    N = 1 + the highest used symbol, n = the number of symbols, cum[i] = (count of symbols below i << pb) // n.  Then, in symbol
    order, every used symbol i whose range is empty (cum[i + 1] == cum[i]) takes one slot from the donor: the first symbol
    with the smallest width among the widths greater than 1.  A donor below i moves the boundaries donor + 1 .. i down by one, a
    donor above moves i + 1 .. donor up by one.

    -> F (N widths), N, steals = [(i, donor, donor's width before, number of symbols tied at that width)] and the counts
    below / above (donor < i / donor > i), tied (steals that chose among two or more), donors (distinct), to_one (donors
    driven from width 2 to width 1)."""
    h = [int(v) for v in hist]
    n = sum(h)
    N = max(i for i, v in enumerate(h) if v) + 1
    cum, run = [0], 0
    for i in range(N):
        run += h[i]
        cum.append((run << pb) // n)
    steals = []
    for i in range(N):
        if h[i] == 0 or cum[i + 1] != cum[i]:
            continue
        width = [cum[j + 1] - cum[j] for j in range(N)]
        givers = [wd for wd in width if wd > 1]
        assert givers, "no symbol wider than 1: the reference has no answer for this table"
        least = min(givers)
        donor = width.index(least)
        if donor < i:
            for j in range(donor + 1, i + 1):
                cum[j] -= 1
        else:
            for j in range(i + 1, donor + 1):
                cum[j] += 1
        steals.append((i, donor, least, givers.count(least)))
    F = [cum[i + 1] - cum[i] for i in range(N)]
    assert sum(F) == 1 << pb and all((f > 0) == (c > 0) for f, c in zip(F, h))
    return dict(F=F, N=N, n=n, steals=steals,
                below=sum(d < i for i, d, _, _ in steals), above=sum(d > i for i, d, _, _ in steals),
                tied=sum(t > 1 for _, _, _, t in steals), donors=len({d for _, d, _, _ in steals}),
                to_one=sum(wd == 2 for _, _, wd, _ in steals))


def block_forecast(syms, nominalN: int, pb: int) -> dict:
    """The v2 block of a symbol stream: type 0 (empty), 1 (one symbol), 2 (raw), 3 (dense table), 4 (sparse table), its length,
    and for types 2..4 the length of the rANS candidate (cand) and of the raw block (raw) and the profile of the table.

    The table is sparse iff N + distinct * pb < N * pb; the candidate is the oracle's coding of the stream with the PROFILE's
    table in that form; raw wins iff len(candidate) >= 8 + 4 * rawWords, rawWords = ceil(bit_width(N - 1) * n / 32)."""
    from oracle import pyoracle as po
    syms = np.ascontiguousarray(syms, dtype=np.uint8)
    n = len(syms)
    if n == 0:
        return dict(type=0, length=4)
    hist = np.bincount(syms, minlength=nominalN)[:nominalN]
    distinct = int((hist > 0).sum())
    if distinct == 1:
        return dict(type=1, length=8)
    prof = normalise_profile(hist, pb)
    N = prof["N"]
    sparse = N + distinct * pb < N * pb
    cand = len(po.rans2_encode_table(prof["F"], syms, pb, sparse))
    raw = 8 + 4 * (((N - 1).bit_length() * n + 31) // 32)
    btype = 2 if cand >= raw else 3 + int(sparse)
    return dict(type=btype, length=raw if btype == 2 else cand, cand=cand, raw=raw, sparse=sparse, distinct=distinct, profile=prof)


# ---------------------------------------------------------------- alpha catalogue (pb 15, alphabet 256)

def counts(hot: dict, ones=(), fill: int = None, n: int = BIG_N) -> dict:
    """every symbol of `ones` once, the `hot` symbols as given, `fill` takes the rest up to n"""
    c = {int(s): 1 for s in ones}
    c.update(hot)
    rest = n - sum(c.values())
    assert rest >= 0 and (rest == 0 or fill is not None)
    if rest:
        c[fill] = c.get(fill, 0) + rest
    return c


# name: symbol counts of a 400 x 300 alpha stream.  The steal list depends on the histogram alone: EXPECT holds the census.
BIG_COUNTS = {
    "donor_below": counts({0: 60000, 2: 9}, range(100, 160), 4),
    "donor_above": counts({250: 60000, 252: 9}, range(10, 70), 254),
    "exhaust": counts({0: 50000, 2: 8, 6: 8, 8: 12, 200: 8}, range(20, 120), 4),
    "tied": counts({0: 50000, 10: 11, 200: 11}, list(range(50, 60)) + list(range(220, 230)), 4),
    "all_once": counts({0: 70000}, range(1, 256), 2),
    "dominant": counts({0: BIG_N - 1, 1: 1}),                  # F = {32767, 1}: no steal, the last symbol keeps the remainder
    "dominant_steal": counts({0: 1, 1: BIG_N - 1}),            # F = {1, 32767}: the single symbol comes first and steals its slot
    # symbol 0 scales to 4096 = 2^12 and symbol 2 to 1025 = 2^10 + 1 (no steal: every width is above 1)
    "pow2": counts({0: 15000, 2: 3754}, (), 4),
    # ONE steal, chosen between two donors of width 3 on either side of the taker: the table shows which of them gave (the
    # shapes above that choose among ties go on until every tied donor has given, so their tables do not depend on the order)
    "tie_once": counts({0: 50000, 10: 9, 200: 9}, [100], 4),
}
# name: (steals, below, above, donors, to_one, tied at least, block type)
EXPECT = {
    "donor_below": (43, 43, 0, 2, 1, 0, 4),
    "donor_above": (44, 0, 44, None, None, 0, 4),
    "exhaust": (73, 71, 2, 5, 4, 2, 4),
    "tied": (14, 12, 2, None, None, 1, 4),
    "all_once": (183, None, None, 1, None, 0, 3),
    "tie_once": (1, 1, 0, 1, 0, 1, 4),
}

# table form at N = 15: 14 symbols in use make the two forms equally long (15 + 14 * 15 == 15 * 15: dense); 13 in use: sparse
FORM_DIMS = (40, 25)
FORM_COUNTS = {
    "form_tie": counts({0: 800, 14: 60}, [s for s in range(1, 14) if s != 7], 1, n=999),
    "form_sparse": counts({0: 800, 14: 60}, [s for s in range(1, 14) if s not in (7, 9)], 1, n=999),
}

# raw blocks: symbols uniform in [0, 2^b); (b, w, h).  b * n mod 32 over the family holds 0, 1 and 31 (RAW_BITS_TAILS)
RAW_BITS = [(1, 8, 8), (2, 7, 7), (3, 11, 4), (5, 12, 7), (6, 7, 7), (7, 8, 7), (3, BIG_W, BIG_H), (7, BIG_W, BIG_H)]
RAW_BITS_TAILS = {0, 1, 31}

# short streams on the raw / rANS threshold, found by search_short_streams(): kind -> (trial, w, h)
SHORT_SEED, SHORT_TRIALS = 20240, 2000
SHORT_KINDS = {"raw_tie": 0, "raw_by_one_word": 4, "rans_by_one_word": -4}   # candidate length minus raw length
SHORT_PICKS = {"raw_tie": (1, 23, 6), "raw_by_one_word": (2, 37, 16), "rans_by_one_word": (5, 28, 20)}


ALPHA_NAMES = (list(BIG_COUNTS) + list(FORM_COUNTS) + [f"raw_bits{b}_{w}x{h}" for b, w, h in RAW_BITS] + list(SHORT_PICKS))
BIG_NAMES = list(BIG_COUNTS) + [f"raw_bits{b}_{w}x{h}" for b, w, h in RAW_BITS if (w, h) == (BIG_W, BIG_H)]


def _dims_of(n: int):
    """the most nearly square (w, h), w >= h >= 4, with w * h - 1 == n, or None"""
    for h in range(int((n + 1) ** 0.5), 3, -1):
        if (n + 1) % h == 0:
            return (n + 1) // h, h
    return None


def short_stream(trial: int):
    """trial -> (w, h, symbols): 20..600 symbols of a random alphabet with a geometric skew, in a raster that holds exactly them"""
    rng = np.random.default_rng([SHORT_SEED, trial])
    while True:
        n = int(rng.integers(20, 601))
        if _dims_of(n):
            break
    w, h = _dims_of(n)
    top = int(rng.choice([1, 2, 3, 5, 7, 12, 15, 31, 40, 63, 100, 127, 200, 255]))
    p = float(rng.choice([0.05, 0.1, 0.2, 0.3, 0.5, 0.7]))
    syms = np.minimum(rng.geometric(p, n) - 1, top).astype(np.uint8)
    syms[int(rng.integers(0, n))] = top
    return w, h, syms


def search_short_streams(trials: int = SHORT_TRIALS) -> dict:
    """kind -> (first trial that gives it, w, h, how many trials gave it): the search behind SHORT_PICKS (CPU only)"""
    found = {}
    for t in range(trials):
        w, h, syms = short_stream(t)
        f = block_forecast(syms, 256, 15)
        if f["type"] < 2:
            continue
        for kind, diff in SHORT_KINDS.items():
            if f["cand"] - f["raw"] == diff:
                first = found.get(kind, (t, w, h, 0))
                found[kind] = first[:3] + (first[3] + 1,)
    return found


def _alpha_raster(syms, w: int, h: int, seed: int, kind: str = "photo") -> np.ndarray:
    """RGB of synth_raster(kind) - one colour ("flat") under the short streams, whose files would otherwise not be smaller than
    their rasters and be rewritten at level 7 - with the alpha plane that carries syms; pixels of alpha 0 are zeroed"""
    from xpng_amd.synth import synth_raster
    r = synth_raster(kind, w, h, True, seed=seed).copy()
    r[..., 3] = rt.alpha_plane(np.ascontiguousarray(syms, dtype=np.uint8), w, h)
    r[r[..., 3] == 0] = 0
    return np.ascontiguousarray(r)


def alpha_catalogue() -> dict:
    """name -> (raster, the alpha stream it carries), in the order of ALPHA_NAMES"""
    out = {}
    for k, (name, c) in enumerate(BIG_COUNTS.items()):
        syms = rt.symbols_from_counts(c, np.random.default_rng(100 + k))
        out[name] = (_alpha_raster(syms, BIG_W, BIG_H, 3 + k), syms)
    for k, (name, c) in enumerate(FORM_COUNTS.items()):
        syms = rt.symbols_from_counts(c, np.random.default_rng(200 + k))
        out[name] = (_alpha_raster(syms, *FORM_DIMS, 20 + k), syms)
    for k, (b, w, h) in enumerate(RAW_BITS):
        rng = np.random.default_rng(300 + k)
        syms = rng.integers(0, 1 << b, w * h - 1).astype(np.uint8)
        syms[int(rng.integers(0, len(syms)))] = (1 << b) - 1     # the top symbol is present: b bits per symbol
        out[f"raw_bits{b}_{w}x{h}"] = (_alpha_raster(syms, w, h, 30 + k, "photo" if (w, h) == (BIG_W, BIG_H) else "flat"), syms)
    for k, (name, pick) in enumerate(SHORT_PICKS.items()):
        w, h, syms = short_stream(pick[0])
        assert (w, h) == tuple(pick[1:])
        out[name] = (_alpha_raster(syms, w, h, 40 + k, "flat"), syms)
    return out


# ---------------------------------------------------------------- context streams (pb 12, alphabet 9)

# (amp, k, mag, seed): every channel (x // 3 + y // 5) + uniform noise in [0, amp); k isolated pixels raised by mag
# in this order: donor below / sparse table, donor below / dense, donor above / sparse, donor above / dense, both directions in one
# block, a steal chosen among tied donors (found by a CPU search over amp, k, mag and seed; the census test pins what they reach)
CTX_PARAMS = [(1, 5, 40, 0), (8, 5, 40, 0), (4, 30, 40, 0), (16, 0, 0, 1), (16, 5, 40, 1), (16, 200, 40, 1)]


def ctx_raster(amp: int, k: int, mag: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng([7, amp, k, mag, seed])
    yy, xx = np.mgrid[0:BIG_H, 0:BIG_W]
    r = (xx // 3 + yy // 5)[..., None] + rng.integers(0, amp, (BIG_H, BIG_W, 3))
    if k:
        spots = rng.choice((BIG_W // 4) * (BIG_H // 4), k, replace=False)        # one per 4 x 4 cell at most: isolated
        r[4 * (spots // (BIG_W // 4)) + 1, 4 * (spots % (BIG_W // 4)) + 1] += mag
    assert r.max() < 256
    return np.ascontiguousarray(r.astype(np.uint8))


def ctx_streams(raster):
    """[(tile index, stream c, raw histogram F[c], symbols)] of every tile of a level-1 encode, as the oracle forms them"""
    from oracle import pyoracle as po
    h, w, ch = raster.shape
    out = []
    for ti, t in enumerate(po.tile_table(w, h, ch)):
        pr, _ = po.choose_predictor(raster, t)
        planes = po.m1_planes(raster, t, pr)
        st = po.m1_streams(raster, t, planes)
        out += [(ti, c, st["F"][c], st["ctx"][c]) for c in range(9)]
    return out


def ctx_census(profiles) -> dict:
    """what the context family reaches, counted in blocks over a list of (profile, block type): steals with the donor below /
    above the taker under a dense (type 3) and under a sparse (type 4) table, both directions in one block, a tied choice"""
    def blocks(cond):
        return sum(1 for p, t in profiles if cond(p, t))
    return dict(below_dense=blocks(lambda p, t: p["below"] and t == 3), below_sparse=blocks(lambda p, t: p["below"] and t == 4),
                above_dense=blocks(lambda p, t: p["above"] and t == 3), above_sparse=blocks(lambda p, t: p["above"] and t == 4),
                both_in_one=blocks(lambda p, t: p["below"] and p["above"]), tied=blocks(lambda p, t: p["tied"] > 0))


# ---------------------------------------------------------------- level-2 gray (pb 15, alphabet 256)

GRAY_NAMES = ("exhaust", "all_once", "tie_once")


def gray_raster(name: str) -> np.ndarray:
    """R = G = B = the plane whose left-predictor residuals (the pixel above in column 0) are the catalogue stream `name`"""
    k = list(BIG_COUNTS).index(name)
    g = rt.alpha_plane(rt.symbols_from_counts(BIG_COUNTS[name], np.random.default_rng(100 + k)), BIG_W, BIG_H)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def gray_streams(g: np.ndarray):
    """the four residual streams of a gray tile (predictor 0 left, 1 up, 2 average, 3 gradient; row 0 from the left, column 0
    from above), each as zig-zag symbols of pixels 1 .. w * h - 1"""
    v = g.astype(np.int64)
    L, U, UL = np.roll(v, 1, axis=1), np.roll(v, 1, axis=0), np.roll(np.roll(v, 1, axis=0), 1, axis=1)
    pred = [L.copy(), U.copy(), (L + U + 1) >> 1, (3 * L + 3 * U - 2 * UL + 2) >> 2]
    out = []
    for p in pred:
        p[0, :] = L[0, :]
        p[:, 0] = U[:, 0]
        d = (((v - p) + 128) & 255) - 128
        out.append(np.where(d >= 0, 2 * d, -2 * d - 1).astype(np.uint8).reshape(-1)[1:])
    return out
