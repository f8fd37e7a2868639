"""The level-2 colour streams (17 rANS v1 streams at 14 probability bits per tile): tables, block choice, symbol lookup, the splice
into the shared bit stream, on inputs built for the branches they are named after (tests/_m2_colour.py).

These streams run through kernels nothing else uses: k_m2_streams, k_rans1_encode, k_rans1_prep / chain / finish, k_m2_bits (encode);
k_m2_dec_parse, k_rans1_decode, k_rans1_dec_prep, k_rans1_dec_chain<false> (slots 0..9, 11: register search, 32-word ring),
k_rans1_dec_chain<true> (slots 10, 12..16: coarse byte and forward scan, 64-word ring), k_m2_dec_resid (decode).

CPU part (not marked gpu): the parser, the numpy restatement of the stream formation and the oracle's v1 decoder agree on every
catalogue tile; v1_forecast gives the oracle's block type, length and table for every block; the census (run with -s to read it; one
run is kept as profiles/m2_colour_census.txt) proves that every entry reaches what it is named after; flipping one rule of the
checker at a time changes a forecast, so the inputs tell the rules apart; the catalogue is pinned to the compiled reference through
tests/golden/m2_colour.json (oracle/make_m2_colour_golden.py).

GPU part (-m gpu): everything is on bytes, no tolerance.  Context.fetch serves the blocks of a level-1 encode only, so the blocks of
a level-2 tile are compared by running the parser over the device's tile: a failure names the slot and what differs.

What arithmetic makes unreachable is listed in UNREACHABLE with its proof and asserted to stay unseen."""
import json
import os

import numpy as np
import pytest

import _m2_colour as mc
import _rans_encode as re_
import _rans_tables as rt

from _kit import gpu, md5, po, ROOT, SENTINEL
from conftest import GOLD

FORMS = ["XPNG_NARROW_RANS", "XPNG_WIDE_RANS"]
NAMES = mc.names()

UNREACHABLE = {
    "dense/sparse equality": "a v1 table always has the slot's nominal N entries, so the forms are equally long iff (N - d) + 15 d == 14 N, "
                             "i.e. 14 d == 13 N; N is 8, 9, 16, 32, 64, 128 or 256, none a multiple of 14, so no count d of used symbols "
                             "gives equality (and '<=' for '<' in the form rule cannot change any block)",
    "class 1 dense": "symbol 0 cannot occur in class 1: at most 7 of 8 entries are used, 1 + 7 * 15 = 106 < 8 * 14 = 112: always sparse",
    "class 2 dense": "the 8 symbols with every field below 2 cannot occur in class 2: at most 56 of 64 used, 8 + 56 * 15 = 848 < 896",
    "context raw tie": "N = 9: a sparse table has 9 + 14 d bits, an odd number, and a dense one 126; 8 * bytes is a multiple of 32 and "
                       "rawBits * n = 4 n a multiple of 4: neither 9 + 14 d + 32 k nor 126 + 32 k is one",
}


def _hist(syms, N):
    return np.bincount(syms, minlength=N)[:N]


@pytest.fixture(scope="module")
def cat(po):
    """name -> raster, predictor, designed streams, the oracle's tile and file, and for a coded colour tile the parsed tile, the
    restated streams and the forecast of every slot: computed once, shared, never changed"""
    out = {}
    for name in NAMES:
        raster, pr, vseq, streams = mc.entry(name)
        r = np.ascontiguousarray(raster)
        h, w, _ = r.shape
        assert len(po.tile_table(w, h, 3)) == 1, name
        tile = po.encode_tiles(2, r)
        e = dict(raster=r, w=w, h=h, pr=pr, streams=streams, tile=tile, coded=tile[3] >> 4 == 1)
        if e["coded"]:
            e["parsed"] = mc.parse_colour_tile(tile)
            e["syms"] = mc.colour_streams(r, (0, 0, w, h), e["parsed"]["pr"])
            e["forecast"] = [mc.v1_forecast(e["syms"][s], mc.NOMINAL[s]) for s in range(17)]
        out[name] = e
    return out


def _big_names(cat):
    return [n for n in NAMES if (cat[n]["w"], cat[n]["h"]) == (mc.W, mc.H)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_parser_streams_and_oracle_decode_agree(po, cat):
    """Every catalogue raster is one tile, round-trips through the oracle, is neither gray nor single-colour, takes the designed
    predictor, and - unless it is too small to be coded - gives the designed class streams; all 17 streams are recovered from the
    oracle's bytes by the parser and the oracle's v1 decoder, and equal the restated stream formation."""
    raw_tiles = []
    for name, e in cat.items():
        r, w, h = e["raster"], e["w"], e["h"]
        assert np.array_equal(po.decode_tiles(2, e["tile"], w, h, 3), r), name
        assert e["tile"][3] != 255 and e["tile"][3] >> 4 != 2, (name, "gray or single-colour")
        assert not (r[..., 0] == r[..., 1]).all() and len(np.unique(r.reshape(-1, 3), axis=0)) > 1, name
        assert po.choose_predictor(r, (0, 0, w, h))[0] & 3 == e["pr"], (name, "the chooser did not take the designed predictor")
        designed = mc.colour_streams(r, (0, 0, w, h), e["pr"])
        for c, s in e["streams"].items():
            assert np.array_equal(designed[8 + c], np.asarray(s, np.uint8)), (name, "class", c)
        if not e["coded"]:
            assert e["tile"][3] == 0 and len(e["tile"]) == 3 * w * h + 4, name
            raw_tiles.append(name)
            continue
        pt = e["parsed"]
        assert pt["pr"] == e["pr"] and pt["first"] == tuple(int(v) for v in r[0, 0]), name
        assert sum(sl["n"] for sl in pt["slots"][:9]) == w * h - 1, name
        for s in range(17):
            assert np.array_equal(mc.slot_symbols(pt, s), e["syms"][s]), (name, s)
            sl = pt["slots"][s]
            if sl["type"] == 1:
                assert (e["syms"][s] == sl["syms"]).all(), (name, s)
            if sl["type"] == 2:
                assert np.array_equal(sl["syms"], e["syms"][s]), (name, s)
    # the tiles too small to be coded (17 block headers alone outweigh their pixels) still run the encoder's stream kernels
    assert set(raw_tiles) == {"tiny_3x2", "tiny_4x4", "tiny_5x4", "tiny_9x7"}, raw_tiles


def test_forecast_equals_the_oracle_blocks(po, cat):
    """v1_forecast against the oracle for every block of every coded tile: type, length, table, bits put into b; and against the
    oracle's stand-alone v1 coder (block and bits)."""
    types = set()
    for name, e in cat.items():
        if not e["coded"]:
            continue
        for s, (sl, f) in enumerate(zip(e["parsed"]["slots"], e["forecast"])):
            assert (sl["type"], len(sl["block"]), sl["bit1"] - sl["bit0"]) == (f["type"], f["length"], f["bits"]), (name, s)
            if sl["type"] >= 3:
                assert np.array_equal(sl["F"], f["F"]) and f["type"] == 3 + f["sparse"], (name, s)
            blk, bits, nb = po.rans1_encode(_hist(e["syms"][s], mc.NOMINAL[s]), mc.NOMINAL[s], e["syms"][s], mc.PB)
            assert blk == sl["block"] and nb == f["bits"], (name, s)
            types.add((s >= 9, sl["type"]))
    assert types == {(k, t) for k in (False, True) for t in range(5)}


def test_raw_edge_search_finds_the_committed_picks():
    assert mc.search_raw_edges() == mc.RAW_EDGE_PICKS
    assert {k for k, _ in mc.RAW_EDGE_PICKS} == set(mc.RAW_EDGE_KINDS) and {c for _, c in mc.RAW_EDGE_PICKS} == {3, 4, 5, 6, 7, 8}
    assert mc.search_ctx_edges() == mc.CTX_EDGE_PICKS and set(mc.CTX_EDGE_PICKS) == set(mc.RAW_EDGE_KINDS) - {"raw_tie"}


def _rans_slots(cat, names=None):
    for name in names or NAMES:
        e = cat[name]
        if e["coded"]:
            for s, (sl, f) in enumerate(zip(e["parsed"]["slots"], e["forecast"])):
                if sl["type"] >= 3:
                    yield name, s, sl, f


def test_census(po, cat):
    """What the catalogue reaches, counted on the CPU.  Printed with -s; profiles/m2_colour_census.txt keeps one run."""
    assert "#define XPNG_W1D_CBITS %d\n" % mc.W1D_CBITS in open(os.path.join(ROOT, "xpng_amd", "csrc", "rans1_wide_dec.hpp")).read()
    alph = {16: 256, 15: 128, 14: 64, 13: 32, 12: 16, 10: 64}
    steal = {}            # (alphabet tag, dense?) -> set of what was seen
    per_alph = {}
    look, trace, offs, nws, lens = {}, {}, set(), set(), set()
    raw_widths, types_in_tile, long_raw = {}, {}, []
    for name, e in cat.items():
        if not e["coded"]:
            print(f"{name}: {e['w']} x {e['h']}, raw tile (too small to be coded)")
            continue
        pt = e["parsed"]
        types_in_tile[name] = {sl["type"] for sl in pt["slots"]}
        raw_widths[name] = {(mc.NOMINAL[s] - 1).bit_length() for s, sl in enumerate(pt["slots"]) if sl["type"] == 2}
        line = [f"{name}: {e['w']} x {e['h']}, pr {pt['pr']}, {len(e['tile'])} B, b {pt['bsz']} B"]
        for s, sl in enumerate(pt["slots"]):
            if s >= 9:
                lens.add(sl["n"])
            if sl["type"] >= 2:
                offs.add(sl["bit0"] % 32)
            if sl["type"] == 2:
                bits = sl["bit1"] - sl["bit0"]
                line.append(f"  slot {s}: raw n {sl['n']}, {bits} bits at offset {sl['bit0'] % 32}")
                if bits > 256 * 32:
                    long_raw.append((name, s, bits))
        for _, s, sl, f in _rans_slots(cat, [name]):
            p, cp = f["profile"], mc.colour_profile(sl["F"], s)
            tag = "ctx" if s < 9 else ("c2" if s == 10 else alph.get(s, "small"))
            seen = steal.setdefault((tag, sl["type"] == 3), set())
            per_alph[mc.NOMINAL[s]] = per_alph.get(mc.NOMINAL[s], 0) + len(p["steals"])
            seen |= {k for k in ("below", "above", "tied", "to_one") if p[k]}
            if len(p["steals"]) == 1 and p["steals"][0][3] >= 2:
                i, donor, width, ties = p["steals"][0]
                others = [j for j in range(p["N"]) if j != donor and p["F"][j] == width]
                assert p["F"][donor] == width - 1 and others and min(others) > donor, (name, s, "the first tied donor gave")
                seen.add("which")
            tr = mc.refill_trace(sl["block"], sl["F"], sl["n"])
            assert np.array_equal(tr["syms"], e["syms"][s]) and tr["used"] == tr["nw"], (name, s)
            trace[(name, s)] = tr
            look[(name, s)] = cp
            nws.add(tr["nw"])
            x = (f"  slot {s}: type {sl['type']} n {sl['n']} offset {sl['bit0'] % 32}; steals {len(p['steals'])} (below {p['below']}, above "
                 f"{p['above']}, tied {p['tied']}, to width 1 {p['to_one']}); used {cp['used']} holes {cp['holes']} min width {cp['min_width']}; "
                 f"narrow: hot {cp['hot0']}/{cp['hot1']}{' tie' if cp['hot_tie'] else ''} coarse scan {cp['coarse_scan']}; ")
            x += (f"wide scan: max_bound {cp['max_bound']} zero steps {cp['zero_steps']} width-1 run {cp['width1_run']}; " if cp["wide"] == "scan"
                  else f"wide reg{' sym8' if cp['sym8'] else ''}; ")
            line.append(x + f"nw {tr['nw']}, words per block max {tr['max8']}, idle blocks {tr['idle8']}, margin {f['margin']}")
        print("\n".join(line))
    print("steals per alphabet:", dict(sorted(per_alph.items())))
    print("steal census:", {str(k): sorted(v) for k, v in sorted(steal.items(), key=str)})
    print("piece offsets mod 32:", sorted(offs))
    # ---- steals
    full = {"below", "above", "tied", "to_one", "which"}
    for tag in (256, 64, "ctx"):
        assert steal[(tag, False)] >= full and steal[(tag, True)] >= full, (tag, steal[(tag, False)], steal[(tag, True)])
    assert steal[("c2", False)] >= {"below", "above", "tied", "to_one", "which"} and ("c2", True) not in steal   # UNREACHABLE: class 2 dense
    for N in (16, 32, 128):
        assert per_alph[N] >= 1 and steal[(N, False)] and steal[(N, True)], N
    # ---- table form and raw threshold
    for N in mc.NOMINAL:
        assert all((N - d) + 15 * d != 14 * N for d in range(N + 1)), UNREACHABLE["dense/sparse equality"]
        if N == 9:
            assert all((9 + 14 * d + 32 * k) % 4 for d in range(10) for k in range(4)) and 126 % 4, UNREACHABLE["context raw tie"]
    d15, s14 = cat["c4_form_dense15"]["forecast"][12], cat["c4_form_sparse14"]["forecast"][12]
    assert (d15["distinct"], d15["type"], s14["distinct"], s14["type"]) == (15, 3, 14, 4)      # either side of the form boundary at N = 16
    for (kind, c), _ in mc.RAW_EDGE_PICKS.items():
        f = cat[f"{kind}_c{c}"]["forecast"][8 + c]
        lo, hi = mc.RAW_EDGE_KINDS[kind]
        assert lo <= f["margin"] <= hi and f["type"] == (2 if f["margin"] >= 0 else 3 + f["sparse"]), (kind, c, f["margin"])
    for kind, (_, c) in mc.CTX_EDGE_PICKS.items():                                              # the same for a context stream (alphabet 9)
        f = cat[f"ctx_{kind}"]["forecast"][c]
        assert mc.RAW_EDGE_KINDS[kind][0] <= f["margin"] <= mc.RAW_EDGE_KINDS[kind][1], (kind, c, f["margin"])
    for name, e in cat.items():
        if e["coded"]:
            assert e["parsed"]["slots"][9]["type"] != 3 and e["parsed"]["slots"][10]["type"] != 3, (name, UNREACHABLE["class 1 dense"])
    # ---- lookup
    big = {k: v for k, v in look.items() if v["wide"] == "scan"}
    small = {k: v for k, v in look.items() if v["wide"] == "reg"}
    assert look[("c8_scan31", 16)]["max_bound"] >= 31 and look[("c8_scan31", 16)]["zero_steps"] == 0     # 31 real boundaries in a bucket
    assert look[("c8_zero_gap", 16)]["zero_steps"] >= 200
    assert look[("c8_equal", 16)]["equal"] and look[("c8_equal", 16)]["hot_tie"] and look[("c8_equal", 16)]["used"] == 128
    assert {v["slot"] for v in big.values()} == set(mc.BIG_SLOTS) and {v["slot"] for v in small.values()} == set(mc.SMALL_SLOTS)
    assert any(v["used"] < 9 and v["holes"] for v in small.values()) and any(v["sym8"] for v in small.values())
    assert any(v["min_width"] == 1 and v["max_width"] >= 1 << 13 and v["used"] <= 3 for v in small.values())
    assert any(v["coarse_scan"] >= 7 and v["zero_steps"] == 0 for v in big.values())                # 7 boundaries in a group of 8 slots
    # ---- clustered streams
    clustered = [n for n in NAMES if n.endswith("_cluster")]
    for name in clustered:
        for (nm, s), tr in trace.items():
            if nm == name and s in (0, 8 + max(cat[name]["streams"], key=lambda c: len(cat[name]["streams"][c]))):
                print(f"clustered {name} slot {s}: words per block max {tr['max8']}, idle blocks {tr['idle8']}, nw {tr['nw']}")
    assert max(tr["max8"] for (nm, s), tr in trace.items() if nm in clustered) <= 8                  # 8 * 14 bits: at most 4 refills per state
    for name in ("c8_donor_below_cluster", "c8_exhaust_cluster", "c8_scan31_cluster", "c7_steal_sparse_cluster", "c6_donor_below_cluster"):
        s = 8 + int(name[1])
        assert trace[(name, s)]["max8"] >= 7 and cat[name]["parsed"]["slots"][s]["n"] > 1 << 15, (name, trace[(name, s)]["max8"])
        assert trace[(name.replace("_cluster", ""), s)]["max8"] <= 3, name                          # the shuffled twin never gets there
    assert trace[("ctx_cluster", 0)]["max8"] >= 7
    for name, s, D in (("c8_idle_run", 16, 128), ("c3_idle_run", 11, 4)):
        sy, F = cat[name]["syms"][s], cat[name]["parsed"]["slots"][s]["F"]
        runs = np.diff(np.nonzero(np.concatenate([[1], sy != D, [1]]))[0]) - 1
        assert F[D] >= 1 << 13 and runs.max() > 4096 and trace[(name, s)]["idle8"] >= 100 and trace[(name, s)]["max8"] >= 5, name
    # ---- ring and block edges
    # (lengths of class streams whatever their block: the encoder writes the short ones raw or as one symbol; rANS chains of 2, 3,
    #  15, 16 and 17 symbols exist only in the crafted short_rans tiles, and one symbol is never a chain)
    assert lens >= {1, 2, 3, 15, 16, 17, 511, 512, 513}, sorted(lens)[:40]
    assert 0 in nws and any(0 < v < 32 for v in nws) and any(32 <= v < 64 for v in nws)
    assert any(tr["nw"] > 768 for (nm, s), tr in trace.items() if (cat[nm]["w"], cat[nm]["h"]) == (mc.W, mc.H))
    # ---- splice
    assert types_in_tile["splice_mixed"] == {0, 1, 2, 3, 4}
    assert len(raw_widths["splice_raw_widths"] & {3, 4, 5, 6, 7, 8}) >= 3
    assert {0, 1, 31} <= offs and long_raw, (sorted(offs), long_raw)
    # ---- routing
    assert (cat["route_all_class1"]["syms"][0] == 1).all() and cat["route_all_class1"]["parsed"]["slots"][9]["n"] == mc.NPIX
    assert cat["route_all_class5"]["parsed"]["slots"][13]["n"] == 3 * mc.NPIX
    v = mc.entry("route_alternate")[2]
    assert (np.diff(v[v > 0][:24000]) != 0).all()
    # in TILE pixels (pixel 0 is not coded, vseq[i] is the class of pixel i + 1): pixel p starts a run where its class differs from p - 1's
    vr = np.concatenate([[-1], mc.entry("route_runs_1024")[2]])
    starts = set((np.nonzero(np.diff(vr[1:]))[0] + 2).tolist())
    assert starts == set(mc.ROUTE_CHANGES) and {p % 1024 for p in starts} == {1, 1023} and {p % 4096 for p in starts if p > 3000} == {1, 4095}
    assert cat["route_runs_1024"]["coded"] and cat["route_runs_1024"]["syms"][0][0] == mc.ROUTE_RUNS[0][0]       # pixel 1 opens the first run
    coded = [n for n in NAMES if cat[n]["coded"]]
    assert {cat[n]["w"] % 4 for n in coded} >= {1, 2, 3} and {(cat[n]["w"] * cat[n]["h"]) % 4 for n in coded} >= {1, 2, 3}


def test_flipped_rules_change_a_forecast(cat):
    """One rule of the checker flipped at a time: the last instead of the first of the tied donors, '>' for '>=' at the raw threshold.
    Each changes the forecast of an entry, so the inputs can tell the rules apart.  '<=' for '<' at the table form can change
    nothing, whatever the stream: the equality has no solution (UNREACHABLE)."""
    changed = {flip: [] for flip in mc.FLIPS}
    for name, e in cat.items():
        if not e["coded"]:
            continue
        for s, f in enumerate(e["forecast"]):
            if f["type"] < 2:
                continue
            for flip in mc.FLIPS:
                g = mc.v1_forecast(e["syms"][s], mc.NOMINAL[s], flip=flip)
                if (g["type"], g["length"], g["bits"]) != (f["type"], f["length"], f["bits"]) or not np.array_equal(g["F"], f["F"]):
                    changed[flip].append((name, s))
    print({k: v[:6] for k, v in changed.items()})
    assert any(n.endswith("tie_once") for n, _ in changed["donor_last"]) and len(changed["donor_last"]) >= 4
    assert {n for n, _ in changed["raw_strict"]} == {f"raw_tie_c{c}" for c in range(3, 9)}
    assert changed["form_le"] == [], UNREACHABLE["dense/sparse equality"]


def test_crafted_tiles_are_tables_the_format_allows(po, cat):
    """Every crafted table sums to 2^14 and gives every used symbol a width; the oracle decodes the crafted tile to the raster it
    was made from; and each tile holds what it is named after."""
    got = {}
    for name, (r, tile, src) in mc.crafted().items():
        h, w, _ = r.shape
        assert np.array_equal(po.decode_tiles(2, tile, w, h, 3), r) and tile != cat[src]["tile"], name
        pt, orig = mc.parse_colour_tile(tile), cat[src]["parsed"]
        got[name] = []
        for s in range(17):
            sl = pt["slots"][s]
            syms = mc.slot_symbols(pt, s)
            assert np.array_equal(syms, cat[src]["syms"][s]), (name, s)
            if sl["block"] != orig["slots"][s]["block"] or sl["type"] != orig["slots"][s]["type"]:
                F = sl["F"]
                assert sl["type"] >= 3 and int(F.sum()) == 1 << mc.PB and (F[np.unique(syms)] > 0).all(), (name, s)
                tr = mc.refill_trace(sl["block"], F, sl["n"])
                got[name].append((s, sl, mc.colour_profile(F, s), tr, _hist(syms, mc.NOMINAL[s])))
                print(f"crafted {name} slot {s}: type {sl['type']} n {sl['n']} nw {tr['nw']} words per block max {tr['max8']}, {len(tile)} B")
        assert got[name], name
    for name, slot in (("top_width1_big", 16), ("top_width1_small", 9)):
        (s, sl, cp, tr, hist), = got[name]
        assert s == slot and sl["F"][int(np.argmax(hist))] == 1 and tr["max8"] == 8 and tr["nw"] > 2000, name
    assert [(s, sl["type"]) for s, sl, *_ in got["class1_dense"]] == [(9, 3)]
    assert all(sl["type"] == 3 for _, sl, *_ in got["trailing_zeros"]) and any(cp["top"] < cp["N"] - 1 for _, _, cp, *_ in got["trailing_zeros"])
    (s, sl, cp, tr, hist), = got["width1_bucket"]
    cum = np.concatenate([[0], np.cumsum(sl["F"])])
    assert cum[129] % cp["bucket"] == 0 and (sl["F"][129:161] == 1).all()
    assert {sl["n"] for n in ("short_rans_a", "short_rans_b") for _, sl, *_ in got[n]} >= {2, 3, 15, 16, 17}


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLD, "m2_colour.json")) as f:
        return json.load(f)


def test_generator_and_oracle_agree_with_the_reference_pins(po, cat, pinned):
    """tests/golden/m2_colour.json was written by oracle/make_m2_colour_golden.py from the compiled reference: the generator still
    gives those rasters and the oracle's level-2 file is the reference's."""
    from xpng_amd.synth import to_seven_bytes
    rasters = {n: cat[n]["raster"] for n in NAMES}
    rasters["gray_cluster"] = mc.gray_cluster_raster()
    assert set(pinned) == set(rasters)
    for name, r in rasters.items():
        ent = pinned[name]
        assert r.shape == (ent["h"], ent["w"], 3) and md5(to_seven_bytes(r)) == ent["seven_md5"], name
        data = po.encode_image(2, r)
        assert (len(data), md5(data)) == (ent["L2"]["size"], ent["L2"]["md5"]), name
        if name in cat and cat[name]["coded"]:                                # (a file no smaller than its raster is rewritten at level 7)
            assert data[8:] == cat[name]["tile"] and data[3] == 2, name


def test_gray_cluster_carries_the_unshuffled_stream(po):
    """The clustered gray tile (slot 17, pb 15, the same chain kernel): the left predictor's residuals are the "exhaust" counts with
    the rare symbols in one run, and the decode recurrence takes 7 words or more inside one block of 8 pair steps."""
    g = mc.gray_cluster_raster()
    tile = rt.tile_blobs(po.encode_image(2, g)[8:], 1)[0]
    btype, F = rt.gray_table(tile)
    assert tile[3] == 0x20 and btype == 4
    stream = re_.gray_streams(g[..., 0])[0]
    assert np.array_equal(_hist(stream, 256), _hist(re_.gray_streams(re_.gray_raster("exhaust")[..., 0])[0], 256))
    bsz = int.from_bytes(tile[4:8], "little")
    tr = mc.refill_trace(tile[4 + bsz:], F, len(stream), 15)
    print(f"gray_cluster: nw {tr['nw']}, words per block max {tr['max8']}, idle blocks {tr['idle8']}")
    assert np.array_equal(tr["syms"], stream) and tr["max8"] >= 7


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _explain(got: bytes, want: bytes):
    """where a device tile differs from the oracle's: the first slot whose block or piece of b differs"""
    try:
        a, b = mc.parse_colour_tile(got), mc.parse_colour_tile(want)
    except AssertionError as err:
        return f"the device's tile does not parse: {err}"
    for s in range(17):
        x, y = a["slots"][s], b["slots"][s]
        if (x["type"], x["n"], x["block"], x["bit1"] - x["bit0"]) != (y["type"], y["n"], y["block"], y["bit1"] - y["bit0"]):
            return f"slot {s}: type {x['type']} / {y['type']}, n {x['n']} / {y['n']}, block {len(x['block'])} / {len(y['block'])} B"
        if x["F"] is not None and not np.array_equal(x["F"], y["F"]):
            return f"slot {s}: table differs at {np.nonzero(x['F'] != y['F'])[0][:8].tolist()}"
    return "b differs outside the blocks' pieces" if a["b"] != b["b"] else "header"


def _encode_and_decode(gpu, raster, want, what, encode=True):
    """encode_device(2) == want with nothing written behind it; decode_device(2) of want == raster, status 0, sentinels around it"""
    import torch
    h, w, ch = raster.shape
    ctx = gpu.Context(w, h, ch)
    try:
        if encode:
            d_r = torch.from_numpy(raster.copy()).cuda()
            d_b = torch.full((ctx.blob_bound() + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
            n = ctx.encode_device(2, d_r.data_ptr(), d_b.data_ptr())
            got = d_b.cpu().numpy()
            blob = got[:n].tobytes()
            if blob != want:
                pytest.fail(f"{what}: encode differs from the oracle ({n} / {len(want)} B): "
                            f"{_explain(blob, want) if want[3] >> 4 == 1 and n >= 8 and blob[3] >> 4 == 1 else 'tile kind'}")
            assert (got[n:] == SENTINEL).all(), (what, "bytes behind the blob written")
        d_blob = torch.from_numpy(np.frombuffer(want + b"\0" * 64, dtype=np.uint8).copy()).cuda()
        nbytes = w * h * ch
        buf = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        ctx.decode_device(2, d_blob.data_ptr(), len(want), None, buf.data_ptr() + 64)
        assert ctx.decode_status() == 0, what
        out = buf.cpu().numpy()
        assert np.array_equal(out[64:64 + nbytes].reshape(h, w, ch), raster), (what, "decode")
        assert (out[:64] == SENTINEL).all() and (out[64 + nbytes:] == SENTINEL).all(), (what, "sentinel")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_entry_encodes_and_decodes(gpu, cat, monkeypatch, name, form):
    """encode_device(2) bytes == the oracle's (a difference is reported by slot), decode_device(2) == the raster, status 0, the
    sentinels behind every output untouched; on the narrow and on the forced wide form."""
    monkeypatch.setenv(form, "1")
    _encode_and_decode(gpu, cat[name]["raster"], cat[name]["tile"], (name, form))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gray_cluster_encodes_and_decodes(gpu, po, monkeypatch, form):
    monkeypatch.setenv(form, "1")
    g = mc.gray_cluster_raster()
    _encode_and_decode(gpu, g, po.encode_tiles(2, g), ("gray_cluster", form))


def _batch(gpu, rasters, wants, B, encode_k):
    """One encode_device_batch over the first encode_k (rasters, wants) pairs cycling, one decode_device_batch over all of them
    cycling: blobs == the oracle's with nothing written behind them, pixels == the rasters, status 0, sentinels kept."""
    import torch
    h, w, ch = rasters[0].shape
    k = len(rasters)
    ctx = gpu.Context(w, h, ch, batch=B)
    try:
        assert ctx.n_tiles == 1 and ctx.n_tiles * 17 * B > 2048                # the launch selects the wide kernels by itself
        d_src = [torch.from_numpy(r.copy()).cuda() for r in rasters]
        cap = (ctx.blob_bound() + 64 + 15) & ~15
        d_b = torch.full((B, cap), SENTINEL, dtype=torch.uint8, device="cuda")
        lens = ctx.encode_device_batch(2, [d_src[i % encode_k].data_ptr() for i in range(B)], [d_b[i].data_ptr() for i in range(B)])
        got = d_b.cpu().numpy()
        for i in range(B):
            want = wants[i % encode_k]
            assert lens[i] == len(want) and got[i, :lens[i]].tobytes() == want, (i, "encode")
            assert (got[i, lens[i]:] == SENTINEL).all(), (i, "bytes behind the blob written")
        d_want = [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in wants]
        nbytes = w * h * ch
        d_o = torch.full((B, nbytes + 64), SENTINEL, dtype=torch.uint8, device="cuda")
        ctx.decode_device_batch(2, [d_want[i % k].data_ptr() for i in range(B)], [len(wants[i % k]) for i in range(B)], None,
                                [d_o[i].data_ptr() for i in range(B)])
        assert ctx.decode_status() == 0
        for i in range(B):
            assert torch.equal(d_o[i, :nbytes], d_src[i % k].reshape(-1)), (i, "decode")
        assert bool((d_o[:, nbytes:] == SENTINEL).all())
    finally:
        ctx.close()


@pytest.mark.gpu
def test_batch_of_the_big_entries_selects_the_wide_kernels(gpu, cat):
    """128 single-tile 200 x 150 images cycling through the catalogue: tiles x 17 x images > 2048, so the launch takes the wide
    kernels by itself, and every 32-lane chain wave mixes lengths, empty, one-symbol and raw blocks beside rANS blocks, clustered
    beside shuffled streams; the lanes finish at different blocks."""
    names = _big_names(cat)
    assert 30 <= len(names) <= 128 and any(n.endswith("_cluster") for n in names)
    _batch(gpu, [cat[n]["raster"] for n in names], [cat[n]["tile"] for n in names], 128, len(names))


@pytest.mark.gpu
def test_crafted_tiles_in_a_batch_beside_ordinary_tiles(gpu, cat):
    """The crafted 200 x 150 tiles beside the tiles they were made from and the clustered ones, 128 images in one decode launch (the
    wide kernels by themselves); the encode half of the batch runs over the ordinary rasters."""
    crafted = [(r, tile) for r, tile, src in mc.crafted().values() if r.shape[:2] == (mc.H, mc.W)]
    plain = [n for n in _big_names(cat) if n.endswith("_cluster") or n in {src for _, _, src in mc.crafted().values()}]
    assert len(crafted) == 5 and len(plain) >= 8
    rasters = [cat[n]["raster"] for n in plain] + [r for r, _ in crafted]
    wants = [cat[n]["tile"] for n in plain] + [t for _, t in crafted]
    _batch(gpu, rasters, wants, 128, len(plain))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_crafted_tiles_decode(gpu, monkeypatch, form):
    """decode_device(2) of every crafted tile, and all of them in one MixedContext.decode_batch(2), on both forms."""
    import torch
    monkeypatch.setenv(form, "1")
    items = list(mc.crafted().items())
    for name, (r, tile, _) in items:
        _encode_and_decode(gpu, np.ascontiguousarray(r), tile, (name, form), encode=False)
    rasters = [np.ascontiguousarray(r) for _, (r, _, _) in items]
    ctx = gpu.MixedContext([(r.shape[1], r.shape[0]) for r in rasters], 3)
    try:
        d_b = [torch.from_numpy(np.frombuffer(t + b"\0" * 64, dtype=np.uint8).copy()).cuda() for _, (_, t, _) in items]
        d_o = [torch.full((r.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for r in rasters]
        ctx.decode_batch(2, [t.data_ptr() for t in d_b], [len(t) for _, (_, t, _) in items], [t.data_ptr() for t in d_o])
        assert ctx.decode_status() == 0
        for (name, _), r, t in zip(items, rasters, d_o):
            got = t.cpu().numpy()
            assert np.array_equal(got[: r.size].reshape(r.shape), r) and (got[r.size:] == SENTINEL).all(), (name, form)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_tiny_and_big_entries_in_one_mixed_call(gpu, cat, monkeypatch, form):
    """Every entry smaller than 200 x 150 and eight big ones (clustered, dense, steal-heavy, raw-heavy) in ONE MixedContext call
    per direction: blobs == the oracle's, pixels == the rasters, nothing written around them."""
    import torch
    monkeypatch.setenv(form, "1")
    big = ["c8_exhaust_cluster", "c8_donor_below_dense", "c8_scan31_cluster", "c8_zero_gap", "ctx_cluster", "splice_mixed", "route_runs_1024",
           "route_alternate"]
    names = [n for n in NAMES if cat[n]["w"] * cat[n]["h"] < mc.W * mc.H] + big
    assert len(names) >= 30
    rasters, wants = [cat[n]["raster"] for n in names], [cat[n]["tile"] for n in names]
    ctx = gpu.MixedContext([(r.shape[1], r.shape[0]) for r in rasters], 3)
    try:
        d_b = [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in wants]
        d_o = [torch.full((r.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for r in rasters]
        ctx.decode_batch(2, [t.data_ptr() for t in d_b], [len(b) for b in wants], [t.data_ptr() for t in d_o])
        assert ctx.decode_status() == 0
        for n, r, t in zip(names, rasters, d_o):
            got = t.cpu().numpy()
            assert np.array_equal(got[: r.size].reshape(r.shape), r) and (got[r.size:] == SENTINEL).all(), (n, form, "decode")
        d_r = [torch.from_numpy(r.reshape(-1).copy()).cuda() for r in rasters]
        d_e = [torch.full((ctx.blob_bound(i) + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for i in range(len(names))]
        lens = ctx.encode_batch(2, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_e])
        torch.cuda.synchronize()
        for n, want, t, ln in zip(names, wants, d_e, lens):
            got = t.cpu().numpy()
            assert ln == len(want) and got[:ln].tobytes() == want, (n, form, "encode")
            assert (got[ln:] == SENTINEL).all(), (n, form, "bytes behind the blob written")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c8_exhaust_cluster", "splice_mixed", "len_b"])
def test_files_equal_the_pinned_reference_files(gpu, cat, pinned, monkeypatch, tmp_path, name):
    """store writes the file the compiled reference wrote (size and md5 of tests/golden/m2_colour.json) and load gives the raster
    back, on both forms."""
    path = str(tmp_path / "f.xpng")
    for form in FORMS:
        with monkeypatch.context() as m:
            m.setenv(form, "1")
            gpu.store(2, cat[name]["raster"], path)
            data = open(path, "rb").read()
            assert (len(data), md5(data)) == (pinned[name]["L2"]["size"], pinned[name]["L2"]["md5"]), (name, form, "store")
            assert np.array_equal(gpu.load(path), cat[name]["raster"]), (name, form, "load")
