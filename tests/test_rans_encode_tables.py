"""The tables of the rANS ENCODERS on inputs that reach the steal repair, both table forms and the raw fallback.

Every encoder builds its block with rans_histogram / rans_alphabet / rans_tables (xpng_amd/csrc/rans2.hpp): the narrow level-1
wave (rans2_encode_block), the wide level-1 trio (k_rans2_prep / chain2 / finish), the narrow level-2 wave (k_rans1_encode) and the
wide level-2 form (k_rans1_prep / chain / finish).  tests/_rans_encode.py restates the reference's normalisation rule and the
choice of the block type on Python integers, and builds the inputs: an alpha catalogue (pb 15, alphabet 256), a family of RGB
rasters whose context streams reach the repair (pb 12, alphabet 9), and gray level-2 tiles that carry catalogue streams (pb 15).

CPU part: the checker is pinned to the oracle - table, type and length of every block - and every input is shown to reach the
branch it is named after (the census; run with -s to read it).  GPU part (-m gpu): bytes against the oracle, per block
(Context.fetch serves the blocks of the narrow and of the wide form: both write them to the same place), per file, in one batch
that selects the wide kernels by itself, in one mixed-size call, and at level 2.  The level-2 colour streams (pb 14) are compared
as bytes only here; tests/test_m2_colour_streams.py parses the level-2 colour blocks and holds the census of their steals."""
import numpy as np
import pytest

import _rans_encode as re_
import _rans_tables as rt

from _kit import gpu, po, SENTINEL

FORMS = ["XPNG_NARROW_RANS", "XPNG_WIDE_RANS"]
CTX_IDS = ["amp%d-k%d-mag%d-seed%d" % p for p in re_.CTX_PARAMS]


def _hist(syms, N=256):
    return np.bincount(syms, minlength=N)[:N]


@pytest.fixture(scope="module")
def alpha(po):
    """name -> raster, alpha stream, the oracle's alpha block, level-1 file and tile blobs, the forecast: computed once"""
    out = {}
    for name, (raster, syms) in re_.alpha_catalogue().items():
        out[name] = dict(raster=raster, syms=syms, block=po.rans2_encode(_hist(syms), 256, syms, 15), file=po.encode_image(1, raster),
                         blobs=po.encode_tiles(1, raster), forecast=re_.block_forecast(syms, 256, 15))
    assert list(out) == re_.ALPHA_NAMES
    return out


@pytest.fixture(scope="module")
def context(po):
    """per entry of CTX_PARAMS: raster, [(tile, stream, the oracle's block, forecast)], the oracle's level-1 and level-2 files"""
    out = []
    for prm in re_.CTX_PARAMS:
        raster = re_.ctx_raster(*prm)
        streams = [(ti, c, po.rans2_encode(F, 9, syms, 12), re_.block_forecast(syms, 9, 12)) for ti, c, F, syms in re_.ctx_streams(raster)]
        out.append(dict(raster=raster, streams=streams, file1=po.encode_image(1, raster), file2=po.encode_image(2, raster)))
    return out


@pytest.fixture(scope="module")
def gray(po):
    out = {}
    for name in re_.GRAY_NAMES:
        raster = re_.gray_raster(name)
        out[name] = dict(raster=raster, file=po.encode_image(2, raster))
    return out


def _check_block(blk, f, what):
    """a block of the oracle's against the forecast: type, length, and the table it wrote against the profile's"""
    t, n, pb, F = rt.parse_v2_block(blk)
    assert (t, len(blk)) == (f["type"], f["length"]), (what, t, len(blk), f["type"], f["length"])
    if t >= 3:
        assert F.tolist() == f["profile"]["F"], what


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_profile_census_of_the_alpha_shapes(alpha):
    """The steals of every counted shape, from the histogram alone; the five measured shapes give the issue's exact numbers."""
    for name, c in list(re_.BIG_COUNTS.items()) + list(re_.FORM_COUNTS.items()):
        hist = np.zeros(256, np.int64)
        hist[list(c)] = list(c.values())
        assert np.array_equal(hist, _hist(alpha[name]["syms"])), name
        p, f = re_.normalise_profile(hist, 15), alpha[name]["forecast"]
        print(f"{name}: steals {len(p['steals'])} (below {p['below']}, above {p['above']}), donors {p['donors']}, to width 1 "
              f"{p['to_one']}, among ties {p['tied']}; N {p['N']}, in use {f['distinct']}, type {f['type']}, rANS {f['cand']} B, raw {f['raw']} B")
        if name in re_.EXPECT:
            steals, below, above, donors, to_one, tied, btype = re_.EXPECT[name]
            assert len(p["steals"]) == steals and f["type"] == btype, name
            for got, want in ((p["below"], below), (p["above"], above), (p["donors"], donors), (p["to_one"], to_one)):
                assert want is None or got == want, (name, got, want)
            assert p["tied"] >= tied, name
        for i, donor, width, ties in p["steals"]:
            assert donor != i and width >= 2 and ties >= 1
    x = {n: re_.normalise_profile(_hist(alpha[n]["syms"]), 15) for n in re_.BIG_COUNTS}
    assert x["donor_below"]["above"] == 0 and x["donor_above"]["below"] == 0
    assert x["exhaust"]["tied"] == 2 and x["all_once"]["below"] == 183
    assert x["dominant"]["F"] == [32767, 1] and x["dominant"]["steals"] == []
    assert x["dominant_steal"]["F"] == [1, 32767] and x["dominant_steal"]["steals"] == [(0, 1, 32768, 1)]
    t = x["tie_once"]                                          # the first of the two tied donors gave: 10, below the taker
    assert t["steals"] == [(100, 10, 3, 2)] and (t["F"][10], t["F"][100], t["F"][200]) == (2, 1, 3)
    F = x["pow2"]["F"]                                         # the reciprocal's shift is 32 - clz(F - 1): F = 2^k and F = 2^k + 1 differ
    assert 4096 in F and 1025 in F
    assert any(v >= 4 and v & (v - 1) == 0 for v in F) and any(v >= 5 and (v - 1) & (v - 2) == 0 for v in F)


def test_alpha_catalogue_blocks_follow_the_forecast(po, alpha):
    """Every catalogue raster is one coded level-1 tile whose alpha stream is the crafted one; the oracle's alpha block has the
    forecast's type and length and the profile's table, and it is the block inside the oracle's file."""
    tails = set()
    for name, a in alpha.items():
        raster, syms, f = a["raster"], a["syms"], a["forecast"]
        H, W, _ = raster.shape
        tiles = po.tile_table(W, H, 4)
        assert len(tiles) == 1 and len(syms) == W * H - 1, name
        pr, _ = po.choose_predictor(raster, tiles[0])
        planes = po.m1_planes(raster, tiles[0], pr)
        assert np.array_equal(planes["a"][1:], syms), name
        assert np.array_equal(po.m1_streams(raster, tiles[0], planes)["FA"], _hist(syms)), name
        _check_block(a["block"], f, name)
        assert a["file"][3] == 1 and a["file"][8:] == a["blobs"], (name, "stored at level 1")
        tile = rt.tile_blobs(a["blobs"], 1)[0]
        assert tile[3] != 0 and rt.m1_blocks(tile, 4)[1][9] == a["block"], (name, "the tile is coded and holds the block")
        assert np.array_equal(po.normalize_rgba(raster), raster), name
        print(f"{name}: {W} x {H}, n {len(syms)}, type {f['type']}, rANS {f['cand']} B, raw {f['raw']} B")
        if name.startswith("raw_bits"):
            b = int(name[8])
            assert f["type"] == 2 and f["profile"]["N"] == 1 << b, name
            tails.add(b * len(syms) % 32)
    assert len(po.tile_table(re_.BIG_W, re_.BIG_H, 4)) == 1
    assert re_.RAW_BITS_TAILS <= tails and {b for b, _, _ in re_.RAW_BITS} == {1, 2, 3, 5, 6, 7}
    assert [w * h for b, w, h in re_.RAW_BITS if b in (3, 7)].count(re_.BIG_W * re_.BIG_H) == 2
    tie, sparse = alpha["form_tie"]["forecast"], alpha["form_sparse"]["forecast"]
    assert (tie["profile"]["N"], tie["distinct"], tie["type"]) == (15, 14, 3) and 15 + 14 * 15 == 15 * 15
    assert (sparse["profile"]["N"], sparse["distinct"], sparse["type"]) == (15, 13, 4)
    for kind, diff in re_.SHORT_KINDS.items():
        f = alpha[kind]["forecast"]
        assert f["cand"] - f["raw"] == diff and f["type"] == (2 if diff >= 0 else 3 + f["sparse"]), kind
        assert 20 <= len(alpha[kind]["syms"]) <= 600


def test_short_stream_search_finds_the_committed_picks(po):
    """The seeded search behind SHORT_PICKS, and the forecast against the oracle's own choice on each of its streams."""
    found = re_.search_short_streams()
    print("short streams:", found)
    assert {k: v[:3] for k, v in found.items()} == re_.SHORT_PICKS
    types = set()
    for t in range(400):
        w, h, syms = re_.short_stream(t)
        f = re_.block_forecast(syms, 256, 15)
        _check_block(po.rans2_encode(_hist(syms), 256, syms, 15), f, t)
        types.add(f["type"])
    assert types >= {2, 3, 4}


def test_context_rasters_reach_the_repair(po, context):
    """Every context block of the family has the forecast's type, length and table; over the committed parameter list the steal
    repair of a context block takes a slot from below and from above, both in one block, chooses among tied donors, and does so
    under both table forms."""
    total = []
    for prm, cx in zip(re_.CTX_PARAMS, context):
        profs = []
        for ti, c, blk, f in cx["streams"]:
            _check_block(blk, f, (prm, ti, c))
            if f["type"] >= 2:
                assert f["profile"]["N"] <= 9
                profs.append((f["profile"], f["type"]))
        assert cx["file1"][3] == 1 and cx["file2"][3] == 2 and len(cx["file1"]) < cx["raster"].size, prm
        census = re_.ctx_census(profs)
        print(prm, census, "steals", sum(len(p["steals"]) for p, _ in profs))
        total += profs
    census = re_.ctx_census(total)
    assert all(census.values()), census
    own = [re_.ctx_census([(f["profile"], f["type"]) for _, _, _, f in cx["streams"] if f["type"] >= 2]) for cx in context]
    assert own[0]["below_sparse"] and own[1]["below_dense"] and own[2]["above_sparse"] and own[3]["above_dense"]
    assert own[4]["both_in_one"] and own[5]["tied"]


def test_gray_rasters_carry_the_catalogue_streams(po, gray):
    """The level-2 gray tile of a catalogue plane: the table the oracle wrote is the profile's table of the residual stream it
    selected (the left predictor's: the crafted stream), and that profile shows the catalogue's steals."""
    assert len(po.tile_table(re_.BIG_W, re_.BIG_H, 3)) == 1
    for name, g in gray.items():
        tile = rt.tile_blobs(g["file"][8:], 1)[0]
        assert g["file"][3] == 2 and rt.gray_table(tile) is not None, name
        btype, F = rt.gray_table(tile)
        m = tile[3] & 3
        stream = re_.gray_streams(g["raster"][..., 0])[m]
        p = re_.normalise_profile(_hist(stream), 15)
        assert F[:p["N"]].tolist() == p["F"] and not F[p["N"]:].any(), name
        print(f"gray {name}: predictor {m}, type {btype}, steals {len(p['steals'])} (below {p['below']}, above {p['above']}), among ties {p['tied']}")
        assert m == 0 and len(p["steals"]) == re_.EXPECT[name][0] and btype == re_.EXPECT[name][6], name


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _encode_one(gpu, raster):
    """a level-1 encode of one raster on a context of its own -> (context, blob bytes); nothing written behind the blob"""
    import torch
    H, W, ch = raster.shape
    ctx = gpu.Context(W, H, ch)
    d_r = torch.from_numpy(raster).cuda()
    d_b = torch.full((ctx.blob_bound() + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    n = ctx.encode_device(1, d_r.data_ptr(), d_b.data_ptr())
    got = d_b.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    return ctx, got[:n].tobytes()


def _store_and_load(gpu, monkeypatch, tmp_path, level, raster, want, what):
    path = str(tmp_path / "f.xpng")
    for form in FORMS:
        with monkeypatch.context() as m:
            m.setenv(form, "1")
            gpu.store(level, raster, path)
            assert open(path, "rb").read() == want, (what, form, "store")
            assert np.array_equal(gpu.load(path), raster), (what, form, "load")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", re_.ALPHA_NAMES)
def test_alpha_block_equals_the_oracle(gpu, alpha, monkeypatch, name, form):
    """The alpha block as the encoder left it (fetch 29) and the tile blob, on the narrow and on the forced wide form."""
    monkeypatch.setenv(form, "1")
    a = alpha[name]
    ctx, blob = _encode_one(gpu, a["raster"])
    try:
        blk = ctx.fetch(29, 0).tobytes()
        assert (blk[3], len(blk)) == (a["forecast"]["type"], a["forecast"]["length"]), (name, form, blk[3], len(blk))
        assert blk == a["block"], (name, form)
        assert blob == a["blobs"], (name, form)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", re_.ALPHA_NAMES)
def test_alpha_file_equals_the_oracle(gpu, alpha, monkeypatch, tmp_path, name):
    """store == the oracle's file and load == the raster (it is its own normalised form), on both forms."""
    _store_and_load(gpu, monkeypatch, tmp_path, 1, alpha[name]["raster"], alpha[name]["file"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", range(len(re_.CTX_PARAMS)), ids=CTX_IDS)
def test_context_blocks_equal_the_oracle(gpu, context, monkeypatch, k, form):
    """Every context block of every tile (fetch 20 + c) and the tile blobs, on both forms."""
    monkeypatch.setenv(form, "1")
    cx = context[k]
    ctx, blob = _encode_one(gpu, cx["raster"])
    try:
        for ti, c, want, f in cx["streams"]:
            blk = ctx.fetch(20 + c, ti).tobytes()
            assert blk == want, (re_.CTX_PARAMS[k], form, ti, c, f["type"], len(blk), len(want))
        assert blob == cx["file1"][8:], (re_.CTX_PARAMS[k], form)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("k", range(len(re_.CTX_PARAMS)), ids=CTX_IDS)
def test_context_files_equal_the_oracle(gpu, context, monkeypatch, tmp_path, k, level):
    """Level 1 (pb 12) and level 2 (colour tiles, pb 14): store == the oracle's file, load == the raster, on both forms."""
    _store_and_load(gpu, monkeypatch, tmp_path, level, context[k]["raster"], context[k]["file%d" % level], (re_.CTX_PARAMS[k], level))


@pytest.mark.gpu
@pytest.mark.parametrize("name", re_.GRAY_NAMES)
def test_gray_level2_file_equals_the_oracle(gpu, gray, monkeypatch, tmp_path, name):
    """A level-2 gray tile whose pb-15 table needs dozens of steals: store == the oracle's file, round trip, on both forms."""
    _store_and_load(gpu, monkeypatch, tmp_path, 2, gray[name]["raster"], gray[name]["file"], name)


@pytest.mark.gpu
def test_big_shapes_share_one_natural_wide_launch(gpu, alpha):
    """208 single-tile 400 x 300 images, the eleven big shapes in turn: the batch selects the wide kernels by itself and every alpha
    chain wavefront mixes steal-heavy, dense, sparse and raw streams.  Every blob == the oracle's, nothing written behind it."""
    import torch
    names, B = re_.BIG_NAMES, 208
    assert len(names) == 11 and {alpha[n]["forecast"]["type"] for n in names} == {2, 3, 4}
    ctx = gpu.Context(re_.BIG_W, re_.BIG_H, 4, batch=B)
    try:
        assert ctx.n_tiles == 1 and ctx.n_tiles * 10 * B > 2048
        d_r = [torch.from_numpy(alpha[n]["raster"]).cuda() for n in names]
        cap = (ctx.blob_bound() + 64 + 15) & ~15
        d_b = torch.full((B, cap), SENTINEL, dtype=torch.uint8, device="cuda")
        lens = ctx.encode_device_batch(1, [d_r[i % len(names)].data_ptr() for i in range(B)], [d_b[i].data_ptr() for i in range(B)])
        got = d_b.cpu().numpy()
        for i in range(B):
            want = alpha[names[i % len(names)]]["blobs"]
            assert lens[i] == len(want) and got[i, :lens[i]].tobytes() == want, (i, names[i % len(names)])
            assert (got[i, lens[i]:] == SENTINEL).all(), (i, "bytes behind the blob written")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_small_and_big_shapes_in_one_mixed_call(gpu, alpha, monkeypatch, form):
    """Every raster smaller than 400 x 300 (table forms, raw widths, the raw / rANS threshold) and two big shapes in ONE mixed-size
    encode: every blob == the oracle's, nothing written behind it."""
    import torch
    monkeypatch.setenv(form, "1")
    names = [n for n in re_.ALPHA_NAMES if n not in re_.BIG_NAMES] + ["exhaust", "all_once"]
    assert len(names) == len(re_.ALPHA_NAMES) - len(re_.BIG_NAMES) + 2
    rasters = [alpha[n]["raster"] for n in names]
    ctx = gpu.MixedContext([(r.shape[1], r.shape[0]) for r in rasters], 4)
    try:
        d_r = [torch.from_numpy(r.reshape(-1)).cuda() for r in rasters]
        d_b = [torch.full((ctx.blob_bound(i) + 256,), SENTINEL, dtype=torch.uint8, device="cuda") for i in range(len(names))]
        lens = ctx.encode_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
        torch.cuda.synchronize()
        for name, t, n in zip(names, d_b, lens):
            got = t.cpu().numpy()
            assert got[:n].tobytes() == alpha[name]["blobs"], (name, form)
            assert (got[n:] == SENTINEL).all(), (name, form, "bytes behind the blob written")
    finally:
        ctx.close()
