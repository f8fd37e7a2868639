"""CPU half of the rANS symbol-lookup tests: the oracle's table-given v2 encoder, the table tools of tests/_rans_tables.py,
and the validity of the crafted files the GPU tests decode (the oracle decodes them, and so does the genuine reference
when oracle/_ref is built)."""
import tempfile

import numpy as np
import pytest

import _rans_tables as rt
from _kit import po


def catalogue(pb):
    """Hand-made normalised tables: name -> F (len(F) = N as written)."""
    T = 1 << pb
    cat = {
        "two": [T - 7, 7],
        "tied": [T // 2 - 100, T // 2 - 100, 50, 0, 150],
        "hot_first": [T - 255] + [1] * 255,
        "hot_last": [1] * 255 + [T - 255],
        "holes": [0] * 256,
        "flat": [T // 256] * 256,
        "skew9": [1] * 4 + [T - 8] + [1] * 4,
        "trailing": [T // 16] * 8 + [T // 2] + [0] * 31,
        "lone": [T - 1, 0],
        "dense_bucket": [T // 3, T // 3 - 200] + [1] * 200 + [T - 2 * (T // 3) + 200 - 200],
    }
    h = cat["holes"]
    for s in range(0, 256, 7):
        h[s] = 1
    h[252] += T - sum(h)
    for name, F in cat.items():
        assert sum(F) == T - (name == "lone") and min(F) >= 0 and max(F) < T, (name, pb)
    return cat


@pytest.mark.parametrize("pb", [10, 11, 12, 13, 14, 15])
def test_rans2_encode_table_round_trips_every_catalogue_shape(po, pb):
    rng = np.random.default_rng(pb)
    for name, F in catalogue(pb).items():
        F = np.array(F, dtype=np.uint32)
        for n in (1, 2, 5001):
            syms = rng.choice(len(F), size=n, p=F / F.sum()).astype(np.uint8)
            for sparse in (False, True):
                blk = po.rans2_encode_table(F, syms, pb, sparse)
                t, bn, bpb, got = rt.parse_v2_block(blk)
                assert (t, bn, bpb) == (4 if sparse else 3, n, pb) and np.array_equal(got, F), (name, n, sparse)
                back, csz = po.rans2_decode(blk, n)
                assert csz == len(blk) and np.array_equal(back, syms), (name, pb, n, sparse)
    with pytest.raises(ValueError):   # a symbol without a slot
        po.rans2_encode_table(np.array([1 << pb, 0], np.uint32) - 1, np.array([1], np.uint8), pb, False)


def test_lookup_profile_known_answers():
    p = rt.lookup_profile(10, [512, 512])                       # tie: the higher index is hot0
    assert (p["hot0"], p["hot1"], p["cold"], p["rsh"], p["route"]) == (1, 0, 0, 0, "exact")
    p = rt.lookup_profile(15, [(1 << 15) - 255] + [1] * 255)    # hot at index 0; F = 1 ties -> hot1 = 255
    assert (p["hot0"], p["hot1"], p["cold"], p["rsh"], p["max_bound"]) == (0, 255, 254, 0, 0)
    p = rt.lookup_profile(15, [1] * 255 + [(1 << 15) - 255])    # hot at index 255
    assert (p["hot0"], p["hot1"], p["cold"], p["route"]) == (255, 254, 254, "exact")
    # pb 12: hot 5 (3000) and 9 (400) with zero holes at 6, 7: cold 696 -> rsh 1; ranks 4, 5 are slots 4 and 3005 (symbols 4
    # and 8): count8 steps over 5, 6, 7 and 8 -> 4 boundaries, and that bucket straddles hot0's range
    F = [1, 1, 1, 1, 1, 3000, 0, 0, 1, 400, 390, 300]
    p = rt.lookup_profile(12, F)
    assert (p["hot0"], p["hot1"], p["cold"], p["rsh"], p["max_bound"], p["route"], p["straddles"]) == (5, 9, 696, 1, 4, "round1", 1)
    p = rt.lookup_profile(15, [(1 << 15) - 1, 0])                # one used symbol
    assert p["single"] and p["hot0"] == p["hot1"] == 0 and p["cold"] == 1 and p["route"] == "exact"
    # 17 zero entries between two F = 1 symbols inside one 2-rank bucket: the scan
    F = [8000, 7684, 1] + [0] * 17 + [1, 698]
    p = rt.lookup_profile(14, F)
    assert (p["cold"], p["rsh"], p["max_bound"], p["route"]) == (700, 1, 18, "scan")
    # context layouts
    assert rt.lookup_profile(12, [100] * 8 + [(1 << 12) - 800], alpha=False)["layout"] == "small"
    assert rt.lookup_profile(13, [100] * 8 + [(1 << 13) - 800], alpha=False)["layout"] == "rest"
    assert rt.lookup_profile(10, [100] * 9 + [(1 << 10) - 900], alpha=False)["layout"] == "rest"
    assert rt.gray_profile([1] * 40 + [(1 << 15) - 40] + [0] * 215)["max_bound"] == 40


def _ref_decodes(po, data, raster):
    from xpng_amd.synth import to_seven_bytes
    if not po.have_ref():
        return
    with tempfile.TemporaryDirectory() as td:
        seven, _ = po.ref_decode(data, td)
    assert seven == to_seven_bytes(raster)


def test_crafted_files_are_valid_input(po):
    """Every crafted mode-1 file decodes to its raster through the oracle and through the genuine reference; together the
    re-coded blocks reach every context layout at pb 10..12, both alpha table shapes at pb 10..14 in dense and sparse form,
    and the one-symbol alpha table."""
    seen = set()
    for name, raster, blobs, prof in rt.craft_m1_variants():
        H, W, ch = raster.shape
        assert np.array_equal(po.decode_tiles(1, blobs, W, H, ch), raster), name
        _ref_decodes(po, rt.file_header(W, H, 1, True) + blobs, raster)
        for p in prof:
            seen.add((p["layout"], p["pb"], p["route"] if p["layout"] == "alpha" else p["N"] > 9, p["single"]))
    for pb in (10, 11, 12):
        assert ("small", pb, False, False) in seen and ("rest", pb, True, False) in seen, pb
    for pb in (10, 11, 12, 13, 14):
        assert any(s[0] == "alpha" and s[1] == pb and s[2] != "exact" for s in seen), pb
    assert {s[2] for s in seen if s[0] == "alpha" and s[1] < 15} >= {"round1", "round2", "scan"}
    assert ("alpha", 15, "exact", True) in seen


def test_alpha_shape_rasters_reach_their_routes(po):
    """The reference-writable alpha shapes of the GPU tests: the table the encoder writes takes the named route (and the
    genuine reference writes the same file)."""
    from xpng_amd.synth import to_seven_bytes
    for name in rt.ALPHA_SHAPES:
        raster = rt.shape_raster(name)
        data = po.encode_image(1, raster)
        (pb, F), = rt.alpha_block_tables(data[8:], rt.SHAPE_W, rt.SHAPE_H)
        assert np.array_equal(F[:256], [rt.ALPHA_SHAPES[name].get(s, 0) for s in range(len(F))]), name
        p = rt.lookup_profile(pb, F)
        assert p["route"] == rt.ALPHA_ROUTES[name], (name, p)
        if po.have_ref():
            with tempfile.TemporaryDirectory() as td:
                assert po.ref_encode(1, to_seven_bytes(raster), td)[0] == data, name
    raster = rt.scan_recipe_raster()
    profs = [rt.lookup_profile(pb, F) for pb, F in rt.alpha_block_tables(po.encode_image(1, raster)[8:], 888, 444)]
    assert len(profs) == 2 and any(p["rsh"] >= 5 and p["max_bound"] >= 17 for p in profs)


def test_gray_table_parser_and_scan_raster(po):
    raster = rt.gray_scan_raster()
    H, W, _ = raster.shape
    data = po.encode_image(2, raster)
    tabs = [rt.gray_table(t) for t in rt.tile_blobs(data[8:], len(po.tile_table(W, H, 3)))]
    assert len(tabs) == 1 and tabs[0] is not None
    btype, F = tabs[0]
    assert btype in (3, 4) and F.sum() == 1 << 15
    assert rt.gray_profile(F)["max_bound"] > 16
    assert np.array_equal(po.decode_image(data), raster)
    _ref_decodes(po, data, raster)
