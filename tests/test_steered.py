"""Every predictor and tile kind on every kernel form: steered rasters (tests/_steered.py) against the oracle.

The CPU part (not marked gpu) is a census: it walks the oracle's tile blobs and proves that the steered set reaches every branch of
the format the encoder can write, and pins the rasters to the compiled reference through tests/golden/steered.json
(oracle/make_steered_golden.py).  The GPU part runs the same rasters through the device entry points, bit-exact against the
oracle.  No timing and no tolerance anywhere: every comparison is on bytes."""
import json
import os

import numpy as np
import pytest

import _steered as S
from _kit import gpu, md5, po
from conftest import GOLD


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLD, "steered.json")) as f:
        return json.load(f)


def _u32(b, o):
    return int.from_bytes(b[o:o + 4], "little")


def census(raster, level):
    """The set of format branches the oracle takes on `raster` at `level` (tile headers: encode_tile_m1 / encode_tile_m2 /
    encode_tile_gray in oracle/xpng_oracle.c).  Members:
      ("l1", "raw") / ("l2", "raw") / ("l2", "one_colour")     tiles that are not coded
      ("l1_pr", channels, p)         level-1 tile with predictor p          ("l2_pr", p)    level-2 colour tile
      ("l1_ctx", type)               a level-1 context block of that type   ("l1_alpha", type)   the alpha block
      ("gray", mode byte)            a gray tile                            ("gray_blk", type)   its block
      ("l2_ctx", type)               one of the 9 level-2 context blocks    ("l2_cls", class, type)   one of the 8 class blocks"""
    from oracle import pyoracle as po
    h, w, ch = raster.shape
    blobs = po.encode_tiles(level, raster)
    out, o = set(), 0
    for _ in po.tile_table(w, h, ch):
        h0 = _u32(blobs, o)
        typ, size = h0 >> 24, h0 & 0xFFFFFF
        if typ == 0:
            out.add((f"l{level}", "raw"))
        elif typ == 255:
            out.add(("l2", "one_colour"))
        elif level == 1:
            assert typ >> 4 == 1 and ((typ >> 2) & 1) == (ch == 4)
            out.add(("l1_pr", ch, typ & 3))
            p = o + 4
            p += _u32(blobs, p)                       # the k words
            for c in range(9 + (ch == 4)):
                hdr = _u32(blobs, p)
                out.add(("l1_ctx" if c < 9 else "l1_alpha", hdr >> 24))
                p += hdr & 0xFFFFFF
            assert p == o + size
        elif typ >> 4 == 2:
            out.add(("gray", typ))
            if typ != 0x28:
                p = o + 4 + _u32(blobs, o + 4)        # behind the bit stream
                hdr = _u32(blobs, p)
                out.add(("gray_blk", hdr >> 24))
                assert p + (hdr & 0xFFFFFF) == o + size
        else:
            assert typ >> 4 == 1
            out.add(("l2_pr", typ & 3))
            p = o + 4 + _u32(blobs, o + 4)
            for slot in range(17):
                hdr = _u32(blobs, p)
                out.add(("l2_ctx", hdr >> 24) if slot < 9 else ("l2_cls", slot - 8, hdr >> 24))
                p += hdr & 0xFFFFFF
            assert p == o + size
        o += size
    assert o == len(blobs)
    return out


# Branches of the format that no input can make the encoder write, each with its reason.  The census asserts that they stay unseen.
UNREACHABLE = {
    ("gray_blk", 2): "a raw gray block puts 8 bits per pixel into the bit stream, so that candidate is never smaller than the "
                     "tile's pixel count and the raw gray tile 0x28 is written instead (libxpng.c:606-612)",
    ("l2_cls", 1, 3): "class 1 holds pixels of bit width 1, so symbol 0 never occurs: at most 7 of 8 table entries are non-zero and "
                      "the sparse table (1 + 7 * 15 = 106 bits) always beats the dense one (8 * 14 = 112 bits)",
    ("l2_cls", 2, 3): "class 2 holds pixels of bit width 2, so the 8 symbols with every field below 2 never occur: at most 56 of 64 "
                      "entries are non-zero and the sparse table (8 + 56 * 15 = 848 bits) always beats the dense one (896 bits)",
}


@pytest.fixture(scope="module")
def survey(po):
    """name -> (census at level 1, census at level 2 or None for RGBA); every raster round-trips through the oracle on the way."""
    out = {}
    for name in S.named():
        r = S.raster(name)
        h, w, ch = r.shape
        assert S.tile_table(w, h) == [tuple(int(v) for v in t) for t in po.tile_table(w, h, ch)], name
        for level in (1, 2) if ch == 3 else (1,):
            assert np.array_equal(po.decode_tiles(level, po.encode_tiles(level, r), w, h, ch), r), (name, level)
        out[name] = (census(r, 1), census(r, 2) if ch == 3 else None)
    return out


def test_generator_and_oracle_agree_with_the_reference_pins(po, pinned):
    """tests/golden/steered.json was written by oracle/make_steered_golden.py from the compiled reference: the generator still
    gives those rasters, and the oracle's encode_image still gives the reference's files at levels 1 and 2."""
    from xpng_amd.synth import to_seven_bytes
    assert set(pinned) == set(S.named())
    for name, ent in pinned.items():
        r = S.raster(name)
        assert r.shape == (ent["h"], ent["w"], ent["ch"]) and md5(to_seven_bytes(r)) == ent["seven_md5"], name
        if ent["ch"] == 4:
            assert np.array_equal(po.normalize_rgba(r), r), name          # stays RGBA, no hidden colour to zero
        for level in (1, 2):
            data = po.encode_image(level, r)
            assert (len(data), md5(data)) == (ent[f"L{level}"]["size"], ent[f"L{level}"]["md5"]), (name, level)


def test_chooser_returns_the_wanted_predictor_on_every_tile(po):
    ties = {"all": lambda s: s[0] == s[1] == s[2] == s[3], "avg": lambda s: s[0] == s[1] < min(s[2], s[3]),
            "grad": lambda s: s[2] == s[3] < min(s[0], s[1]), "green": lambda s: s[1] == s[3] < s[0] == s[2]}
    for name, (_, meta) in S.named().items():
        if "pr" not in meta:
            continue
        r = S.raster(name)
        h, w, ch = r.shape
        for t in po.tile_table(w, h, ch):
            pr, sums = po.choose_predictor(r, t)
            assert pr & 3 == meta["pr"], (name, t, sums)
            if "tie" in meta:
                assert ties[meta["tie"]](sums), (name, t, sums)
            else:
                assert all(sums[meta["pr"]] < sums[k] for k in range(4) if k != meta["pr"]), (name, t, sums)


def test_free_pixels_hold_every_edge_neighbourhood(po):
    """Every (L, U, UL) drawn from {0, 1, 2, 127, 128, 129, 253, 254, 255} stands in front of a coded interior pixel, in every
    channel, of every steered colour raster (the 64 x 64 ones have fewer free triples than the 729 combinations and carry a
    share of them); RGBA: a transparent run leaves a row's end and enters column 0 of the next row in some tile."""
    for name, (_, meta) in S.named().items():
        if not name.startswith("pr"):
            continue
        r = S.raster(name)
        h, w, ch = r.shape
        found = S.edge_combinations(r)
        for c in range(3):
            assert len(found[c]) >= (729 if (w, h) != (64, 64) else 90), (name, c, len(found[c]))
        if ch == 4:
            wraps = 0
            for (tx, ty, tw, th) in S.tile_table(w, h):
                a = r[ty:ty + th, tx:tx + tw, 3]
                wraps += int(((a[:-1, -1] == 0) & (a[1:, 0] == 0)).sum())
                assert (a[3::4, 3::4][: th // 4, : tw // 4] >= 1).all(), name        # no sampled pixel is skipped
            assert wraps >= 1, name
            assert (r[r[..., 3] == 0] == 0).all() and (r[..., 3] == 0).any() and (r[..., 3] == 255).any(), name


def test_gray_rasters_take_their_mode_and_ties_are_exact(survey):
    for name, (_, meta) in S.named().items():
        if "gray" not in meta:
            continue
        modes = {b[1] for b in survey[name][1] if b[0] == "gray"}
        assert modes == {meta["gray"]}, (name, modes)
        if meta["kind"] in S.GRAY_TIES:
            cand = S.gray_candidates(S.raster(name))
            tied = S.GRAY_TIES[meta["kind"]]
            for m in tied[1:]:
                assert np.array_equal(cand[tied[0]], cand[m]), (name, m)       # the same stream: the same size, whatever the coder
            assert all(not np.array_equal(cand[tied[0]], cand[m]) for m in range(4) if m not in tied)
            assert meta["gray"] == 0x20 + tied[0]                                # the first of the tied candidates wins
        if meta["kind"] == "one":
            assert ("gray_blk", 1) in survey[name][1]
    both = survey["mixed_gray_1000x900"][1]
    assert {("gray", 0x20), ("gray", 0x23), ("l2", "one_colour"), ("l2_pr", 3)} <= both


def test_census_reaches_every_branch_the_encoder_can_write(survey):
    """The acceptance census: the union of the branches over the steered set."""
    union = set()
    for name, (c1, c2) in survey.items():
        meta = S.named()[name][1]
        if "pr" in meta or meta.get("coded"):                                  # meant to be coded: never a raw tile
            assert ("l1", "raw") not in c1 and (c2 is None or ("l2", "raw") not in c2), name
        if "pr" in meta:                                                       # every tile with the wanted predictor, both levels
            assert {b[2] for b in c1 if b[0] == "l1_pr"} == {meta["pr"]}, name
            assert c2 is None or {b[1] for b in c2 if b[0] == "l2_pr"} == {meta["pr"]}, name
        union |= c1 | (c2 or set())
    print("census:", sorted(union, key=str))
    want = {("l1_pr", ch, p) for ch in (3, 4) for p in range(4)} | {("l2_pr", p) for p in range(4)}
    want |= {("gray", m) for m in (0x20, 0x21, 0x22, 0x23, 0x28)} | {("gray_blk", t) for t in (1, 3, 4)}
    want |= {("l1_alpha", t) for t in (1, 2, 3, 4)} | {("l1_ctx", t) for t in range(5)} | {("l2_ctx", t) for t in range(5)}
    missing = want - union
    assert not missing, missing
    for t in range(5):                                                         # every class-block type, on some class
        assert any(("l2_cls", c, t) in union for c in range(1, 9)), t
    dense = {c for c in range(1, 9) if ("l2_cls", c, 3) in union}
    assert dense == {3, 4, 5, 6, 7, 8}, dense                                  # every class that can be dense is
    assert ("l2_cls", 1, 1) in union and ("l2_cls", 1, 2) in union             # one-symbol and raw class-1 blocks
    for branch, why in UNREACHABLE.items():
        assert branch not in union, (branch, "listed as unreachable, but the encoder wrote it:", why)
    # the four tie outcomes (first minimum wins: 0, 0, 2, 1) are checked tile by tile in test_chooser_returns_the_wanted_predictor_on_every_tile
    for kind, p in S.TIES.items():
        assert ("l1_pr", 3, p) in survey[f"tie_{kind}_rgb_900x460"][0] and ("l1_pr", 4, p) in survey[f"tie_{kind}_rgba_900x460"][0]


# ================================================================================================ GPU: bit-exact against the oracle
# Which kernel form a geometry selects (xpng_hip.hip launch_transform; recon.hpp recon_geometry, for m1_decode.hpp decode_m1_plan and
# m2_decode.hpp decode_m2_launch alike):
#   transform       tiles up to TR_MAXW = 672 px wide: the LDS-staged k_m1_transform_rgba / _rgb (m1_pixel_interior, byte-parallel);
#                   wider (30000 x 4, 2500 x 70): k_m1_transform_generic (m1_pixel, scalar).
#   reconstruction  narrow entropy path, or wide with a tile beyond RB_MAXW = 2048 px: k_dec_recon<PXSZ, DecTile / M2DecTile>, which runs
#                   recon_free when the tile is at most 1024 rows and its rows fit the LDS (900 x 460, 64 x 64, 2500 x 70) and
#                   recon_wavefront otherwise (30000 x 4: rows too long; 7 x 9000: nine bands of 1024 rows with seams);
#                   wide entropy path (XPNG_WIDE_RANS=1 or more than 2048 chains) and tiles up to 2048 px: k_dec_recon_band<PXSZ,
#                   DecTile / M2DecTile> (recon_band_core).
#   routing         by small_blocks(items) = items > 2048 (common.hpp), a selector of its own that no environment variable of the release
#                   library moves: up to 2048 (tile, stream) items k_m1_streams<PXSZ, 1024> (launch_encode_m1), k_m2_streams<1024>
#                   (launch_encode_m2) and k_m2_dec_resid<1024> (decode_m2_launch), 4096 pixels per loop iteration; beyond,
#                   k_m1_streams<PXSZ, 256>, k_m2_streams<256> and k_m2_dec_resid<256>, 1024 pixels per iteration.  XPNG_WIDE_RANS=1 on the
#                   single images here keeps the 1024-thread form beside the wide chains; only the batches below that select the wide
#                   kernels by their size run the 256-thread form (tests/test_iteration_edges.py crafts tiles for it).
_ORACLE = {}


def _blobs(po, name, level):
    """The oracle's tile blobs of a named raster (computed once, shared, never changed)."""
    if (name, level) not in _ORACLE:
        _ORACLE[(name, level)] = po.encode_tiles(level, S.raster(name))
    return _ORACLE[(name, level)]


def _encode_then_decode(gpu, raster, want, level, what, shifts=(0,)):
    """encode_device gives `want`; decode_device of `want` into a sentinel-filled buffer gives the raster and leaves the sentinel
    around it (at every shift of the destination)."""
    import torch
    h, w, ch = raster.shape
    ctx = gpu.Context(w, h, ch)
    try:
        d_r = torch.from_numpy(raster.copy()).cuda()
        d_b = torch.zeros(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(level, d_r.data_ptr(), d_b.data_ptr())
        assert n == len(want) and d_b[:n].cpu().numpy().tobytes() == want, (what, "encode")
        d_blob = torch.from_numpy(np.frombuffer(want + b"\0" * 64, dtype=np.uint8).copy()).cuda()
        nbytes = w * h * ch
        for shift in shifts:
            buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
            ctx.decode_device(level, d_blob.data_ptr(), len(want), None, buf.data_ptr() + 64 + shift)
            assert ctx.decode_status() == 0, (what, shift)
            out = buf.cpu().numpy()
            assert np.array_equal(out[64 + shift:64 + shift + nbytes].reshape(h, w, ch), raster), (what, "decode", shift)
            assert (out[:64 + shift] == 0xA5).all() and (out[64 + shift + nbytes:] == 0xA5).all(), (what, "sentinel", shift)
    finally:
        ctx.close()


STAGE = [f"pr{p}_{f}_{s}" for p in (1, 2, 3) for f in ("rgb", "rgba") for s in ("900x460", "30000x4")] + \
        [f"tie_{k}_{f}_900x460" for k in S.TIES for f in ("rgb", "rgba")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE)
def test_stage_planes_and_streams_on_steered_predictors(gpu, po, name):
    """What test_stage_planes_and_streams_match_oracle does for predictor 0, for predictors 1, 2, 3 and the four cost ties: chooser
    sums and choice, the residual planes, then the nine context streams, k and every rANS block, per tile.  900 x 460: two tiles
    through the LDS-staged transform (m1_pixel_interior: 16-bit-lane gradient, byte-parallel green-subtract); 30000 x 4: one tile
    wider than TR_MAXW through k_m1_transform_generic (m1_pixel, scalar gradient)."""
    import torch
    raster = S.raster(name)
    h, w, ch = raster.shape
    ctx = gpu.Context(w, h, ch)
    try:
        d_r = torch.from_numpy(raster.copy()).cuda()
        d_b = torch.zeros(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda")
        assert ctx.tiles() == po.tile_table(w, h, ch)
        ctx.transform_device(d_r.data_ptr())
        keep = []
        for ti, t in enumerate(ctx.tiles()):
            pr, sums = po.choose_predictor(raster, t)
            assert pr & 3 == S.named()[name][1]["pr"]
            assert ctx.fetch("sums", ti).view(np.uint32).tolist() == sums, (name, ti)
            assert int(ctx.fetch("pr", ti)[0]) == pr, (name, ti)
            planes = po.m1_planes(raster, t, pr)
            for k in ("nl", "r", "g", "b") + (("a",) if ch == 4 else ()):
                assert np.array_equal(ctx.fetch(k, ti), planes[k]), (name, ti, k)
            keep.append((pr, planes))
        n = ctx.encode_device(1, d_r.data_ptr(), d_b.data_ptr())
        assert d_b[:n].cpu().numpy().tobytes() == _blobs(po, name, 1), name
        for ti, t in enumerate(ctx.tiles()):
            pr, planes = keep[ti]
            assert int(ctx.fetch("pr", ti)[0]) == pr
            st = po.m1_streams(raster, t, planes)
            for c in range(9):
                assert np.array_equal(ctx.fetch(10 + c, ti), st["ctx"][c]), (name, ti, c)
            assert np.array_equal(ctx.fetch("k", ti).view(np.uint32), st["k"]), (name, ti)
            for c in range(9):
                assert ctx.fetch(20 + c, ti).tobytes() == po.rans2_encode(st["F"][c], 9, st["ctx"][c], 12), (name, ti, c)
            if ch == 4:
                assert np.array_equal(ctx.fetch("a", ti)[1:], planes["a"][1:]), (name, ti)
                assert ctx.fetch(29, ti).tobytes() == po.rans2_encode(st["FA"], 256, planes["a"][1:], 15), (name, ti)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("force_wide", [False, True])
@pytest.mark.parametrize("size,level", [(s, 1) for s in S.SIZES + S.BAND_SIZES] + [((900, 460), 2), ((7, 9000), 2)])
def test_every_predictor_encodes_and_decodes(gpu, po, monkeypatch, size, level, force_wide):
    """Every predictor (RGB and RGBA at level 1, RGB at level 2) through encode_device / decode_device, bytes and pixels, on the
    narrow entropy path and with XPNG_WIDE_RANS=1.  Narrow: 900 x 460 and 64 x 64 reach the LDS-staged transforms and recon_free;
    30000 x 4 k_m1_transform_generic and recon_wavefront (rows too long for the LDS form); 7 x 9000 recon_wavefront across eight
    band seams.  Forced wide: recon_band_core for every tile up to 2048 px; 30000 x 4 and 2500 x 70 are wider than its seam
    buffer, so k_dec_recon takes over beside the wide chains (recon_wavefront and recon_free respectively).  The band sizes
    (453 x 130, 1003 x 777, 2500 x 70) carry the gradient predictors only."""
    if force_wide:
        monkeypatch.setenv("XPNG_WIDE_RANS", "1")
    w, h = size
    done = 0
    for pr in range(4):
        for fmt in ("rgb", "rgba") if level == 1 else ("rgb",):
            name = f"pr{pr}_{fmt}_{w}x{h}"
            if name in S.named():
                _encode_then_decode(gpu, S.raster(name), _blobs(po, name, level), level, (name, level, force_wide))
                done += 1
    assert done >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(1003, 777), (453, 130)])
def test_band_reconstruction_with_gradient_and_green(gpu, po, monkeypatch, geom):
    """recon_band_core (forced wide path) on steered predictor-2 and predictor-3 rasters, RGBA and RGB, with the destination at each
    16-byte phase of a 64-byte line, as test_band_reconstruction_row_staging_at_every_alignment does for predictor 0: the
    byte-parallel gradient and the green add-back inside the band form, chunk phases included."""
    monkeypatch.setenv("XPNG_WIDE_RANS", "1")
    for pr in (2, 3):
        for fmt in ("rgba", "rgb"):
            name = f"pr{pr}_{fmt}_{geom[0]}x{geom[1]}"
            _encode_then_decode(gpu, S.raster(name), _blobs(po, name, 1), 1, name, shifts=(0, 16, 32, 48))


@pytest.mark.gpu
@pytest.mark.parametrize("force_wide", [False, True])
@pytest.mark.parametrize("kind", list(S.GRAY))
def test_level2_gray_modes(gpu, po, monkeypatch, kind, force_wide):
    """Every gray mode (0x20 left, 0x21 up, 0x22 average, 0x23 gradient, 0x28 raw), the one-symbol block and the two exact ties
    (k_m2_gray_syms, k_m2_select with its first-minimum rule) through encode_device(2) and decode_device(2).  420 x 300: recon_free
    (narrow) / recon_band_core (wide) with predictor modes 2 (left) and 1 (gradient) among them; 7 x 9000: recon_wavefront
    (narrow) / recon_band_core (wide) across band seams."""
    if force_wide:
        monkeypatch.setenv("XPNG_WIDE_RANS", "1")
    for name, (_, meta) in S.named().items():
        if meta.get("kind") == kind:
            want = _blobs(po, name, 2)
            assert want[3] == S.GRAY[kind], name
            _encode_then_decode(gpu, S.raster(name), want, 2, (name, force_wide))


@pytest.mark.gpu
@pytest.mark.parametrize("force_wide", [False, True])
def test_gray_left_and_gradient_beside_colour_tiles(gpu, po, monkeypatch, force_wide):
    """Gray "left" and gray "gradient" tiles beside a colour tile (predictor 3) and a single-colour tile in one raster: the four
    tiles of one launch take four different paths (recon_head, recon_fill) of k_dec_recon / k_dec_recon_band<3, M2DecTile>."""
    if force_wide:
        monkeypatch.setenv("XPNG_WIDE_RANS", "1")
    name = "mixed_gray_1000x900"
    want = _blobs(po, name, 2)
    assert {t[0] for t in census(S.raster(name), 2)} >= {"gray", "l2", "l2_pr"}
    _encode_then_decode(gpu, S.raster(name), want, 2, (name, force_wide))


@pytest.mark.gpu
@pytest.mark.parametrize("force_wide", [False, True])
def test_rarely_written_block_forms(gpu, po, monkeypatch, force_wide):
    """Level 2: one-symbol, raw, dense, sparse and empty class blocks (flat tile with single outliers; 1-, 2- and 3-bit noise).
    Level 1: alpha blocks of one symbol, raw, and with a dense table.  Bytes and round trip."""
    if force_wide:
        monkeypatch.setenv("XPNG_WIDE_RANS", "1")
    for name in S.named():
        if name.startswith("l2_"):
            _encode_then_decode(gpu, S.raster(name), _blobs(po, name, 2), 2, (name, force_wide))
        if name.startswith("alpha_"):
            _encode_then_decode(gpu, S.raster(name), _blobs(po, name, 1), 1, (name, force_wide))


def _batch_round_trip(gpu, level, rasters, wants, B, chains_per_tile):
    """One encode_device_batch and one decode_device_batch over B images cycling through `rasters`."""
    import torch
    h, w, ch = rasters[0].shape
    k = len(rasters)
    ctx = gpu.Context(w, h, ch, batch=B)
    try:
        assert ctx.n_tiles * chains_per_tile * B > 2048                        # the launch selects the wide kernels by itself
        d_src = [torch.from_numpy(r.copy()).cuda() for r in rasters]
        d_b = [torch.zeros(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = ctx.encode_device_batch(level, [d_src[i % k].data_ptr() for i in range(B)], [t.data_ptr() for t in d_b])
        d_want = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in wants]
        for i in range(B):
            assert lens[i] == len(wants[i % k]) and torch.equal(d_b[i][: lens[i]], d_want[i % k]), (level, i)
        nbytes = w * h * ch
        d_o = [torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(B)]
        ctx.decode_device_batch(level, [t.data_ptr() for t in d_b], lens, None, [t.data_ptr() for t in d_o])
        assert ctx.decode_status() == 0
        for i in range(B):
            assert torch.equal(d_o[i][:nbytes], d_src[i % k].reshape(-1)), (level, i)
            assert bool((d_o[i][nbytes:] == 0xA5).all()), (level, i)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["rgba", "rgb"])
def test_level1_batch_of_all_predictors_selects_the_wide_kernels(gpu, po, fmt):
    """A batch big enough to select the wide kernels by itself (tiles x streams x images > 2048), as
    test_large_batch_takes_the_wide_path_and_matches, with the steered predictors 0..3 cycling through its images: chains and
    band reconstructions of tiles with different predictors share wavefronts and workgroup slots."""
    names = [f"pr{p}_{fmt}_900x460" for p in range(4)]
    _batch_round_trip(gpu, 1, [S.raster(n) for n in names], [_blobs(po, n, 1) for n in names], 104 if fmt == "rgba" else 116,
                      10 if fmt == "rgba" else 9)


@pytest.mark.gpu
def test_level2_batch_with_every_gray_mode_selects_the_wide_kernels(gpu, po):
    """The same at level 2: the four predictors and the eight gray rasters, resized to the batch geometry, in one launch (the wide
    rANS v1 kernels; k_m2_gray_syms / k_m2_select and k_dec_recon_band<3, M2DecTile> on tiles of every kind side by side)."""
    rasters = [S.raster(f"pr{p}_rgb_900x460") for p in range(4)] + [S.gray(k, 900, 460) for k in S.GRAY]
    seen = set()
    for r in rasters:
        seen |= census(r, 2)
    assert {("gray", m) for m in (0x20, 0x21, 0x22, 0x23, 0x28)} | {("l2_pr", p) for p in range(4)} <= seen
    wants = [po.encode_tiles(2, np.ascontiguousarray(r)) for r in rasters]
    _batch_round_trip(gpu, 2, rasters, wants, 72, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("level,fmt", [(1, "rgba"), (1, "rgb"), (2, "rgb")])
def test_mixed_size_batch_of_all_predictors(gpu, po, level, fmt):
    """One MixedContext batch holding a raster of each predictor - and, for RGB, of the four gray modes - at different sizes:
    decoded in one call, encoded in one call."""
    import torch
    names = [f"pr0_{fmt}_900x460", f"pr1_{fmt}_64x64", f"pr2_{fmt}_453x130", f"pr3_{fmt}_1003x777", f"pr1_{fmt}_7x9000"]
    if fmt == "rgb":
        names += ["gray_left_420x300", "gray_up_7x9000", "gray_avg_420x300", "gray_grad_420x300", "gray_grad_7x9000"]
    rasters = [S.raster(n) for n in names]
    wants = [_blobs(po, n, level) for n in names]
    ch = rasters[0].shape[2]
    ctx = gpu.MixedContext([(r.shape[1], r.shape[0]) for r in rasters], ch)
    try:
        d_b = [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in wants]
        d_o = [torch.full((r.size + 64,), 0xA5, dtype=torch.uint8, device="cuda") for r in rasters]
        ctx.decode_batch(level, [t.data_ptr() for t in d_b], [len(b) for b in wants], [t.data_ptr() for t in d_o])
        assert ctx.decode_status() == 0
        for n, r, t in zip(names, rasters, d_o):
            got = t.cpu().numpy()
            assert np.array_equal(got[: r.size].reshape(r.shape), r) and (got[r.size:] == 0xA5).all(), (n, level)
        d_r = [torch.from_numpy(r.copy()).cuda() for r in rasters]
        d_e = [torch.full((ctx.blob_bound(i) + 64,), 0xA5, dtype=torch.uint8, device="cuda") for i in range(len(names))]
        lens = ctx.encode_batch(level, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_e])
        for n, want, t, ln in zip(names, wants, d_e, lens):
            got = t.cpu().numpy()
            assert ln == len(want) and got[:ln].tobytes() == want and (got[ln:] == 0xA5).all(), (n, level)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level,fmt", [(1, "rgba"), (1, "rgb"), (2, "rgb")])
def test_region_crop_of_every_predictor(gpu, po, level, fmt):
    """One region decode launch over the four predictors, each with a rectangle of its own that starts inside a tile (and, for
    three of them, reaches into the second tile of the 900 x 460 raster, whose tiles meet at x = 456)."""
    import torch
    names = [f"pr{p}_{fmt}_900x460" for p in range(4)]
    W, H, ch = 900, 460, 4 if fmt == "rgba" else 3
    rects = [(301, 45, 400, 333), (5, 3, 120, 450), (455, 101, 3, 7), (457, 1, 443, 459)]
    ctx = gpu.Context(W, H, ch, batch=4)
    try:
        wants = [_blobs(po, n, level) for n in names]
        d_b = [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in wants]
        out_bpr = max(r[2] for r in rects) * ch + 64
        d_o = [torch.full((r[3] * out_bpr + 256,), 0xA5, dtype=torch.uint8, device="cuda") for r in rects]
        ctx.decode_region_batch(level, [t.data_ptr() for t in d_b], [len(b) for b in wants], rects, [t.data_ptr() for t in d_o], out_bpr)
        assert ctx.decode_status() == 0
        for n, (x, y, w, h), t in zip(names, rects, d_o):
            got = t.cpu().numpy()
            rows = got[: h * out_bpr].reshape(h, out_bpr)
            assert np.array_equal(rows[:, : w * ch].reshape(h, w, ch), S.raster(n)[y:y + h, x:x + w]), (n, level)
            assert (rows[:, w * ch:] == 0xA5).all() and (got[h * out_bpr:] == 0xA5).all(), (n, level, "padding written")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_tile_range_sharding_on_gradient_and_green_tiles(gpu, po):
    """test_tile_range_sharding_concatenates_to_whole on the four tiles of a predictor-3 RGBA and a predictor-2 RGB raster, and at
    level 2: ranges encoded apart concatenate to the whole."""
    import torch
    for name, level in (("pr3_rgba_1003x777", 1), ("pr2_rgb_1003x777", 1), ("pr3_rgb_1003x777", 2)):
        raster = S.raster(name)
        h, w, ch = raster.shape
        ctx = gpu.Context(w, h, ch)
        try:
            d_r = torch.from_numpy(raster.copy()).cuda()
            d_b = torch.zeros(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda")
            parts = b""
            for a, b in ((0, 1), (1, 3), (3, 4)):
                n = ctx.encode_device(level, d_r.data_ptr(), d_b.data_ptr(), t0=a, t1=b)
                parts += d_b[:n].cpu().numpy().tobytes()
            assert parts == _blobs(po, name, level), (name, level)
        finally:
            ctx.close()
