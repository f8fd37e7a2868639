"""Symbol lookup of the rANS decoders on tables that reach every branch (run with -m gpu on an MI355X).

The wide alpha chain (k_rans2_dec_chain<true>, rans2_wide_dec.hpp) resolves a slot by one of five routes - the hot pair in
registers, the exact coarse byte (rsh == 0 on the whole wave), one count8 round, a second round, the plain scan - and the
context streams take the register-searched small layout or k_rans2_decode_rest.  Every case first asserts, with
tests/_rans_tables.lookup_profile on the oracle's or the crafted bytes, that it reaches the route it names."""
import os

import numpy as np
import pytest

import _rans_tables as rt

from _kit import gpu, po

pytestmark = pytest.mark.gpu


def _load_both_ways(gpu, monkeypatch, path, want, what):
    for env in ("XPNG_NARROW_RANS", "XPNG_WIDE_RANS"):
        with monkeypatch.context() as m:
            m.setenv(env, "1")
            assert np.array_equal(gpu.load(path), want), (what, env)


@pytest.mark.parametrize("shape", list(rt.ALPHA_SHAPES) + ["recipe"])
def test_reference_writable_alpha_shapes(gpu, po, monkeypatch, tmp_path, shape):
    """Alpha tables the reference encoder writes, one per lookup route: store bytes == oracle, load == the normalised raster on
    the narrow and on the wide path."""
    if shape == "recipe":
        raster, W, H, route = rt.scan_recipe_raster(), 888, 444, "scan"
    else:
        raster, W, H, route = rt.shape_raster(shape), rt.SHAPE_W, rt.SHAPE_H, rt.ALPHA_ROUTES[shape]
    want = po.encode_image(1, raster)
    profs = [rt.lookup_profile(pb, F) for pb, F in rt.alpha_block_tables(want[8:], W, H)]
    assert any(p["route"] == route for p in profs), (shape, profs)
    p = profs[0]
    if shape == "exact":
        assert p["rsh"] == 0 and (rt.alpha_block_tables(want[8:], W, H)[0][1] == 1).sum() >= 200
    elif shape == "two":
        assert p["cold"] == 0
    elif shape == "tied":
        assert p["F0"] == p["F1"] and p["hot0"] > p["hot1"]
    elif shape == "hot_inside":
        F = rt.alpha_block_tables(want[8:], W, H)[0][1]
        assert p["straddles"] >= 2 and all(F[h - 1] and F[h + 1] for h in (p["hot0"], p["hot1"]))
    elif shape in ("scan", "recipe"):
        assert any(q["rsh"] >= 5 and q["max_bound"] >= 17 for q in profs)
    path = str(tmp_path / "a.xpng")
    gpu.store(1, raster, path)
    assert open(path, "rb").read() == want, shape
    _load_both_ways(gpu, monkeypatch, path, np.ascontiguousarray(po.normalize_rgba(raster)), shape)


def test_alpha_shapes_share_one_wide_launch(gpu, po):
    """224 single-tile images, the seven shapes in turn: a batch that selects the wide path by itself, in which every 32-stream
    alpha wave mixes exact and non-exact streams, hot-hit and cold lanes, and a cold-free stream.  Encode bytes == oracle,
    decode == raster, status 0, nothing written behind an output."""
    import torch
    from xpng_amd.api import walk_tile_offsets
    names = list(rt.ALPHA_SHAPES)
    base = [rt.shape_raster(n) for n in names]
    W, H, B = rt.SHAPE_W, rt.SHAPE_H, 224
    ctx = gpu.Context(W, H, 4, batch=B)
    try:
        assert ctx.n_tiles * 10 * B > 2048
        want = [po.encode_tiles(1, r) for r in base]
        profs = [rt.lookup_profile(*rt.alpha_block_tables(w, W, H)[0]) for w in want]
        wave = [profs[i % len(names)] for i in range(32)]
        assert {p["rsh"] == 0 for p in wave} == {True, False} and len({p["route"] for p in wave}) == 4
        d_r = [torch.from_numpy(base[i % len(names)]).cuda() for i in range(B)]
        d_b = [torch.empty(ctx.blob_bound() + 64, dtype=torch.uint8, device="cuda") for _ in range(B)]
        lens = ctx.encode_device_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_b])
        offs = []
        for i in range(B):
            blob = d_b[i][:lens[i]].cpu().numpy().tobytes()
            assert blob == want[i % len(names)], i
            offs.append(walk_tile_offsets(blob, ctx.n_tiles)[0])
        n = W * H * 4
        d_o = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(B)]
        ctx.decode_device_batch(1, [t.data_ptr() for t in d_b], lens, offs, [t.data_ptr() for t in d_o])
        torch.cuda.synchronize()
        assert ctx.decode_status() == 0
        for i in range(B):
            got = d_o[i].cpu().numpy()
            assert np.array_equal(got[:n].reshape(H, W, 4), base[i % len(names)]), (i, names[i % len(names)])
            assert bool((got[n:] == 0xA5).all()), i
    finally:
        ctx.close()


def test_crafted_tables_decode_five_ways(gpu, po, monkeypatch):
    """Decode-only files (tests/_rans_tables.craft_m1_variants): context blocks at pb 10..12 in every table shape (symbol 8 in
    the table, zero holes, one dominant symbol, N > 9 with trailing zeros), alpha blocks at pb 10..14 (dense-bucket and flat)
    and a one-symbol alpha table, each in dense and sparse form.  Narrow; forced wide; one natural-wide batch whose images
    carry different re-codings; decode_region_batch over that batch; the device-side size walk.  Each == the raster == the
    oracle's decode."""
    import torch
    from xpng_amd import api
    from xpng_amd.api import walk_tile_offsets
    variants = rt.craft_m1_variants()
    routes = {(p["layout"], p["pb"], p["route"] if p["layout"] == "alpha" else p["N"] > 9) for v in variants for p in v[3]}
    assert {("small", pb, False) for pb in (10, 11, 12)} | {("rest", pb, True) for pb in (10, 11, 12)} <= routes
    assert {r[2] for r in routes if r[0] == "alpha" and r[1] < 15} >= {"round1", "round2", "scan"}
    assert any(p["single"] for v in variants for p in v[3])
    H, W, ch = variants[0][1].shape
    for name, raster, blobs, _ in variants:
        assert np.array_equal(po.decode_tiles(1, blobs, W, H, ch), raster), name
        for env in ("XPNG_NARROW_RANS", "XPNG_WIDE_RANS"):
            with monkeypatch.context() as m:
                m.setenv(env, "1")
                assert np.array_equal(api.decode_tiles(1, blobs, W, H, ch), raster), (name, env)
    B = 210
    ctx = gpu.Context(W, H, ch, batch=B)
    try:
        assert ctx.n_tiles * 10 * B > 2048
        pick = [variants[i % len(variants)] for i in range(B)]
        d_b = [torch.from_numpy(np.frombuffer(v[2] + b"\0" * 64, dtype=np.uint8).copy()).cuda() for v in pick]
        lens = [len(v[2]) for v in pick]
        offs = [walk_tile_offsets(v[2], ctx.n_tiles)[0] for v in pick]
        n = W * H * ch
        for walk in ("host", "device"):
            d_o = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(B)]
            ctx.decode_device_batch(1, [t.data_ptr() for t in d_b], lens, offs if walk == "host" else None,
                                    [t.data_ptr() for t in d_o])
            torch.cuda.synchronize()
            assert ctx.decode_status() == 0, walk
            for i in range(B):
                got = d_o[i].cpu().numpy()
                assert np.array_equal(got[:n].reshape(H, W, ch), pick[i][1]), (walk, i, pick[i][0])
                assert bool((got[n:] == 0xA5).all()), (walk, i)
        rng = np.random.default_rng(2)
        rects = []
        for i in range(B):
            x, y = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
            rects.append((0, 0, W, H) if i % 3 == 0 else (x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
        out_bpr = W * ch + 64
        d_o = [torch.full((r[3] * out_bpr + 64,), 0xA5, dtype=torch.uint8, device="cuda") for r in rects]
        ctx.decode_region_batch(1, [t.data_ptr() for t in d_b], lens, rects, [t.data_ptr() for t in d_o], out_bpr, tile_offs=offs)
        assert ctx.decode_status() == 0
        torch.cuda.synchronize()
        for i, (x, y, w, h) in enumerate(rects):
            got = d_o[i].cpu().numpy()
            rows = got[: h * out_bpr].reshape(h, out_bpr)
            assert np.array_equal(rows[:, : w * ch].reshape(h, w, ch), pick[i][1][y:y + h, x:x + w]), (i, rects[i], pick[i][0])
            assert (rows[:, w * ch:] == 0xA5).all() and (got[h * out_bpr:] == 0xA5).all(), (i, "padding written")
    finally:
        ctx.close()


def test_level2_gray_tile_scan(gpu, po, monkeypatch, tmp_path):
    """Level-2 gray tile whose 256-symbol pb-15 table puts more than 16 boundaries in one 64-slot coarse bucket: the forward
    scan of k_rans1_dec_chain<true> (rans1_wide_dec.hpp) runs long.  Bytes == oracle, round trip narrow and wide."""
    raster = rt.gray_scan_raster()
    H, W, _ = raster.shape
    want = po.encode_image(2, raster)
    tabs = [rt.gray_table(t) for t in rt.tile_blobs(want[8:], len(po.tile_table(W, H, 3)))]
    assert tabs[0] is not None and rt.gray_profile(tabs[0][1])["max_bound"] > 16
    path = str(tmp_path / "g.xpng")
    gpu.store(2, raster, path)
    assert open(path, "rb").read() == want
    _load_both_ways(gpu, monkeypatch, path, raster, "gray")
    assert os.path.getsize(path) == len(want)
