"""Packed context queues of the wide level-1 decode (run with -m gpu on an MI355X).

The batched decode hands the nine context queues of every work item of the lane-per-tile walk (k_dec_walk_wide) from the rANS
kernels to the walk two symbols to a byte (xpng_amd/csrc/rans_dec.hpp: ctxn_*); the big-tile class of a split decode keeps a
symbol to a byte for the scalar walk.  Every case forces the wide form (XPNG_WIDE_RANS=1), decodes a batch in one device call and
compares every image byte for byte with the oracle's decode_tiles and with the narrow form (XPNG_NARROW_RANS=1, which packs
nothing), and checks that nothing is written behind an output.  Only blobs the oracle's encoder or the crafting kits wrote - streams
the parsers accept - reach the GPU."""
import numpy as np
import pytest

import _rans_tables as rt

from _kit import gpu, po

pytestmark = pytest.mark.gpu


def _ctx_block_types(po, blobs, W, H, ch):
    """the v2 block types of the context streams of every coded tile"""
    types = set()
    for tile in rt.tile_blobs(blobs, len(po.tile_table(W, H, ch))):
        if tile[3] != 0:
            types |= {blk[3] for blk in rt.m1_blocks(tile, ch)[1][:9]}
    return types


def _check_batch(gpu, po, monkeypatch, items, W, H, ch, B):
    """items: the distinct (blobs, expected raster) of the batch, taken in turn for its B images"""
    import torch
    from xpng_amd import api
    from xpng_amd.api import walk_tile_offsets
    for blobs, want in items:
        with monkeypatch.context() as m:
            m.setenv("XPNG_NARROW_RANS", "1")
            assert np.array_equal(api.decode_tiles(1, blobs, W, H, ch), want), "narrow form"
    ctx = gpu.Context(W, H, ch, batch=B)
    try:
        pick = [items[i % len(items)] for i in range(B)]
        d_b = [torch.from_numpy(np.frombuffer(p[0] + b"\0" * 64, dtype=np.uint8).copy()).cuda() for p in pick]
        lens = [len(p[0]) for p in pick]
        offs = [walk_tile_offsets(p[0], ctx.n_tiles)[0] for p in pick]
        n = W * H * ch
        d_o = [torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(B)]
        with monkeypatch.context() as m:
            m.setenv("XPNG_WIDE_RANS", "1")
            ctx.decode_device_batch(1, [t.data_ptr() for t in d_b], lens, offs, [t.data_ptr() for t in d_o])
            torch.cuda.synchronize()
        assert ctx.decode_status() == 0
        for i in range(B):
            got = d_o[i].cpu().numpy()
            assert np.array_equal(got[:n].reshape(H, W, ch), pick[i][1]), i
            assert bool((got[n:] == 0xA5).all()), i
    finally:
        ctx.close()


_CACHE = {}


def _items(po, kind, W, H, alpha, seeds):
    """[(the oracle's tile blobs, the oracle's decode of them)], made once per raster and shared by the cases"""
    from xpng_amd.synth import synth_raster
    ch = 3 + int(alpha)
    out = []
    for seed in seeds:
        key = (kind, W, H, alpha, seed)
        if key not in _CACHE:
            blobs = po.encode_tiles(1, synth_raster(kind, W, H, alpha, seed=seed))
            want = po.decode_tiles(1, blobs, W, H, ch)
            want.setflags(write=False)
            _CACHE[key] = (blobs, want)
        out.append(_CACHE[key])
    return out


@pytest.mark.parametrize("kind", ["photo", "flat", "gray"])
@pytest.mark.parametrize("alpha", [True, False])
@pytest.mark.parametrize("B", [3, 32])
def test_two_size_classes_in_one_launch(gpu, po, monkeypatch, kind, alpha, B):
    """1501 x 1203: nine tiles, three of them in the big-tile class.  B = 32: 96 work items keep bytes and go to the scalar walk, 192
    are packed for the lane-per-tile walk, in one launch.  B = 3: the class boundary (9) is no whole wavefront of chains, it is
    rounded down to 0 and every tile is packed."""
    W, H, ch = 1501, 1203, 3 + int(alpha)
    sizes = [t[2] * t[3] for t in po.tile_table(W, H, ch)]
    assert len(sizes) == 9 and sum(4 * n >= 3 * max(sizes) for n in sizes) == 3
    items = _items(po, kind, W, H, alpha, (1, 2) if kind != "flat" else (1,))
    if kind == "flat":
        assert _ctx_block_types(po, items[0][0], W, H, ch) <= {0, 1}  # one queue takes every pop, the other eight are empty
    _check_batch(gpu, po, monkeypatch, items, W, H, ch, B)


@pytest.mark.parametrize("kind", ["photo", "flat", "gray"])
def test_no_split_every_tile_on_the_lane_walk(gpu, po, monkeypatch, kind):
    """900 x 460 RGBA, B = 2: two equal tiles, no size classes - every queue is packed."""
    _check_batch(gpu, po, monkeypatch, _items(po, kind, 900, 460, True, (1, 2)), 900, 460, 4, 2)


@pytest.mark.parametrize("W,H,alpha", [(64, 64, True), (64, 64, False), (5, 7, True), (5, 7, False), (1, 5, False)])
def test_tiny_queues(gpu, po, monkeypatch, W, H, alpha):
    """Queues of a few symbols, odd lengths, most of them empty; short queues also come as raw (type 2) and one-symbol (type 1)
    blocks, which k_rans2_dec_prep packs itself.  (The smallest rasters are stored as raw tiles: no queues at all, every kernel of
    the wide form must pass them by.  Level 1 has no RGBA raster narrower than 4 pixels.)"""
    items = _items(po, "photo", W, H, alpha, (1, 2, 3)) + _items(po, "noise", W, H, alpha, (1,))
    _check_batch(gpu, po, monkeypatch, items, W, H, 3 + int(alpha), 5)


def test_plain_block_types_on_context_streams(gpu, po, monkeypatch):
    """Natural streams whose context blocks are of type 1 (one distinct symbol) and of type 2 (raw symbols) as well as rANS blocks,
    asserted on the oracle's bytes before anything is decoded."""
    seen, items, W, H = set(), [], 64, 64
    for kind, seeds in (("photo", (1, 2)), ("gray", (1,)), ("flat", (1,)), ("noise", (1,))):
        for it in _items(po, kind, W, H, False, seeds):
            seen |= _ctx_block_types(po, it[0], W, H, 3)
            items.append(it)
    assert {1, 2} <= seen and (seen & {3, 4}), seen
    _check_batch(gpu, po, monkeypatch, items, W, H, 3, 7)


def test_crafted_context_tables_reach_the_rest_kernel(gpu, po, monkeypatch):
    """Crafted valid files (tests/_rans_tables.craft_m1_variants): context blocks whose tables name more than nine symbols go to
    k_rans2_decode_rest, which packs through its LDS ring; the others take the chain at pb 10..12, dense and sparse."""
    W, H = 300, 200
    variants = rt.craft_m1_variants(W, H)[:8]
    profs = [p for v in variants for p in v[3] if p["layout"] != "alpha"]
    assert any(p["layout"] == "rest" for p in profs) and any(p["layout"] == "small" for p in profs)
    items = []
    for name, raster, blobs, _ in variants:
        assert np.array_equal(po.decode_tiles(1, blobs, W, H, 4), raster), name
        items.append((blobs, raster))
    _check_batch(gpu, po, monkeypatch, items, W, H, 4, 8)
