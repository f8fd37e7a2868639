"""The top class of the batched (wide) level-1 encode (run with -m gpu on an MI355X).

In a size-sorted wide RGBA launch the alpha streams of the biggest tiles - the tiles as large as the largest, when the cut rule
(xpng_amd/csrc/top_class_cut.hpp, tests/test_top_class_cut_host.py) takes them: k tiles, work items [0, n1 = k * B) - get a wavefront
each (the narrow alpha role of k_rans2_chain_all) in front of the wide alpha groups, which start at work item n1, and k_rans2_prep
leaves their tables in the layout that role reads.  The shapes put n1 off a multiple of 32 (2 and 3 with k = 1, 4 with two equal
top tiles), leave the cut out (four equal tiles; RGB has no alpha role) and the contents put every block type into the top tile's
alpha stream - rANS, one symbol (type 1), raw (type 2), a raw tile - in every image of a batch or in one image only, so that every
role passes by what is not its own and k_rans2_finish completes what either alpha role left.  Every case forces the wide form
(XPNG_WIDE_RANS=1), runs ONE device call per batch (and the same call again), compares byte for byte with the oracle's encode_tiles
and with the narrow form (XPNG_NARROW_RANS=1), and checks the 0xA5 guard behind every blob.  (The decode has no such role: measured
inside the pipeline, its serial launch is bounded by the lane-per-tile walk, not by the alpha chains - profiles/top_class_timing.txt.)"""
import numpy as np
import pytest

import _rans_tables as rt

from _kit import gpu, po
from xpng_amd.shard import tile_table

pytestmark = pytest.mark.gpu

_CACHE = {}


def _noise_alpha(W, H, seed):
    """alpha bytes uniform over 1..255 (0 mapped to 1): their differences fill the alphabet, the alpha block is stored raw"""
    from xpng_amd.synth import _hash_np
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    a = (_hash_np(xs, ys, 3, seed) >> np.uint64(24)).astype(np.uint8)
    return np.where(a == 0, 1, a).astype(np.uint8)


def _raster(content, W, H, alpha, seed):
    """content: photo | opaque | rawblock | rawtile, or 'top:<content>' - a photo whose top-left tile alone has that content"""
    from xpng_amd.synth import synth_raster
    if content.startswith("top:"):
        x, y, w, h = tile_table(W, H)[0]
        r = synth_raster("photo", W, H, alpha, seed=seed)
        r[y:y + h, x:x + w] = _raster(content[4:], W, H, alpha, seed)[y:y + h, x:x + w]
        return r
    r = synth_raster("noise" if content == "rawtile" else "photo", W, H, alpha, seed=seed)
    if alpha and content == "opaque":
        r[..., 3] = 255
    if alpha and content in ("rawblock", "rawtile"):
        r[..., 3] = _noise_alpha(W, H, seed + 8)
    return r


def _item(po, content, W, H, alpha, seed):
    """(raster, the oracle's tile blobs of it, the kind of every tile's alpha block: 0 = raw tile, else the block type), made once
    and shared by the cases; the oracle's decode of the blobs is the raster (asserted once, here)"""
    key = (content, W, H, alpha, seed)
    if key not in _CACHE:
        ch = 3 + int(alpha)
        raster = _raster(content, W, H, alpha, seed)
        blobs = po.encode_tiles(1, raster)
        assert np.array_equal(po.decode_tiles(1, blobs, W, H, ch), raster)
        kinds = []
        for tile in rt.tile_blobs(blobs, len(tile_table(W, H))):
            kinds.append(0 if tile[3] == 0 else (rt.m1_blocks(tile, ch)[1][9][3] if alpha else -1))
        raster.setflags(write=False)
        _CACHE[key] = (raster, blobs, kinds)
    return _CACHE[key]


def _check_encode(gpu, monkeypatch, items, W, H, ch, B, tile_range=None):
    """items: the distinct (raster, blobs, kinds) of the batch, taken in turn for its B images; tile_range (t0, t1): a context and
    a call for those tiles only, whose bytes are that piece of the oracle's.  A second call on the same context gives the same
    bytes again."""
    import torch
    from xpng_amd import api
    from xpng_amd.api import walk_tile_offsets
    n_tiles = len(tile_table(W, H))
    t0, t1 = tile_range or (0, n_tiles)
    for raster, want, _ in items:
        with monkeypatch.context() as m:
            m.setenv("XPNG_NARROW_RANS", "1")
            assert api.encode_tiles(1, raster) == want, "narrow form"
    ctx = gpu.Context(W, H, ch, batch=B, tile_range=tile_range)
    try:
        pick = [items[i % len(items)] for i in range(B)]
        wants = []
        for _, blobs, _ in pick:
            off, end = walk_tile_offsets(blobs, n_tiles)
            off = list(off) + [end]
            wants.append(blobs[off[t0]:off[t1]])
        d_r = [torch.from_numpy(np.concatenate([p[0].reshape(-1), np.zeros(64, np.uint8)])).cuda() for p in pick]
        for call in range(2):
            d_e = [torch.full((ctx.blob_bound(t0, t1) + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(B)]
            with monkeypatch.context() as m:
                m.setenv("XPNG_WIDE_RANS", "1")
                lens = ctx.encode_device_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_e], t0=t0, t1=t1)
            for i in range(B):
                got = d_e[i].cpu().numpy()
                assert lens[i] == len(wants[i]) and got[: lens[i]].tobytes() == wants[i], (call, i)
                assert bool((got[lens[i]:] == 0xA5).all()), (call, i)
    finally:
        ctx.close()


def _sizes(W, H, t0=0, t1=None):
    return sorted((w * h for (_, _, w, h) in tile_table(W, H)[t0:t1]), reverse=True)


TOP_KIND = {"photo": (3, 4), "opaque": (1,), "rawblock": (2,), "rawtile": (0,)}


@pytest.mark.parametrize("content,B", [("photo", 2), ("photo", 3), ("opaque", 2), ("rawblock", 2), ("rawtile", 2)])
def test_one_top_tile_every_block_type(gpu, po, monkeypatch, content, B):
    """988 x 988 RGBA, all four tiles (295 936 / 241 536 x 2 / 197 136): k = 1, n1 = B = 2 or 3 - the wide alpha role starts off a
    multiple of 32 - and the top tile's alpha block is of the kind the content forces, in every image."""
    W = H = 988
    assert _sizes(W, H) == [295936, 241536, 241536, 197136]
    items = [_item(po, content, W, H, True, seed) for seed in (1, 2)]
    assert all(it[2][0] in TOP_KIND[content] for it in items), [it[2] for it in items]
    _check_encode(gpu, monkeypatch, items, W, H, 4, B)


@pytest.mark.parametrize("odd,B", [("top:opaque", 3), ("top:rawblock", 2), ("top:rawtile", 3), ("photo", 3)])
def test_one_image_whose_top_tile_differs_in_kind(gpu, po, monkeypatch, odd, B):
    """988 x 988 RGBA: the top tile of ONE image of the batch has an alpha block of another kind than the others' - a one-symbol
    block, a raw block or a raw tile among rANS blocks, and (odd = photo) a rANS block among one-symbol blocks."""
    W = H = 988
    rest = "opaque" if odd == "photo" else "photo"
    items = [_item(po, odd, W, H, True, 3), _item(po, rest, W, H, True, 1)] + ([_item(po, rest, W, H, True, 2)] if B > 2 else [])
    assert items[0][2][0] in TOP_KIND[odd.replace("top:", "")] and items[1][2][0] in TOP_KIND[rest], [it[2] for it in items]
    assert items[0][2][0] != items[1][2][0]
    _check_encode(gpu, monkeypatch, items, W, H, 4, B)


def test_two_equal_top_tiles_of_a_tile_range(gpu, po, monkeypatch):
    """988 x 988 RGBA, tiles (1, 4) on a context of that range, B = 2: 241 536 x 2 / 197 136, k = 2, n1 = 4."""
    assert _sizes(988, 988, 1, 4) == [241536, 241536, 197136]
    items = [_item(po, "photo", 988, 988, True, seed) for seed in (1, 2)]
    _check_encode(gpu, monkeypatch, items, 988, 988, 4, 2, tile_range=(1, 4))


def test_six_tiles_of_three_sizes(gpu, po, monkeypatch):
    """1432 x 988 RGBA, B = 2: six tiles, one of them the largest."""
    s = _sizes(1432, 988)
    assert len(s) == 6 and s[0] > s[1]
    items = [_item(po, "photo", 1432, 988, True, seed) for seed in (1, 2)]
    _check_encode(gpu, monkeypatch, items, 1432, 988, 4, 2)


def test_four_equal_tiles_have_no_cut(gpu, po, monkeypatch):
    """888 x 888 RGBA, B = 2: four equal tiles, k = 0 - the launch without a narrow role."""
    assert _sizes(888, 888) == [197136] * 4
    items = [_item(po, "photo", 888, 888, True, seed) for seed in (1, 2)]
    _check_encode(gpu, monkeypatch, items, 888, 888, 4, 2)


def test_rgb_has_no_alpha_role(gpu, po, monkeypatch):
    """988 x 988 RGB, B = 2: the same tile sizes and no alpha stream at all."""
    items = [_item(po, "photo", 988, 988, False, seed) for seed in (1, 2)]
    _check_encode(gpu, monkeypatch, items, 988, 988, 3, 2)
