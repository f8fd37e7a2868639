"""The merged serial launches of the batched (wide) level-1 form (run with -m gpu on an MI355X).

A wide level-1 decode runs its alpha chains and its lane-per-tile context walk as two workgroup ranges of ONE launch (k_dec_serial:
alpha groups first, none for RGB), a wide encode its alpha and its nine context chain classes alike (k_rans2_chain_all), everything
on the caller's stream.  The shapes are chosen for the role boundaries: a single partly filled group of either role, whole groups
with a half-filled last walk wavefront, one workgroup per role with two live lanes, an empty alpha range, raw and one-symbol
blocks, raw tiles that every role must pass by.  Every case forces the wide form (XPNG_WIDE_RANS=1), runs ONE device call per batch,
compares byte for byte with the oracle (encode_tiles / decode_tiles) and with the narrow form (XPNG_NARROW_RANS=1), and checks the
0xA5 guard behind every output.  Only blobs the oracle's encoder or the crafting kit wrote reach the GPU."""
import numpy as np
import pytest

import _rans_tables as rt

from _kit import gpu, po

pytestmark = pytest.mark.gpu

_CACHE = {}


def _items(po, kind, W, H, alpha, seeds):
    """[(raster, the oracle's tile blobs of it)], made once per raster and shared by the cases; the oracle's decode of the blobs is
    the raster (asserted once, here)"""
    from xpng_amd.synth import synth_raster
    ch = 3 + int(alpha)
    out = []
    for seed in seeds:
        key = (kind, W, H, alpha, seed)
        if key not in _CACHE:
            raster = synth_raster(kind, W, H, alpha, seed=seed)
            blobs = po.encode_tiles(1, raster)
            assert np.array_equal(po.decode_tiles(1, blobs, W, H, ch), raster)
            raster.setflags(write=False)
            _CACHE[key] = (raster, blobs)
        out.append(_CACHE[key])
    return out


def _upload(blobs):
    import torch
    return torch.from_numpy(np.frombuffer(blobs + b"\0" * 64, dtype=np.uint8).copy()).cuda()


def _guarded(n):
    import torch
    return torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")


def _check_decode(gpu, monkeypatch, items, W, H, ch, B):
    """items: the distinct (expected raster, blobs) of the batch, taken in turn for its B images"""
    import torch
    from xpng_amd import api
    from xpng_amd.api import walk_tile_offsets
    for want, blobs in items:
        with monkeypatch.context() as m:
            m.setenv("XPNG_NARROW_RANS", "1")
            assert np.array_equal(api.decode_tiles(1, blobs, W, H, ch), want), "narrow form"
    ctx = gpu.Context(W, H, ch, batch=B)
    try:
        pick = [items[i % len(items)] for i in range(B)]
        d_b = [_upload(p[1]) for p in pick]
        n = W * H * ch
        d_o = [_guarded(n) for _ in range(B)]
        with monkeypatch.context() as m:
            m.setenv("XPNG_WIDE_RANS", "1")
            ctx.decode_device_batch(1, [t.data_ptr() for t in d_b], [len(p[1]) for p in pick],
                                    [walk_tile_offsets(p[1], ctx.n_tiles)[0] for p in pick], [t.data_ptr() for t in d_o])
            torch.cuda.synchronize()
        assert ctx.decode_status() == 0
        for i in range(B):
            got = d_o[i].cpu().numpy()
            assert np.array_equal(got[:n].reshape(H, W, ch), pick[i][0]), i
            assert bool((got[n:] == 0xA5).all()), i
    finally:
        ctx.close()


def _check_encode(gpu, monkeypatch, items, W, H, ch, B):
    """The batched wide bytes equal the oracle's and the narrow form's, and a second call on the same context gives them again
    (every kernel of the call is on one stream now: the side stream used to hide ordering mistakes between prep and chain)."""
    import torch
    from xpng_amd import api
    for raster, want in items:
        with monkeypatch.context() as m:
            m.setenv("XPNG_NARROW_RANS", "1")
            assert api.encode_tiles(1, raster) == want, "narrow form"
    ctx = gpu.Context(W, H, ch, batch=B)
    try:
        pick = [items[i % len(items)] for i in range(B)]
        d_r = [torch.from_numpy(np.concatenate([p[0].reshape(-1), np.zeros(64, np.uint8)])).cuda() for p in pick]
        for call in range(2):
            d_e = [_guarded(ctx.blob_bound()) for _ in range(B)]
            with monkeypatch.context() as m:
                m.setenv("XPNG_WIDE_RANS", "1")
                lens = ctx.encode_device_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_e])
            for i in range(B):
                got = d_e[i].cpu().numpy()
                assert lens[i] == len(pick[i][1]) and got[: lens[i]].tobytes() == pick[i][1], (call, i)
                assert bool((got[lens[i]:] == 0xA5).all()), (call, i)
    finally:
        ctx.close()


_CHECK = {"decode": _check_decode, "encode": _check_encode}
DIRS = ["decode", "encode"]


@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("alpha", [True, False])
@pytest.mark.parametrize("B", [3, 32])
def test_nine_tiles_of_three_sizes(gpu, po, monkeypatch, direction, alpha, B):
    """1501 x 1203: nine tiles, three of them >= 3/4 of the largest.  B = 3: 27 work items, no whole wavefront of either role and a
    single partly filled alpha group.  B = 32: 288 items, nine full alpha groups and 4.5 walk wavefronts (the last half full).
    RGB: the alpha range is empty."""
    W, H, ch = 1501, 1203, 3 + int(alpha)
    sizes = [t[2] * t[3] for t in po.tile_table(W, H, ch)]
    assert len(sizes) == 9 and sum(4 * n >= 3 * max(sizes) for n in sizes) == 3
    _CHECK[direction](gpu, monkeypatch, _items(po, "photo", W, H, alpha, (1, 2)), W, H, ch, B)


@pytest.mark.parametrize("direction", DIRS)
def test_one_workgroup_per_role(gpu, po, monkeypatch, direction):
    """900 x 460 RGBA, B = 2: two equal tiles, so both roles have exactly one workgroup, each with two live lanes."""
    assert len(po.tile_table(900, 460, 4)) == 2
    _CHECK[direction](gpu, monkeypatch, _items(po, "photo", 900, 460, True, (1, 2)), 900, 460, 4, 2)


@pytest.mark.parametrize("direction,W,H,alpha", [(d, w, h, a) for d in DIRS for (w, h) in ((64, 64), (5, 7)) for a in (True, False)] + [("decode", 1, 5, False)])
def test_tiny_tiles(gpu, po, monkeypatch, direction, W, H, alpha):
    """Raw and one-symbol blocks, and raw tiles that every role must pass by.  (Level 1 has no RGBA raster narrower than 4 pixels:
    1 x 5 is RGB, and decode only.)"""
    items = _items(po, "photo", W, H, alpha, (1, 2, 3)) + _items(po, "noise", W, H, alpha, (1,))
    _CHECK[direction](gpu, monkeypatch, items, W, H, 3 + int(alpha), 5)


@pytest.mark.parametrize("direction", DIRS)
def test_crafted_tables_in_front_of_the_merged_launch(gpu, po, monkeypatch, direction):
    """tests/_rans_tables.craft_m1_variants: the rest-kernel and every context-chain layout in front of the merged launch (decode
    takes the crafted blobs, encode the rasters they decode to)."""
    W, H = 300, 200
    variants = rt.craft_m1_variants(W, H)[:8]
    if direction == "decode":
        profs = [p for v in variants for p in v[3] if p["layout"] != "alpha"]
        assert any(p["layout"] == "rest" for p in profs) and any(p["layout"] == "small" for p in profs)
        items = []
        for name, raster, blobs, _ in variants:
            assert np.array_equal(po.decode_tiles(1, blobs, W, H, 4), raster), name
            items.append((raster, blobs))
    else:
        items = [(np.ascontiguousarray(raster), po.encode_tiles(1, raster)) for _, raster, _, _ in variants]
    _CHECK[direction](gpu, monkeypatch, items, W, H, 4, 8)


def test_mixed_sizes_in_one_call(gpu, po, monkeypatch):
    """Three RGBA images of different sizes - 1501 x 1203, 64 x 64 and 900 x 460: twelve work items of five tile sizes - decoded and
    encoded by one call each of the mixed-batch API, wide against the oracle and against the narrow form."""
    import torch
    dims = [(1501, 1203), (64, 64), (900, 460)]
    items = [_items(po, "photo", w, h, True, (1,))[0] for (w, h) in dims]
    rasters, wants = [it[0] for it in items], [it[1] for it in items]
    ctx = gpu.MixedContext(dims, 4)
    try:
        d_b = [_upload(b) for b in wants]
        d_r = [torch.from_numpy(np.concatenate([r.reshape(-1), np.zeros(64, np.uint8)])).cuda() for r in rasters]
        for form in ("XPNG_WIDE_RANS", "XPNG_NARROW_RANS", "XPNG_WIDE_RANS"):  # (the wide form twice: the second call on the same context)
            d_o = [_guarded(r.size) for r in rasters]
            d_e = [_guarded(ctx.blob_bound(i)) for i in range(len(dims))]
            with monkeypatch.context() as m:
                m.setenv(form, "1")
                ctx.decode_batch(1, [t.data_ptr() for t in d_b], [len(b) for b in wants], [t.data_ptr() for t in d_o])
                torch.cuda.synchronize()
                assert ctx.decode_status() == 0
                lens = ctx.encode_batch(1, [t.data_ptr() for t in d_r], [t.data_ptr() for t in d_e])
            for i, (r, want) in enumerate(zip(rasters, wants)):
                got = d_o[i].cpu().numpy()
                assert np.array_equal(got[: r.size].reshape(r.shape), r) and bool((got[r.size:] == 0xA5).all()), (form, i)
                enc = d_e[i].cpu().numpy()
                assert lens[i] == len(want) and enc[: lens[i]].tobytes() == want, (form, i)
                assert bool((enc[lens[i]:] == 0xA5).all()), (form, i)
    finally:
        ctx.close()
