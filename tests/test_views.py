"""Several views per image from one mixed-size decode, only the tiles they touch (include/xpng_hip.h
xpnghip_decode_varsize_device_batch_views, xpnghip_view_tiles, xpnghip_ctx_last_decode_tiles; xpng_amd/tensors.py load_views;
DESIGN.md 20).

The checkers are tests/_resample.py (filter 1) and tests/_resize.py (filter 0): the rule in numpy with the C library's fmaf,
independent of the code under test.  Every comparison with the library is on the bits; there is no tolerance anywhere.
CPU: the symbols; xpnghip_view_tiles against a plain restatement (tile tables in Python, the union per image, a stable sort by
decreasing pixel count) on rectangles that end and start exactly on tile boundaries, several views of one image, an image without a
view, NULL view_image, a small cap and bad arguments; load_views on the host-answered kinds with device="cpu".
GPU (-m gpu): the smallest case first (one view in one tile of a two-tile image); the bits of every view for three formats, three
layout words, three dtypes, both filters and both size walks, with the count of decoded tiles; the equivalence with
decode_batch_resampled; a corrupt tile that no view touches goes unnoticed and one that a view touches does not; stale staging
pixels are never read and the cached records of the tight calls survive; the workspace; misuse; load_views on goldens."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from _kit import (BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _offsets, _torch_dtype, _upload, built,
                  consts_from, declared, expect, exported, gpu, mixed_consts, po, table)
from _resample import Resampled
from _resize import Resized
from xpng_amd import api
from xpng_amd.shard import tile_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_decode_varsize_device_batch_views", "xpnghip_view_tiles", "xpnghip_ctx_last_decode_tiles"]
AA, BIL = api.FILTER_TRIANGLE_AA, api.FILTER_BILINEAR
# the smallest shapes at which the selection can go wrong: 2 x 2 tiles, three in a row, two stacked, and two single-tile images
DIMS = [(889, 889), (1333, 445), (200, 2000), (300, 200), (64, 70)]
# (image, rectangle, flip, (OW, OH)): tile 3 only; tiles 0 and 1 (the union leaves tile 2 of image 0 undecoded); the third tile of
# the wide image; the lower tile of the tall one; the whole small image, which grows in y; a part of it, which grows on both axes.
# Image 3 has no view.  The first four shrink on both axes.
VIEWS = [(0, (500, 500, 300, 300), 0, (37, 29)), (0, (400, 100, 80, 300), 1, (96, 64)), (1, (900, 10, 400, 400), 0, (3, 5)),
         (2, (0, 1100, 200, 800), 1, (37, 29)), (4, (0, 0, 64, 70), 0, (96, 64)), (4, (10, 10, 20, 30), 1, (37, 29))]
SELECTED = 6                                                      # of M = 11: tiles 0, 1, 3 of image 0, one each of images 1, 2 and 4


def view_args(views):
    return [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [(v[3][1], v[3][0]) for v in views]   # sizes as (OH, OW)


def restated(dims, view_image, rects):
    """the launch list, plainly: per image the union over its views of the tiles their rectangles intersect, then every selected
    table index by decreasing w * h, equal sizes in table order"""
    tables = [tile_table(w, h) for (w, h) in dims]
    first = np.cumsum([0] + [len(t) for t in tables])
    keep = set()
    for v, i in enumerate(range(len(dims)) if view_image is None else view_image):
        x, y, w, h = rects[v] if rects is not None else (0, 0) + tuple(dims[i])
        hit = [t for t, (tx, ty, tw, th) in enumerate(tables[i]) if tx < x + w and x < tx + tw and ty < y + h and y < ty + th]
        assert hit == api.region_tiles(dims[i][0], dims[i][1], (x, y, w, h))         # (xpnghip_region_tiles' geometry)
        keep |= {int(first[i]) + t for t in hit}
    area = {int(first[i]) + t: tw * th for i, tab in enumerate(tables) for t, (_, _, tw, th) in enumerate(tab)}
    return sorted(sorted(keep), key=lambda t: -area[t])


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_views_symbols_are_declared_listed_and_exported():
    assert set(NEW) <= set(declared("xpng_hip.h", "xpnghip_")) and set(NEW) <= set(api.HIP_SYMBOLS) and set(NEW) <= exported(api.HIP_SO)
    txt = open(os.path.join(ROOT, "include", "xpng_hip.h")).read()
    assert re.search(r"64-byte record per view", txt)
    assert api.hip_lib().xpnghip_abi_version() == 2
    for name in ("decode_batch_views", "last_decode_tiles"):
        assert hasattr(api.MixedContext, name)
    import xpng_amd
    assert "view_tiles" in xpng_amd.__all__ and callable(xpng_amd.view_tiles)


def test_view_tiles_equals_the_restatement():
    assert [len(tile_table(w, h)) for (w, h) in DIMS] == [4, 3, 2, 1, 1]
    assert tile_table(889, 889)[3][:2] == (445, 445) and [t[0] for t in tile_table(1333, 445)] == [0, 445, 889] and tile_table(200, 2000)[1][1] == 1015
    vi, rects, _, _ = view_args(VIEWS)
    got = api.view_tiles(DIMS, vi, rects)
    assert got == restated(DIMS, vi, rects) and len(got) == SELECTED and 2 not in got and 9 not in got
    # 445 x 445 = 198025, then the two 444 x 445 = 197580 in table order, 444 x 444 = 197136, 200 x 985 = 197000, 64 x 70
    assert got == [0, 1, 6, 3, 8, 10]
    cases = [
        ([0], [(0, 0, 445, 445)]),                                  # ends exactly on both boundaries: last column x = 444 -> tile 0 alone
        ([0], [(445, 0, 444, 445)]),                                # starts exactly on the boundary x = 445 -> tile 1 alone
        ([0], [(444, 444, 2, 2)]),                                  # one pixel on every side of the corner: all four
        ([1, 1], [(0, 0, 445, 10), (889, 0, 444, 445)]),            # two views of one image, disjoint tiles
        ([1, 1], [(400, 0, 100, 10), (440, 5, 500, 10)]),           # ... overlapping tiles: {0, 1} and {0, 1, 2}
        ([2, 0, 2], [(0, 1014, 200, 1), (0, 0, 1, 1), (0, 1015, 1, 1)]),   # the row above and the row on the boundary y = 1015
        ([4, 3, 4, 3], None),                                       # NULL rects: whole images, equal sizes in table order
        ([3], [(299, 199, 1, 1)]),
    ]
    for vi, rects in cases:
        assert api.view_tiles(DIMS, vi, rects) == restated(DIMS, vi, rects), (vi, rects)
    assert api.view_tiles(DIMS, [0], [(0, 0, 445, 445)]) == [0] and api.view_tiles(DIMS, [0], [(445, 0, 444, 445)]) == [1]
    assert api.view_tiles(DIMS, [2], [(0, 1014, 200, 1)]) == [7] and api.view_tiles(DIMS, [2], [(0, 1015, 200, 1)]) == [8]
    # NULL view_image is the identity: every image's whole table, in the context's order
    assert api.view_tiles(DIMS, None, None) == restated(DIMS, None, None) and len(api.view_tiles(DIMS, None, None)) == 11
    assert api.view_tiles(DIMS, None, [(0, 0, 1, 1)] * 5) == restated(DIMS, None, [(0, 0, 1, 1)] * 5)
    # the raw entry point: cap, NULLs and bad arguments
    lib = api.hip_lib()
    flat = (C.c_uint64 * 10)(*[v for d in DIMS for v in d])
    arr = (C.c_uint32 * 16)()

    def raw(nviews, vi, rects, cap=16, dims=flat, nimg=5, out=arr):
        return lib.xpnghip_view_tiles(dims, nimg, nviews, None if vi is None else (C.c_uint32 * len(vi))(*vi),
                                      None if rects is None else (C.c_uint64 * (4 * len(rects)))(*[v for r in rects for v in r]), out, cap)

    assert raw(1, [0], [(444, 444, 2, 2)]) == 4 and list(arr[:4]) == [0, 1, 2, 3]
    assert raw(1, [0], [(444, 444, 2, 2)], cap=3) == -1            # cap too small
    assert raw(1, [0], [(444, 444, 2, 2)], cap=4) == 4
    assert raw(1, [0], [(444, 444, 2, 2)], out=None) == -1
    assert raw(1, [5], [(0, 0, 1, 1)]) == -1                       # no such image
    assert raw(1, [0xFFFFFFFF], None) == -1
    assert raw(1, [0], [(0, 0, 0, 1)]) == -1                       # empty
    assert raw(1, [0], [(889, 0, 1, 1)]) == -1                     # leaves the image
    assert raw(1, [4], [(0, 0, 65, 1)]) == -1                      # valid in image 0, not in image 4
    assert raw(1, [0], [(1 << 63, 0, 1 << 63, 1)]) == -1           # x + w overflows
    assert raw(0, [], None) == -1 and raw(65536, [0] * 65536, None, cap=16) == -1
    assert raw(4, None, None) == -1 and raw(5, None, None) == 11   # NULL view_image needs nviews == nimg
    assert raw(1, [0], None, dims=None) == -1 and raw(1, [0], None, nimg=0) == -1
    assert raw(1, [0], None, dims=(C.c_uint64 * 10)(0, 5, *[7] * 8)) == -1
    for bad in (dict(view_image=[5], rects=[(0, 0, 1, 1)]), dict(view_image=[0], rects=[(0, 0, 890, 1)]), dict(view_image=[0, 1], rects=[(0, 0, 1, 1)])):
        with pytest.raises(api.XpngError):
            api.view_tiles(DIMS, **bad)


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(25, 37, False), (39, 16, False)]:
        p = tmp_path / f"l7_{w}x{h}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if w > 30 else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_views_answers_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(37, 25, 3), (1000, 1000, 3), (16, 39, 3)]
    paths.append(str(tmp_path / "never_read.xpng"))                 # no view names it: it need not exist
    views = [(0, (1, 2, 23, 34), True), (2, None, False), (0, None, False), (1, (100, 200, 300, 150), False), (2, (2, 0, 37, 5), True),
             (0, (24, 36, 1, 1), False)]
    sizes = [(6, 5), (3, 7), (40, 30), (2, 2), (9, 4), (1, 1)]     # (OH, OW): shrinking, growing and mixed
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    for dtype in DTYPES:
        for ch, lay, bgr, aa in ((3, "chw", False, True), (4, "hwc", True, True), (3, "hwc", False, False)):
            scale, bias = consts_from(mean[:ch], std[:ch])
            word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
            kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch], antialias=aa)
            got = tensors.load_views(paths, views, sizes, **kw)
            assert isinstance(got, list) and len(got) == len(views)
            exp = []
            for (i, rect, flip), (oh, ow), g in zip(views, sizes, got):
                z = (Resampled if aa else Resized)(want[i], rect, flip, oh, ow).bits(word, dtype, scale, bias)
                raw = api.resample_host(want[i], (oh, ow), word, dtype, scale, bias, rect=rect, flip=flip, filter=AA if aa else BIL)
                assert g.device.type == "cpu" and g.is_contiguous() and tuple(g.shape) == z.shape and g.dtype == _torch_dtype(dtype)
                assert np.array_equal(_bits(g, dtype), z) and np.array_equal(z.reshape(-1), np.frombuffer(raw, BITS[dtype])), (dtype, ch, lay, i, rect)
                exp.append(z)
            # one size for every view, stacked; and out= slices of two stacked tensors of different sizes, written in place
            whole = tensors.load_views(paths, views, (6, 5), stack=True, **kw)
            assert isinstance(whole, torch.Tensor) and tuple(whole.shape) == (len(views),) + ((ch, 6, 5) if lay == "chw" else (6, 5, ch))
            assert np.array_equal(_bits(whole[0], dtype), exp[0])
            for v, (i, rect, flip) in enumerate(views):
                assert np.array_equal(_bits(whole[v], dtype), (Resampled if aa else Resized)(want[i], rect, flip, 6, 5).bits(word, dtype, scale, bias)), v
            shp = lambda oh, ow: (ch, oh, ow) if lay == "chw" else (oh, ow, ch)   # noqa: E731
            big, small = torch.zeros((2,) + shp(8, 8), dtype=_torch_dtype(dtype)), torch.zeros((4,) + shp(3, 2), dtype=_torch_dtype(dtype))
            outs = [big[0], big[1]] + [small[k] for k in range(4)]
            back = tensors.load_views(paths, views, [(8, 8)] * 2 + [(3, 2)] * 4, out=outs, **kw)
            assert all(b is o for b, o in zip(back, outs))
            for v, (i, rect, flip) in enumerate(views):
                oh, ow = (8, 8) if v < 2 else (3, 2)
                z = (Resampled if aa else Resized)(want[i], rect, flip, oh, ow).bits(word, dtype, scale, bias)
                assert np.array_equal(_bits((big if v < 2 else small)[v if v < 2 else v - 2], dtype), z), ("out", v)
    # channels None keeps each file's count
    g = tensors.load_views(paths, [(2, None, False)], (4, 3), device="cpu", dtype=torch.float32)[0]
    assert tuple(g.shape) == (3, 4, 3)
    # misuse: every one names the offender
    f16 = dict(device="cpu", dtype=torch.float16)
    o1 = [torch.zeros((3, 4, 4), dtype=torch.float16)]
    for words, args, kw in [
            (["view 0", "path 4"], ([(4, None, False)], (4, 4)), f16),
            (["view 1", "path -1"], ([(0, None, False), (-1, None, False)], (4, 4)), f16),
            (["view 0", "(0, 0, 26, 1)", "25 x 37"], ([(0, (0, 0, 26, 1), False)], (4, 4)), f16),
            (["view 0", "(0, 0, 0, 1)"], ([(0, (0, 0, 0, 1), False)], (4, 4)), f16),
            (["rectangle of view 0"], ([(0, (0, 0, 1), False)], (4, 4)), f16),
            (["a view is"], ([(0, None)], (4, 4)), f16),
            (["empty"], ([], (4, 4)), f16),
            (["2 sizes", "1 views"], ([(0, None, False)], [(4, 4), (5, 5)]), f16),
            (["size", "(0, 4)", "view 0"], ([(0, None, False)], (0, 4)), f16),
            (["size", "16385"], ([(0, None, False)], [(4, 16385)]), f16),
            (["size must be"], ([(0, None, False)], 7), f16),
            (["dtype"], ([(0, None, False)], (4, 4)), dict(device="cpu", dtype=torch.uint8)),
            (["layout"], ([(0, None, False)], (4, 4)), dict(layout="nchw", **f16)),
            (["channels"], ([(0, None, False)], (4, 4)), dict(channels=5, **f16)),
            (["stack", "view 1"], ([(0, None, False), (0, None, False)], [(4, 4), (4, 5)]), dict(stack=True, **f16)),
            (["stack", "out"], ([(0, None, False)], (4, 4)), dict(stack=True, out=o1, **f16)),
            (["out has 1", "2 views"], ([(0, None, False), (0, None, False)], (4, 4)), dict(out=o1, **f16)),
            (["out[0]", "shape"], ([(0, None, False)], (4, 5)), dict(out=o1, **f16)),
            (["out[0]", "dtype"], ([(0, None, False)], (4, 4)), dict(out=[torch.zeros((3, 4, 4))], **f16)),
            (["out[0]", "contiguous"], ([(0, None, False)], (4, 4)), dict(out=[torch.zeros((3, 4, 8), dtype=torch.float16)[:, :, ::2]], **f16)),
            (["out[0]", "not a tensor"], ([(0, None, False)], (4, 4)), dict(out=[None], **f16)),
            (["std"], ([(0, None, False)], (4, 4)), dict(std=0.0, **f16)),
            (["cannot read"], ([(3, None, False)], (4, 4)), f16)]:
        with pytest.raises(api.XpngError) as e:
            tensors.load_views(paths, *args, **kw)
        assert all(w in str(e.value) for w in words), (words, str(e.value))
    assert float(o1[0].abs().sum()) == 0.0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): the rasters of DIMS and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "photo"]
    out = {}
    for mode, alpha in FORMATS:
        rasters = [synth_raster(kinds[(i + 1) % 4], w, h, alpha, seed=i + 11) for i, (w, h) in enumerate(DIMS)]
        out[(mode, alpha)] = (rasters, [po.encode_tiles(mode, r) for r in rasters])
    return out


_CHECK = {}


def checked(key, raster, rect, flip, OW, OH, filter=AA):
    """the checker's v for (raster, rectangle, flip, size, filter), computed once for all layout words and dtypes"""
    k = (key, rect, bool(flip), OW, OH, filter)
    if k not in _CHECK:
        _CHECK[k] = (Resampled if filter == AA else Resized)(raster, rect, bool(flip), OH, OW)
    return _CHECK[k]


def run_views(ctx, mode, d_b, lens, views, word, dtype, scale, bias, filter=AA, offs=None, expect_status=0):
    """the views' elements as bit patterns, flat, out of a sentinel-filled arena whose every other byte is checked"""
    ch = api.layout_channels(word, ctx.pxsz)
    vi, rects, flips, sizes = view_args(views)
    ar = Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
    ctx.decode_batch_views(mode, [t.data_ptr() for t in d_b], lens, vi, ar.ptrs, word, dtype, sizes, scale[:ch], bias[:ch], rects=rects, flips=flips,
                           filter=filter, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return [g.view(BITS[dtype]) for g in ar.fetch()]


def assert_geometry(ctx):
    """the boundaries the rectangles of VIEWS rely on, from the context's own table"""
    assert ctx.n_tiles == 11 and ctx.first_tile == [0, 4, 7, 9, 10, 11]
    assert [ctx.tile(t) for t in range(4)] == [(0, 0, 445, 445), (445, 0, 444, 445), (0, 445, 445, 444), (445, 445, 444, 444)]
    assert [ctx.tile(t) for t in range(4, 7)] == [(0, 0, 445, 445), (445, 0, 444, 445), (889, 0, 444, 445)]
    assert [ctx.tile(t) for t in (7, 8)] == [(0, 0, 200, 1015), (0, 1015, 200, 985)]
    assert ctx.tile(9) == (0, 0, 300, 200) and ctx.tile(10) == (0, 0, 64, 70)


@pytest.mark.gpu
def test_one_view_in_one_tile_of_a_two_tile_image(gpu, po):
    """The smallest partial list on a mixed context: the lower tile of a 200 x 2000 image alone."""
    from xpng_amd.synth import synth_raster
    r = synth_raster("photo", 200, 2000, False, seed=5)
    blob = po.encode_tiles(1, r)
    ctx = gpu.MixedContext([(200, 2000)], 3)
    try:
        assert ctx.n_tiles == 2 and ctx.tile(1) == (0, 1015, 200, 985) and ctx.last_decode_tiles() == 0
        views = [(0, (0, 1100, 200, 800), 0, (37, 29))]
        word = api.layout(planar=True, channels=3)
        scale, bias = mixed_consts(F16)
        got = run_views(ctx, 1, _upload([blob]), [len(blob)], views, word, F16, scale, bias)
        assert ctx.last_decode_tiles() == 1 and api.view_tiles([(200, 2000)], [0], [views[0][1]]) == [1]
        assert np.array_equal(got[0], Resampled(r, views[0][1], False, 29, 37).bits(word, F16, scale, bias).reshape(-1))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_bits(gpu, batches, mode, alpha, dtype):
    """Every view equals the checker and api.resample_host on the bits, every sentinel is intact, and the launch held exactly the
    tiles of api.view_tiles - fewer than M, more than none - for a planar BGR word with C != pxsz, the file's own interleaved form
    and an interleaved BGR word, both filters and both size walks."""
    rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    vi, rects, flips, sizes = view_args(VIEWS)
    sel = api.view_tiles(DIMS, vi, rects)
    ctx = gpu.MixedContext(DIMS, px)
    try:
        assert_geometry(ctx)
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word in (api.layout(planar=True, bgr=True, channels=7 - px), api.layout(), api.layout(bgr=True, channels=7 - px)):
            ch = api.layout_channels(word, px)
            for filt in (AA, BIL):
                for offs in (None, _offsets(blobs, ctx)):
                    got = run_views(ctx, mode, d_b, lens, VIEWS, word, dtype, scale, bias, filter=filt, offs=offs)
                    assert ctx.last_decode_tiles() == len(sel) and 0 < len(sel) < ctx.n_tiles and len(sel) == SELECTED
                    for v, (i, rect, flip, (OW, OH)) in enumerate(VIEWS):
                        w = checked((mode, alpha, i), rasters[i], rect, flip, OW, OH, filt).bits(word, dtype, scale, bias).reshape(-1)
                        assert np.array_equal(got[v], w), (hex(word), dtype, filt, offs is None, v, np.argwhere(got[v] != w)[:4].ravel())
                        if offs is None:
                            host = api.resample_host(rasters[i], (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=filt)
                            assert np.array_equal(got[v], np.frombuffer(host, BITS[dtype])), ("host twin", hex(word), dtype, filt, v)
        # another mixed call afterwards launches every tile again
        full = Arena([ES[dtype] * px * w * h for (w, h) in DIMS], ES[dtype])
        ctx.decode_batch_as_float(mode, [t.data_ptr() for t in d_b], lens, full.ptrs, api.layout(), dtype, scale[:px], bias[:px])
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == ctx.n_tiles
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [BIL, AA])
def test_identity_views_equal_the_resampled_call(gpu, batches, filt):
    """view_image NULL and one size: bit for bit what decode_batch_resampled gives on the same context."""
    rasters, blobs = batches[(1, True)]
    rects = [(400, 100, 80, 300), (0, 0, 1333, 445), (5, 900, 190, 300), (0, 0, 300, 200), (10, 10, 20, 30)]
    flips = [1, 0, 1, 0, 1]
    OW, OH = 37, 29
    word, dtype = api.layout(planar=True, channels=3), F16
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(DIMS, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        a, b = (Arena([2 * 3 * OW * OH] * 5, 2) for _ in range(2))
        ctx.decode_batch_resampled(1, ins, lens, a.ptrs, word, dtype, (OH, OW), scale[:3], bias[:3], rects=rects, flips=flips, filter=filt)
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == ctx.n_tiles
        ctx.decode_batch_views(1, ins, lens, None, b.ptrs, word, dtype, (OH, OW), scale[:3], bias[:3], rects=rects, flips=flips, filter=filt)
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == len(api.view_tiles(DIMS, None, rects)) < ctx.n_tiles
        for i, (x, y) in enumerate(zip(a.fetch(), b.fetch())):
            assert np.array_equal(x, y), (filt, i)
        # NULL rects and flips too: whole images, every tile
        a.refill(), b.refill()
        ctx.decode_batch_resampled(1, ins, lens, a.ptrs, word, dtype, (OH, OW), scale[:3], bias[:3], filter=filt)
        ctx.decode_batch_views(1, ins, lens, None, b.ptrs, word, dtype, (OH, OW), scale[:3], bias[:3], filter=filt)
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == ctx.n_tiles
        for i, (x, y) in enumerate(zip(a.fetch(), b.fetch())):
            assert np.array_equal(x, y), ("whole", filt, i)
    finally:
        ctx.close()


def _corrupt(blobs, offs, image, tile):
    bad = bytearray(blobs[image])
    bad[offs[image][tile] + 3] = 0x7F                              # top byte of the tile's first little-endian word
    return blobs[:image] + [bytes(bad)] + blobs[image + 1:]


@pytest.mark.gpu
def test_skipping_is_real(gpu, batches):
    """Tile 2 of image 0, which no view touches, gets type byte 0x7F: the views call reports 0 and every view is exact, while
    decode_batch_resampled on the same blobs and rectangles reports 1.  Then tile 1, which view 1 touches: status 1, every element
    of view 1 with no tap in that tile exact, every other view exact."""
    rasters, blobs = batches[(1, True)]
    word, dtype = api.layout(planar=True, channels=3), F16
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(DIMS, 4)
    try:
        assert_geometry(ctx)
        offs = _offsets(blobs, ctx)
        bb = _corrupt(blobs, offs, 0, 2)
        d_b, lens = _upload(bb), [len(b) for b in bb]
        want = [checked((1, True, i), rasters[i], rect, flip, OW, OH).bits(word, dtype, scale, bias) for (i, rect, flip, (OW, OH)) in VIEWS]
        got = run_views(ctx, 1, d_b, lens, VIEWS, word, dtype, scale, bias, expect_status=0)
        for v, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w.reshape(-1)), v
        rects = [(400, 100, 80, 300), (900, 10, 400, 400), (0, 1100, 200, 800), (0, 0, 300, 200), (0, 0, 64, 70)]   # tile 2 of image 0 untouched here too
        ar = Arena([2 * 3 * 37 * 29] * 5, 2)
        ctx.decode_batch_resampled(1, [t.data_ptr() for t in d_b], lens, ar.ptrs, word, dtype, (29, 37), scale[:3], bias[:3], rects=rects)
        assert ctx.decode_status() == 1                            # that call validates, and reconstructs, every tile
        bb = _corrupt(blobs, offs, 0, 1)
        got = run_views(ctx, 1, _upload(bb), [len(b) for b in bb], VIEWS, word, dtype, scale, bias, expect_status=1)
        tx, ty, tw, th = ctx.tile(1)
        for v, (g, w) in enumerate(zip(got, want)):
            g = g.reshape(w.shape)
            if v != 1:
                assert np.array_equal(g, w), v
                continue
            i, rect, flip, (OW, OH) = VIEWS[v]
            xa, xb, ya, yb = checked((1, True, i), rasters[i], rect, flip, OW, OH).span     # relative to the rectangle, inclusive
            hitx = (rect[0] + xb >= tx) & (rect[0] + xa < tx + tw)
            hity = (rect[1] + yb >= ty) & (rect[1] + ya < ty + th)
            hit = hity[:, None] & hitx[None, :]
            assert hit.any() and not hit.all() and int((~hit).sum()) > 100
            assert np.array_equal(g[:, ~hit], w[:, ~hit])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_stale_staging_is_never_read_and_cached_records_survive(gpu, po):
    """decode_batch_as_float on batch A, then a views call on batch B = 255 - A whose rectangles end and start exactly on tile
    boundaries - the tiles beside them still hold A's pixels in the staging raster - then decode_batch_as_float on A again with the
    pointers it had."""
    from xpng_amd.synth import synth_raster
    dims = [(889, 889), (64, 70)]
    A = [synth_raster("photo", w, h, False, seed=i + 70) for i, (w, h) in enumerate(dims)]
    B = [255 - r for r in A]
    ba, bb = [po.encode_tiles(1, r) for r in A], [po.encode_tiles(1, r) for r in B]
    word, dtype = api.layout(planar=True, channels=3), F16
    scale, bias = mixed_consts(dtype)
    tab = table(dtype, scale[:3], bias[:3])
    views = [(0, (0, 0, 445, 445), 0, (37, 29)), (0, (445, 445, 444, 444), 1, (96, 64)), (0, (100, 445, 345, 444), 0, (3, 5)), (1, (0, 0, 64, 70), 1, (37, 29))]
    ctx = gpu.MixedContext(dims, 3)
    try:
        assert ctx.tile(0) == (0, 0, 445, 445) and ctx.tile(3) == (445, 445, 444, 444)
        da, db = _upload(ba), _upload(bb)
        full = Arena([2 * 3 * w * h for (w, h) in dims], 2)
        ins = [t.data_ptr() for t in da]
        ctx.decode_batch_as_float(1, ins, [len(b) for b in ba], full.ptrs, word, dtype, scale[:3], bias[:3])
        assert ctx.decode_status() == 0
        first = [g.view(np.uint16).copy() for g in full.fetch()]
        for g, r in zip(first, A):
            assert np.array_equal(g, expect(r, True, False, 3, tab).reshape(-1))
        got = run_views(ctx, 1, db, [len(b) for b in bb], views, word, dtype, scale, bias)
        assert ctx.last_decode_tiles() == 4                        # tiles 0, 2 and 3 of image 0 and the one of image 1
        for v, (i, rect, flip, (OW, OH)) in enumerate(views):
            assert np.array_equal(got[v], Resampled(B[i], rect, bool(flip), OH, OW).bits(word, dtype, scale, bias).reshape(-1)), v
        full.refill()
        ctx.decode_batch_as_float(1, ins, [len(b) for b in ba], full.ptrs, word, dtype, scale[:3], bias[:3])
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == ctx.n_tiles
        for g, f in zip(full.fetch(), first):
            assert np.array_equal(g.view(np.uint16), f)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_views_workspace(gpu, batches):
    """The workspace grows by the record table (64 bytes per view) and the list (4 bytes per tile of the table), once; fewer views
    with other rectangles and sizes grow nothing; more views grow it by the records' difference."""
    rasters, blobs = batches[(1, False)]
    word, dtype = api.layout(planar=True, channels=3), F16
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(DIMS, 3)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        full = Arena([2 * 3 * w * h for (w, h) in DIMS], 2)
        ctx.decode_batch_as_float(1, [t.data_ptr() for t in d_b], lens, full.ptrs, word, dtype, scale[:3], bias[:3])
        assert ctx.decode_status() == 0
        ws = ctx.workspace_bytes()
        run_views(ctx, 1, d_b, lens, VIEWS[:4], word, dtype, scale, bias)
        assert ctx.workspace_bytes() - ws == 64 * 4 + 4 * ctx.n_tiles
        other = [(3, (0, 0, 300, 200), 1, (5, 3)), (0, (0, 0, 889, 889), 0, (11, 7)), (4, (1, 1, 2, 2), 0, (4, 4))]
        got = run_views(ctx, 1, d_b, lens, other, word, dtype, scale, bias)
        assert ctx.workspace_bytes() - ws == 64 * 4 + 4 * ctx.n_tiles and ctx.last_decode_tiles() == 6
        for v, (i, rect, flip, (OW, OH)) in enumerate(other):
            assert np.array_equal(got[v], Resampled(rasters[i], rect, bool(flip), OH, OW).bits(word, dtype, scale, bias).reshape(-1)), v
        seven = VIEWS + [(3, (10, 10, 100, 100), 0, (3, 5))]
        got = run_views(ctx, 1, d_b, lens, seven, word, dtype, scale, bias)
        assert ctx.workspace_bytes() - ws == 64 * 7 + 4 * ctx.n_tiles and ctx.last_decode_tiles() == 7
        for v, (i, rect, flip, (OW, OH)) in enumerate(seven):
            assert np.array_equal(got[v], checked((1, False, i), rasters[i], rect, flip, OW, OH).bits(word, dtype, scale, bias).reshape(-1)), v
        run_views(ctx, 1, d_b, lens, VIEWS, word, dtype, scale, bias)
        assert ctx.workspace_bytes() - ws == 64 * 7 + 4 * ctx.n_tiles
    finally:
        ctx.close()


@pytest.mark.gpu
def test_misuse_of_the_views_call(gpu, batches):
    """Every refusal names its value and leaves every byte of the arena as it was."""
    rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, channels=3)
    vi, rects, flips, sizes = view_args(VIEWS)
    scale, bias = mixed_consts(F16)
    ctx = gpu.MixedContext(DIMS, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * oh * ow for (oh, ow) in sizes], 4)

        def refused(words, **kw):
            a = dict(mode=1, d_blobs=ins, lens=lens, view_image=vi, d_outs=outs.ptrs, layout=word, dtype=F16, sizes=sizes, scale=scale[:3], bias=bias[:3],
                     rects=rects, flips=flips, filter=AA)
            a.update(kw)
            with pytest.raises(gpu.XpngError) as e:
                ctx.decode_batch_views(**a)
            assert all(w in str(e.value) for w in words), (words, str(e.value))
            assert outs.untouched(), words

        refused(["view_image[2]", "is 5", "5 images"], view_image=vi[:2] + [5] + vi[3:])
        refused(["view_image is NULL", "nviews is 6", "nimg 5"], view_image=None)
        refused(["{500, 500, 300, 400}", "view 0", "image 0", "889 x 889"], rects=[(500, 500, 300, 400)] + rects[1:])
        refused(["{0, 0, 0, 5}", "view 3", "image 2"], rects=rects[:3] + [(0, 0, 0, 5)] + rects[4:])
        refused(["{0, 0, 65, 70}", "view 4", "image 4", "64 x 70"], rects=rects[:4] + [(0, 0, 65, 70)] + rects[5:])
        refused(["37 x 0", "view 0"], sizes=[(0, 37)] + sizes[1:])
        refused(["16385 x 29", "view 5"], sizes=sizes[:5] + [(29, 16385)])
        refused(["flip 2", "view 1"], flips=[0, 2, 0, 1, 0, 1])
        refused(["filter 2", "XPNGHIP_FILTER_TRIANGLE_AA"], filter=2)
        refused(["out_sizes is NULL"], sizes=None)
        refused(["null", "view 1"], d_outs=[outs.ptrs[0], 0] + outs.ptrs[2:])
        odd = [outs.ptrs[0], outs.ptrs[1] + 1] + outs.ptrs[2:]
        refused(["aligned", "%x" % odd[1], "view 1"], d_outs=odd)
        refused(["dtype 0"], dtype=0)
        refused(["dtype 4"], dtype=4)
        refused(["layout", "0x500"], layout=0x500)
        refused(["scale[1]", "nan"], scale=[1.0, float("nan"), 1.0])
        refused(["bias[0]", "inf"], bias=[float("inf"), 0.0, 0.0])
        refused(["nimg is 2"], d_blobs=ins[:2], lens=lens[:2])
        refused(["mode 2", "RGB"], mode=2)
        refused(["tile mode"], mode=3)
        refused(["null blob", "image 1"], d_blobs=[ins[0], 0] + ins[2:])
        # nviews outside 1 .. 65535, a NULL context and a context that is not mixed, through the raw entry point
        lib = api.hip_lib()
        p1, n1, s1 = (C.c_void_p * 1)(outs.ptrs[0]), (C.c_uint64 * 5)(*lens), (C.c_uint32 * 2)(4, 4)
        b5 = (C.c_void_p * 5)(*ins)
        assert lib.xpnghip_decode_varsize_device_batch_views(ctx._h, 1, b5, n1, 5, None, 0, (C.c_uint32 * 1)(0), p1, s1, None, None, word, F16, None, None, AA, None) != 0
        assert "nviews is 0" in api._err()
        assert lib.xpnghip_decode_varsize_device_batch_views(ctx._h, 1, b5, n1, 5, None, 65536, (C.c_uint32 * 1)(0), p1, s1, None, None, word, F16, None, None, AA, None) != 0
        assert "nviews is 65536" in api._err() and "65535" in api._err()
        assert lib.xpnghip_decode_varsize_device_batch_views(None, 1, b5, n1, 5, None, 1, (C.c_uint32 * 1)(0), p1, s1, None, None, word, F16, None, None, AA, None) != 0
        assert "null context" in api._err()
        one = gpu.Context(64, 64, 4)
        try:
            assert lib.xpnghip_decode_varsize_device_batch_views(one._h, 1, b5, n1, 1, None, 1, (C.c_uint32 * 1)(0), p1, s1, None, None, word, F16, None, None, AA, None) != 0
            assert "not a mixed context" in api._err()
        finally:
            one.close()
        assert outs.untouched()
        # the context still works after all that
        got = run_views(ctx, 1, d_b, lens, VIEWS, word, F16, scale, bias)
        for v, (i, rect, flip, (OW, OH)) in enumerate(VIEWS):
            assert np.array_equal(got[v], checked((1, True, i), rasters[i], rect, flip, OW, OH).bits(word, F16, scale, bias).reshape(-1)), v
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_views_on_goldens(gpu):
    """Two views per reference-written file and one file without a view, written through out= into slices of two stacked tensors
    of different sizes: every view equals api.resample_host of api.load of its file."""
    import torch
    from xpng_amd import tensors
    paths = sorted(p for p in glob.glob(os.path.join(GOLD, "imgfull_*.xpng")) if 11 < os.path.getsize(p) < 200000)[:6]
    assert len(paths) == 6
    want = [gpu.load(p) for p in paths]
    assert len({r.shape for r in want}) >= 2
    dims = [(r.shape[1], r.shape[0]) for r in want]
    g = torch.Generator().manual_seed(20)
    used = [0, 1, 2, 3, 5]                                          # file 4 has no view
    big_r = tensors.random_resized_crops([dims[i] for i in used], generator=g)
    small_r = tensors.random_resized_crops([dims[i] for i in used], scale=(0.05, 0.14), generator=g)
    views = [(i, r, k % 2 == 1) for k, (i, r) in enumerate(zip(used, big_r))] + [(i, r, k % 2 == 0) for k, (i, r) in enumerate(zip(used, small_r))]
    views[0] = (views[0][0], None, False)
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    for lay, bgr, dtype in (("chw", False, F16), ("hwc", True, F32)):
        shp = lambda oh, ow: (3, oh, ow) if lay == "chw" else (oh, ow, 3)   # noqa: E731
        big = torch.zeros((5,) + shp(32, 48), dtype=_torch_dtype(dtype), device="cuda")
        small = torch.zeros((5,) + shp(12, 12), dtype=_torch_dtype(dtype), device="cuda")
        outs = list(big.unbind(0)) + list(small.unbind(0))
        back = tensors.load_views(paths, views, [(32, 48)] * 5 + [(12, 12)] * 5, layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype),
                                  mean=IMAGENET_MEAN, std=IMAGENET_STD, out=outs)
        assert all(b is o for b, o in zip(back, outs))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for v, (i, rect, flip) in enumerate(views):
            oh, ow = (32, 48) if v < 5 else (12, 12)
            raw = api.resample_host(want[i], (oh, ow), word, dtype, scale, bias, rect=rect, flip=flip)
            t = (big if v < 5 else small)[v % 5]
            assert np.array_equal(_bits(t, dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (lay, v, paths[i], rect)
    lst = tensors.load_views(paths, views[:3], (8, 9), channels=3, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, stack=True, antialias=False)
    assert tuple(lst.shape) == (3, 3, 8, 9) and lst.is_cuda
    for v, (i, rect, flip) in enumerate(views[:3]):
        raw = api.resample_host(want[i], (8, 9), api.layout(planar=True, channels=3), F16, scale, bias, rect=rect, flip=flip, filter=BIL)
        assert np.array_equal(_bits(lst[v], F16).reshape(-1), np.frombuffer(raw, BITS[F16])), v
