"""A colour matrix per view in the copy-out of a views decode (include/xpng_hip.h xpnghip_resample_colour_host,
xpnghip_decode_varsize_device_batch_views_colour; xpng_amd/tensors.py load_views(colour=), colour_matrix, compose_colour,
random_colour_jitter).

Every comparison with the library is on the bits.  CPU: the symbols; xpnghip_resample_colour_host against a restatement written
here - api.resample_host into interleaved f32 with scale 1 and bias 0 gives the exact v of the resample rule, then the three
nested fmaf of tests/_resize.py (libm through ctypes, never float64), the clamp, the constants and the narrowing of
tests/_resize.py - consequence (d), the refusals, the matrix helpers, and load_views(colour=) on the host-answered kinds with
device="cpu".  GPU (-m gpu): the smallest case first; the bits of every view for three formats, three layout words, three dtypes
and both filters against the host rule, in sentinel arenas at every alignment; colours None; the workspace; the count of decoded
tiles; misuse; load_views on goldens with random_colour_jitter."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _resize
from _kit import (BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _torch_dtype, _upload, built, consts_from,
                  declared, exported, gpu, mixed_consts, po)
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_resample_colour_host", "xpnghip_decode_varsize_device_batch_views_colour"]
AA, BIL = api.FILTER_TRIANGLE_AA, api.FILTER_BILINEAR
f32 = np.float32

IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
PERM = [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0]                       # R <- B, G <- R, B <- G: not symmetric, so a transposed index shows
GRAY = [0.299, 0.587, 0.114, 0] * 3
RANGE = [3, -2, 0.5, -300, -2, 3, 0, 300, 1, 1, -2, 40]            # drives values below 0 and above 255
DENSE = [0.70710678, -0.31830989, 0.57721566, 12.345678, 0.14142135, 1.6180339, -0.69314718, -7.3890561, -0.43429448, 0.26179939, 1.2020569,
         31.415926]
MATS = [IDENT, PERM, GRAY, RANGE, DENSE]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def triple(raster, rect, flip, OH, OW, filt, m):
    """t of the rule for R, G, B (and the resampled alpha, or None) as (OH, OW) float32 arrays"""
    px = raster.shape[2]
    raw = api.resample_host(raster, (OH, OW), api.layout(channels=px), F32, [1.0] * px, [0.0] * px, rect=rect, flip=flip, filter=filt)
    v = np.frombuffer(raw, np.float32).reshape(OH, OW, px)            # fmaf(v, 1, 0) is v: the exact values of the resample rule
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    t = []
    for k in range(3):
        x = _resize.fmaf(m[k][0], v[..., 0], _resize.fmaf(m[k][1], v[..., 1], _resize.fmaf(m[k][2], v[..., 2], m[k][3])))
        t.append(np.where(x < 0, f32(0), np.where(x > 255, f32(255), x)).astype(f32))
    return t, (v[..., 3] if px == 4 else None)


def restated_bits(t, alpha, OH, OW, word, dtype, scale, bias, px, cache):
    """the caller's buffer as bit patterns; `cache` keeps y per (source, scale, bias) for the layout words and dtypes of one t"""
    planar, bgr, ch = bool(word & 1), bool(word & 2), (word >> 8) or px
    ys = []
    for c in range(ch):
        k = 3 if c == 3 else 2 - c if bgr else c
        key = (k, float(scale[c]), float(bias[c]))
        if key not in cache:
            u = t[k] if k < 3 else alpha if alpha is not None else np.full((OH, OW), f32(255))
            cache[key] = _resize.fmaf(u, f32(scale[c]), f32(bias[c]))
        ys.append(cache[key])
    return _resize.narrow(np.stack(ys, axis=0 if planar else 2), dtype).reshape(-1)


@pytest.fixture(scope="module")
def small():
    from xpng_amd.synth import synth_raster
    return {3: synth_raster("photo", 64, 70, False, seed=3), 4: synth_raster("noise", 64, 70, True, seed=4)}


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_colour_symbols_are_declared_listed_and_exported():
    assert set(NEW) <= set(declared("xpng_hip.h", "xpnghip_")) and set(NEW) <= set(api.HIP_SYMBOLS) and set(NEW) <= exported(api.HIP_SO)
    txt = open(os.path.join(ROOT, "include", "xpng_hip.h")).read()
    assert re.search(r"48 bytes per view", txt) and "64-byte record per view" in txt
    assert api.hip_lib().xpnghip_abi_version() == 2
    import xpng_amd
    from xpng_amd import tensors
    assert "resample_colour_host" in xpng_amd.__all__ and callable(xpng_amd.resample_colour_host)
    for name in ("colour_matrix", "compose_colour", "random_colour_jitter"):
        assert callable(getattr(tensors, name))


def _words(px):
    out = []
    for ch in (3, 4):
        for planar in (False, True):
            for bgr in (False, True):
                out.append(api.layout(planar=planar, bgr=bgr, channels=ch))
    return out


def test_resample_colour_host_equals_the_restatement(small):
    # (rect, (OH, OW)): odd origins.  The small sizes run every matrix with both flips and filters.  The big size (21504 pixels through
    # libm one by one) runs both flips and filters with the permutation, and beside it one of the other four matrices per
    # (filter, flip), so each of the five is checked there for both pixel sizes
    shapes = [((3, 5, 51, 33), (37, 5)), ((7, 1, 40, 69), (1, 1)), ((1, 3, 63, 67), (224, 96))]
    n = 0
    for px in (3, 4):
        ras = small[px]
        for s, (rect, (OH, OW)) in enumerate(shapes):
            for filt in (BIL, AA):
                for flip in (False, True):
                    mats = MATS if OH * OW < 1000 else [PERM, (IDENT, GRAY, RANGE, DENSE)[2 * filt + flip]]
                    for mi, m in enumerate(mats):
                        t, alpha = triple(ras, rect, flip, OH, OW, filt, m)
                        cache = {}
                        for dtype in DTYPES:
                            scale, bias = mixed_consts(dtype)
                            for word in _words(px):
                                ch = api.layout_channels(word, px)
                                got = api.resample_colour_host(ras, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=filt, colour=m)
                                want = restated_bits(t, alpha, OH, OW, word, dtype, scale, bias, px, cache)
                                assert np.array_equal(np.frombuffer(got, BITS[dtype]), want), (px, rect, OH, OW, filt, flip, mi, dtype, hex(word))
                                n += 1
    assert n > 1000
    # the matrix as a (3, 4) array and as 12 numbers are the same call; None is resample_host
    a = api.resample_colour_host(small[3], (5, 7), api.layout(), F32, colour=np.asarray(DENSE).reshape(3, 4))
    assert a == api.resample_colour_host(small[3], (5, 7), api.layout(), F32, colour=DENSE)
    assert api.resample_colour_host(small[4], (5, 7), api.layout(), F16, colour=None) == api.resample_host(small[4], (5, 7), api.layout(), F16)


def test_identity_equals_null_with_filter_0(small):
    """consequence (d)"""
    for px in (3, 4):
        for word in _words(px):
            for dtype in DTYPES:
                ch = api.layout_channels(word, px)
                scale, bias = mixed_consts(dtype)
                for rect, size, flip in (((3, 5, 51, 33), (5, 37), True), (None, (96, 224), False), ((1, 1, 62, 68), (9, 11), False)):
                    a = api.resample_colour_host(small[px], size, word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=BIL, colour=IDENT)
                    b = api.resample_host(small[px], size, word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=BIL)
                    assert a == b, (px, hex(word), dtype, rect)


def test_resample_colour_host_refusals_write_nothing(small):
    lib = api.hip_lib()
    ras = small[3]
    out = np.full(3 * 4 * 4, 0xA5A5A5A5, np.uint32)

    def raw(m, filt=AA, ow=4, oh=4):
        cm = (C.c_float * 12)(*m)
        return lib.xpnghip_resample_colour_host(3, ras.ctypes.data, 64, 70, None, 0, ow, oh, api.layout(), F32, None, None, filt, cm, out.ctypes.data)

    for e, bad, word in ((5, float("nan"), "nan"), (11, float("inf"), "inf"), (2, -float("inf"), "inf"), (6, 65537.0, "65537"), (3, -65536.5, "65536")):
        m = list(DENSE)
        m[e] = bad
        assert raw(m) != 0
        msg = api._err()
        assert "[%d][%d]" % (e // 4, e % 4) in msg and word in msg and "colour" in msg, msg
        assert (out == 0xA5A5A5A5).all()
        with pytest.raises(api.XpngError) as ex:
            api.resample_colour_host(ras, (4, 4), api.layout(), F32, colour=m)
        assert "[%d][%d]" % (e // 4, e % 4) in str(ex.value)
    # the bound itself is allowed; what resample_host refuses is refused with a matrix too
    m = list(IDENT)
    m[3], m[4] = 65536.0, -65536.0
    assert raw(m) == 0 and not (out == 0xA5A5A5A5).any()
    out[:] = 0xA5A5A5A5
    assert raw(IDENT, filt=2) != 0 and "filter 2" in api._err()
    assert raw(IDENT, ow=0) != 0 and (out == 0xA5A5A5A5).all()
    for bad in ([1.0] * 11, np.zeros((4, 3)), "gray", [[1, 2], [3, 4]]):
        with pytest.raises(api.XpngError) as ex:
            api.resample_colour_host(ras, (4, 4), api.layout(), F32, colour=bad)
        assert "colour matrix" in str(ex.value)


def test_colour_matrix_and_compose():
    from xpng_amd import tensors as T
    eye = np.asarray(IDENT, np.float32).reshape(3, 4)
    m = T.colour_matrix()
    assert m.dtype == np.float32 and m.shape == (3, 4) and np.array_equal(m, eye)
    assert np.array_equal(T.colour_matrix(1.0, 1.0, 1.0, 0.0), eye)
    assert np.abs(T.colour_matrix(hue=1.0 / 3.0) - np.asarray(PERM, np.float32).reshape(3, 4)).max() < 1e-6
    g = T.colour_matrix(saturation=0.0)
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[1], g[2]) and np.array_equal(g[0], np.asarray([0.299, 0.587, 0.114, 0.0], np.float32))
    for c in (0.0, 0.6, 1.4, 3.0):
        k = T.colour_matrix(contrast=c).astype(np.float64)
        assert np.abs(k[:, :3] @ np.full(3, 127.5) + k[:, 3] - 127.5).max() < 1e-4
    b = T.colour_matrix(brightness=1.25)
    assert np.array_equal(b, np.asarray([1.25, 0, 0, 0, 0, 1.25, 0, 0, 0, 0, 1.25, 0], np.float32).reshape(3, 4))
    x, y, z = T.colour_matrix(1.2, 0.7, 1.3, 0.05), T.colour_matrix(0.8, 1.4, 0.2, -0.1), T.colour_matrix(1.0, 0.9, 0.0, 0.25)
    assert np.abs(T.compose_colour(T.compose_colour(x, y), z) - T.compose_colour(x, T.compose_colour(y, z))).max() < 1e-5   # the whole 3 x 4
    # b after a, on a pixel
    p = np.asarray([10.0, 200.0, 77.0, 1.0])
    ab = T.compose_colour(x, y).astype(np.float64)
    assert np.abs(ab @ p - (y.astype(np.float64) @ np.append(x.astype(np.float64) @ p, 1.0))).max() < 1e-3
    assert np.array_equal(T.compose_colour(eye, PERM), np.asarray(PERM, np.float32).reshape(3, 4))
    with pytest.raises(api.XpngError):
        T.compose_colour(eye, [1, 2, 3])


def test_random_colour_jitter():
    import torch
    from xpng_amd import tensors as T
    eye = np.asarray(IDENT, np.float32).reshape(3, 4)
    a = T.random_colour_jitter(16, generator=torch.Generator().manual_seed(7))
    b = T.random_colour_jitter(16, generator=torch.Generator().manual_seed(7))
    c = T.random_colour_jitter(16, generator=torch.Generator().manual_seed(8))
    assert len(a) == 16 and all(x.dtype == np.float32 and x.shape == (3, 4) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert len({x.tobytes() for x in a}) > 8                         # the views differ
    assert all(np.array_equal(x, eye) for x in T.random_colour_jitter(12, p=0.0, gray_p=0.0, generator=torch.Generator().manual_seed(1)))
    gray = T.colour_matrix(saturation=0.0)
    assert all(np.array_equal(x, eye) or np.array_equal(x, gray) for x in T.random_colour_jitter(12, p=0.0, generator=torch.Generator().manual_seed(1)))
    for x in T.random_colour_jitter(12, gray_p=1.0, generator=torch.Generator().manual_seed(2)):
        assert np.array_equal(x[0], x[1]) and np.array_equal(x[1], x[2])
    for x in T.random_colour_jitter(64, 0.8, 0.8, 0.8, 0.5, p=1.0, generator=torch.Generator().manual_seed(3)):
        assert np.isfinite(x).all() and np.abs(x).max() <= 65536
    assert T.random_colour_jitter(0) == []


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(25, 37, False), (39, 16, True)]:
        p = tmp_path / f"l7_{w}x{h}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if w > 30 else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_views_colour_answers_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(37, 25, 3), (1000, 1000, 3), (16, 39, 4)]
    views = [(0, (1, 2, 23, 34), True), (2, None, False), (0, None, False), (1, (100, 200, 300, 150), False), (2, (3, 1, 35, 5), True),
             (0, (23, 35, 1, 1), False)]
    sizes = [(6, 5), (3, 7), (40, 30), (2, 2), (9, 4), (1, 1)]     # (OH, OW): per-view sizes
    cols = [PERM, None, tensors.colour_matrix(1.3, 0.6, 0.2, 0.1), RANGE, np.asarray(DENSE).reshape(3, 4), GRAY]
    rule = [IDENT if m is None else m for m in cols]                 # beside a matrix, None is the identity matrix
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    for dtype in DTYPES:
        for ch, lay, bgr, aa in ((3, "chw", False, True), (4, "hwc", True, True), (3, "hwc", False, False)):
            scale, bias = consts_from(mean[:ch], std[:ch])
            word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
            filt = AA if aa else BIL
            kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch], antialias=aa)
            got = tensors.load_views(paths, views, sizes, colour=cols, **kw)
            plain = tensors.load_views(paths, views, sizes, **kw)
            differs = 0
            for v, ((i, rect, flip), (oh, ow), g) in enumerate(zip(views, sizes, got)):
                raw = api.resample_colour_host(want[i], (oh, ow), word, dtype, scale, bias, rect=rect, flip=flip, filter=filt, colour=rule[v])
                assert g.device.type == "cpu" and g.is_contiguous() and g.dtype == _torch_dtype(dtype)
                assert tuple(g.shape) == ((ch, oh, ow) if lay == "chw" else (oh, ow, ch))
                assert np.array_equal(_bits(g, dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (dtype, ch, lay, v)
                differs += not torch.equal(g, plain[v])
            assert differs >= 3                                       # the matrices did something
            if not aa:
                assert torch.equal(got[1], plain[1])                  # consequence (d): with filter 0 the identity is the plain view
            # all None and no argument are the same tensors
            for a, b in zip(tensors.load_views(paths, views, sizes, colour=[None] * len(views), **kw), plain):
                assert torch.equal(a, b)
            # stacked, and out= slices of two stacked tensors of different sizes
            whole = tensors.load_views(paths, views, (6, 5), stack=True, colour=cols, **kw)
            for v, (i, rect, flip) in enumerate(views):
                raw = api.resample_colour_host(want[i], (6, 5), word, dtype, scale, bias, rect=rect, flip=flip, filter=filt, colour=rule[v])
                assert np.array_equal(_bits(whole[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), ("stack", v)
            shp = lambda oh, ow: (ch, oh, ow) if lay == "chw" else (oh, ow, ch)   # noqa: E731
            big, sm = torch.zeros((2,) + shp(8, 8), dtype=_torch_dtype(dtype)), torch.zeros((4,) + shp(3, 2), dtype=_torch_dtype(dtype))
            outs = [big[0], big[1]] + [sm[k] for k in range(4)]
            back = tensors.load_views(paths, views, [(8, 8)] * 2 + [(3, 2)] * 4, out=outs, colour=cols, **kw)
            assert all(b is o for b, o in zip(back, outs))
            for v, (i, rect, flip) in enumerate(views):
                size = (8, 8) if v < 2 else (3, 2)
                raw = api.resample_colour_host(want[i], size, word, dtype, scale, bias, rect=rect, flip=flip, filter=filt, colour=rule[v])
                assert np.array_equal(_bits(outs[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), ("out", v)
    # misuse: the list's length, an entry's shape, an entry the library refuses
    f16 = dict(device="cpu", dtype=torch.float16)
    o1 = [torch.zeros((3, 4, 4), dtype=torch.float16)]
    nan = list(IDENT)
    nan[9] = float("nan")
    for words, col in ((["colour has 2 entries", "1 views"], [None, None]), (["colour[0]", "colour matrix"], [[1.0] * 9]),
                       (["colour[0]", "colour matrix"], [np.zeros((4, 3))]), (["[2][1]", "nan"], [nan])):
        with pytest.raises(api.XpngError) as e:
            tensors.load_views(paths, [(0, None, False)], (4, 4), out=o1, colour=col, **f16)
        assert all(w in str(e.value) for w in words), (words, str(e.value))
    assert float(o1[0].abs().sum()) == 0.0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# tests/test_views.py's shapes: the smallest with 2 x 2, 3 x 1 and 1 x 2 tile tables
DIMS = [(889, 889), (1333, 445), (200, 2000), (300, 200), (64, 70)]
# (image, rectangle, flip, (OW, OH)): three views of image 0 that leave its tile 2 alone, one of image 1, one of image 2, two of
# image 4, none of image 3.  Heights 224, 96, 5 and 1 in one call: the blocks of the short views exit.  224 x 224 and 96 x 96 planes
# are multiples of 16 bytes (the planar kernel's 16-byte stores into every plane), 37 x 5 and 1 x 1 are not (a pixel per lane).
VIEWS = [(0, (500, 500, 300, 300), 0, (224, 224)), (0, (400, 100, 80, 300), 1, (96, 96)), (0, (450, 50, 400, 380), 0, (37, 5)),
         (1, (900, 10, 400, 400), 0, (1, 1)), (2, (0, 1100, 200, 800), 1, (224, 224)), (4, (0, 0, 64, 70), 0, (96, 96)), (4, (10, 10, 20, 30), 1, (37, 5))]
COLS = [PERM, None, GRAY, RANGE, DENSE, IDENT, RANGE]
SELECTED = 6                                                      # of M = 11: tiles 0, 1, 3 of image 0, one each of images 1, 2 and 4


def view_args(views):
    return [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [(v[3][1], v[3][0]) for v in views]   # sizes as (OH, OW)


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


def run_views(ctx, mode, d_b, lens, views, word, dtype, scale, bias, filter=AA, colours=None, plain=False):
    """the views' elements as bit patterns, flat, out of a sentinel-filled arena whose every other byte is checked.  Buffer i starts
    i % 8 elements into its 16-byte aligned region, so heads of every length and the tails run."""
    ch = api.layout_channels(word, ctx.pxsz)
    vi, rects, flips, sizes = view_args(views)
    ar = Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
    kw = {} if plain else dict(colours=colours)
    ctx.decode_batch_views(mode, [t.data_ptr() for t in d_b], lens, vi, ar.ptrs, word, dtype, sizes, scale[:ch], bias[:ch], rects=rects, flips=flips,
                           filter=filter, **kw)
    assert ctx.decode_status() == 0
    return [g.view(BITS[dtype]) for g in ar.fetch()]


def host_rule(raster, view, col, word, dtype, scale, bias, filt, px):
    i, rect, flip, (OW, OH) = view
    ch = api.layout_channels(word, px)
    col = IDENT if col is None else col                                # beside a matrix, None is the identity matrix
    return np.frombuffer(api.resample_colour_host(raster, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=bool(flip), filter=filt, colour=col),
                         BITS[dtype])


@pytest.mark.gpu
def test_one_permuted_view_in_one_tile_of_a_two_tile_image(gpu, po):
    """The smallest case: the lower tile of a 200 x 2000 image alone, its colours permuted."""
    from xpng_amd.synth import synth_raster
    r = synth_raster("photo", 200, 2000, False, seed=5)
    blob = po.encode_tiles(1, r)
    ctx = gpu.MixedContext([(200, 2000)], 3)
    try:
        assert ctx.n_tiles == 2 and ctx.tile(1) == (0, 1015, 200, 985)
        views = [(0, (0, 1100, 200, 800), 0, (37, 29))]
        word = api.layout(planar=True, channels=3)
        scale, bias = mixed_consts(F16)
        d_b = _upload([blob])
        got = run_views(ctx, 1, d_b, [len(blob)], views, word, F16, scale, bias, colours=[PERM])
        assert ctx.last_decode_tiles() == 1
        assert np.array_equal(got[0], host_rule(r, views[0], PERM, word, F16, scale, bias, AA, 3))
        # a permutation of whole bytes: plane k of the permuted view is plane (k + 2) % 3 of the plain one
        plain = run_views(ctx, 1, d_b, [len(blob)], views, word, F16, [1.0] * 3, [0.0] * 3, filter=BIL, plain=True)[0].reshape(3, -1)
        perm = run_views(ctx, 1, d_b, [len(blob)], views, word, F16, [1.0] * 3, [0.0] * 3, filter=BIL, colours=[PERM])[0].reshape(3, -1)
        assert np.array_equal(perm, plain[[2, 0, 1]])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_colour_bits(gpu, batches, mode, alpha, dtype):
    """Every element of every view equals api.resample_colour_host with the view's matrix (None: the identity matrix) and every
    sentinel is intact, for a planar BGR word with C != pxsz, the file's own interleaved form and an interleaved BGR word, both
    filters; the launch held exactly the tiles of api.view_tiles."""
    rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    vi, rects, _, _ = view_args(VIEWS)
    sel = api.view_tiles(DIMS, vi, rects)
    ctx = gpu.MixedContext(DIMS, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word in (api.layout(planar=True, bgr=True, channels=7 - px), api.layout(), api.layout(bgr=True, channels=7 - px)):
            for filt in (AA, BIL):
                got = run_views(ctx, mode, d_b, lens, VIEWS, word, dtype, scale, bias, filter=filt, colours=COLS)
                assert ctx.last_decode_tiles() == len(sel) == SELECTED < ctx.n_tiles
                for v, view in enumerate(VIEWS):
                    w = host_rule(rasters[view[0]], view, COLS[v], word, dtype, scale, bias, filt, px)
                    assert np.array_equal(got[v], w), (hex(word), dtype, filt, v, np.argwhere(got[v] != w)[:4].ravel())
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [BIL, AA])
def test_no_colours_is_the_views_call(gpu, batches, filt):
    """colours None and a list of None are decode_batch_views on the bits, and the workspace does not grow by them."""
    rasters, blobs = batches[(1, True)]
    ctx = gpu.MixedContext(DIMS, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word, dtype in ((api.layout(planar=True, channels=3), F16), (api.layout(bgr=True), F32)):
            scale, bias = mixed_consts(dtype)
            base = run_views(ctx, 1, d_b, lens, VIEWS, word, dtype, scale, bias, filter=filt, plain=True)
            ws = ctx.workspace_bytes()
            for cols in (None, [None] * len(VIEWS)):
                got = run_views(ctx, 1, d_b, lens, VIEWS, word, dtype, scale, bias, filter=filt, colours=cols)
                assert all(np.array_equal(a, b) for a, b in zip(got, base)) and ctx.workspace_bytes() == ws
    finally:
        ctx.close()


@pytest.mark.gpu
def test_views_colour_workspace_and_the_other_tables(gpu, batches):
    """The first colour call grows the workspace by 48 bytes per view, once; as many or fewer views grow nothing; more views grow
    both tables.  A plain views call and a resampled call with their earlier pointers then give their earlier bytes."""
    rasters, blobs = batches[(1, False)]
    word, dtype = api.layout(planar=True, channels=3), F16
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(DIMS, 3)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        rs = Arena([2 * 3 * 37 * 29] * 5, 2)
        rrects = [(400, 100, 80, 300), (900, 10, 400, 400), (0, 1100, 200, 800), (0, 0, 300, 200), (0, 0, 64, 70)]
        ctx.decode_batch_resampled(1, ins, lens, rs.ptrs, word, dtype, (29, 37), scale[:3], bias[:3], rects=rrects, filter=AA)
        assert ctx.decode_status() == 0
        rs_first = [g.copy() for g in rs.fetch()]
        vi, rects, flips, sizes = view_args(VIEWS[:4])
        va = Arena([2 * 3 * oh * ow for (oh, ow) in sizes], 2)
        ctx.decode_batch_views(1, ins, lens, vi, va.ptrs, word, dtype, sizes, scale[:3], bias[:3], rects=rects, flips=flips)
        assert ctx.decode_status() == 0
        va_first = [g.copy() for g in va.fetch()]
        ws = ctx.workspace_bytes()
        got = run_views(ctx, 1, d_b, lens, VIEWS[:4], word, dtype, scale, bias, colours=COLS[:4])
        assert ctx.workspace_bytes() - ws == 48 * 4
        run_views(ctx, 1, d_b, lens, VIEWS[:4], word, dtype, scale, bias, colours=COLS[3:7])
        run_views(ctx, 1, d_b, lens, VIEWS[4:], word, dtype, scale, bias, colours=[DENSE, None, PERM])
        assert ctx.workspace_bytes() - ws == 48 * 4
        run_views(ctx, 1, d_b, lens, VIEWS[:3], word, dtype, scale, bias, plain=True)
        assert ctx.workspace_bytes() - ws == 48 * 4
        got7 = run_views(ctx, 1, d_b, lens, VIEWS, word, dtype, scale, bias, colours=COLS)
        assert ctx.workspace_bytes() - ws == 48 * 7 + 64 * 3
        for v, view in enumerate(VIEWS):
            assert np.array_equal(got7[v], host_rule(rasters[view[0]], view, COLS[v], word, dtype, scale, bias, AA, 3)), v
        for v in range(4):
            assert np.array_equal(got[v], got7[v])
        # the earlier calls with the pointers they had: the cached per-image table and the views' records were not disturbed
        va.refill(), rs.refill()
        ctx.decode_batch_views(1, ins, lens, vi, va.ptrs, word, dtype, sizes, scale[:3], bias[:3], rects=rects, flips=flips)
        ctx.decode_batch_resampled(1, ins, lens, rs.ptrs, word, dtype, (29, 37), scale[:3], bias[:3], rects=rrects, filter=AA)
        assert ctx.decode_status() == 0 and ctx.workspace_bytes() - ws == 48 * 7 + 64 * 3
        assert all(np.array_equal(a, b) for a, b in zip(va.fetch(), va_first)) and all(np.array_equal(a, b) for a, b in zip(rs.fetch(), rs_first))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_misuse_of_the_colour_call(gpu, batches):
    """Every refusal names its value, comes before anything reaches the device and leaves every byte of the arena as it was; what
    the views call refuses is refused with the same text."""
    rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, channels=3)
    vi, rects, flips, sizes = view_args(VIEWS)
    scale, bias = mixed_consts(F16)
    ctx = gpu.MixedContext(DIMS, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * oh * ow for (oh, ow) in sizes], 4)
        ws = ctx.workspace_bytes()

        def refused(words, same_as_plain=True, **kw):
            a = dict(mode=1, d_blobs=ins, lens=lens, view_image=vi, d_outs=outs.ptrs, layout=word, dtype=F16, sizes=sizes, scale=scale[:3], bias=bias[:3],
                     rects=rects, flips=flips, filter=AA, colours=COLS)
            a.update(kw)
            with pytest.raises(gpu.XpngError) as e:
                ctx.decode_batch_views(**a)
            assert all(w in str(e.value) for w in words), (words, str(e.value))
            assert outs.untouched(), words
            if same_as_plain:                                           # the views call's own text, word for word behind the symbol's name
                a.pop("colours")
                with pytest.raises(gpu.XpngError) as p:
                    ctx.decode_batch_views(**a)
                assert str(p.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]

        def with_entry(v, e, x):
            cols = [list(IDENT) if m is None else list(m) for m in COLS]
            cols[v][e] = x
            return cols

        refused(["view 4", "[1][2]", "nan"], same_as_plain=False, colours=with_entry(4, 6, float("nan")))
        refused(["view 0", "[0][3]", "inf"], same_as_plain=False, colours=with_entry(0, 3, float("inf")))
        refused(["view 6", "[2][0]", "65537"], same_as_plain=False, colours=with_entry(6, 8, 65537.0))
        refused(["view 1", "[0][0]", "-1e+30"], same_as_plain=False, colours=with_entry(1, 0, -1e30))
        refused(["colours has 3 entries", "7 views"], same_as_plain=False, colours=COLS[:3])
        refused(["colours[2]", "colour matrix"], same_as_plain=False, colours=COLS[:2] + [[1.0] * 5] + COLS[3:])
        refused(["view_image[2]", "is 5", "5 images"], view_image=vi[:2] + [5] + vi[3:])
        refused(["{500, 500, 300, 400}", "view 0", "image 0", "889 x 889"], rects=[(500, 500, 300, 400)] + rects[1:])
        refused(["224 x 0", "view 0"], sizes=[(0, 224)] + sizes[1:])
        refused(["flip 2", "view 1"], flips=[0, 2, 0, 0, 1, 0, 1])
        refused(["filter 2", "XPNGHIP_FILTER_TRIANGLE_AA"], filter=2)
        refused(["out_sizes is NULL"], sizes=None)
        refused(["null", "view 1"], d_outs=[outs.ptrs[0], 0] + outs.ptrs[2:])
        odd = [outs.ptrs[0], outs.ptrs[1] + 1] + outs.ptrs[2:]
        refused(["aligned", "%x" % odd[1], "view 1"], d_outs=odd)
        refused(["dtype 4"], dtype=4)
        refused(["layout", "0x500"], layout=0x500)
        refused(["scale[1]", "nan"], scale=[1.0, float("nan"), 1.0])
        refused(["mode 2", "RGB"], mode=2)
        refused(["null blob", "image 1"], d_blobs=[ins[0], 0] + ins[2:])
        assert ctx.workspace_bytes() == ws                              # nothing was allocated for a refused call
        # the context still works after all that
        got = run_views(ctx, 1, d_b, lens, VIEWS, word, F16, scale, bias, colours=COLS)
        for v, view in enumerate(VIEWS):
            assert np.array_equal(got[v], host_rule(rasters[view[0]], view, COLS[v], word, F16, scale, bias, AA, 4)), v
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_views_colour_on_goldens(gpu):
    """Two views per reference-written file with random_colour_jitter matrices, written through out= into slices of two stacked
    tensors of different sizes: every view equals api.resample_colour_host of api.load of its file."""
    import torch
    from xpng_amd import tensors
    paths = sorted(p for p in glob.glob(os.path.join(GOLD, "imgfull_*.xpng")) if 11 < os.path.getsize(p) < 200000)[:6]
    assert len(paths) == 6
    want = [gpu.load(p) for p in paths]
    dims = [(r.shape[1], r.shape[0]) for r in want]
    g = torch.Generator().manual_seed(21)
    used = [0, 1, 2, 3, 5]                                          # file 4 has no view
    big_r = tensors.random_resized_crops([dims[i] for i in used], generator=g)
    small_r = tensors.random_resized_crops([dims[i] for i in used], scale=(0.05, 0.14), generator=g)
    views = [(i, r, k % 2 == 1) for k, (i, r) in enumerate(zip(used, big_r))] + [(i, r, k % 2 == 0) for k, (i, r) in enumerate(zip(used, small_r))]
    cols = tensors.random_colour_jitter(len(views), p=0.9, gray_p=0.3, generator=g)
    cols[3] = None
    assert sum(not np.array_equal(m, np.asarray(IDENT, np.float32).reshape(3, 4)) for m in cols if m is not None) >= 5
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    for lay, bgr, dtype in (("chw", False, F16), ("hwc", True, F32)):
        shp = lambda oh, ow: (3, oh, ow) if lay == "chw" else (oh, ow, 3)   # noqa: E731
        big = torch.zeros((5,) + shp(32, 48), dtype=_torch_dtype(dtype), device="cuda")
        small = torch.zeros((5,) + shp(12, 12), dtype=_torch_dtype(dtype), device="cuda")
        outs = list(big.unbind(0)) + list(small.unbind(0))
        back = tensors.load_views(paths, views, [(32, 48)] * 5 + [(12, 12)] * 5, layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype),
                                  mean=IMAGENET_MEAN, std=IMAGENET_STD, out=outs, colour=cols)
        assert all(b is o for b, o in zip(back, outs))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for v, (i, rect, flip) in enumerate(views):
            oh, ow = (32, 48) if v < 5 else (12, 12)
            raw = api.resample_colour_host(want[i], (oh, ow), word, dtype, scale, bias, rect=rect, flip=flip, colour=IDENT if cols[v] is None else cols[v])
            t = (big if v < 5 else small)[v % 5]
            assert np.array_equal(_bits(t, dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (lay, v, paths[i], rect)
