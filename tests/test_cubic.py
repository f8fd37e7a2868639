"""Antialiased bicubic resampling in the copy-out of a views decode (include/xpng_hip.h xpnghip_resample_cubic_host,
xpnghip_decode_varsize_device_batch_views_cubic; xpng_amd/tensors.py load_views / load_files(interpolation="bicubic")).

Every comparison with the library is on the bits unless a test says otherwise.  CPU: the symbols; xpnghip_resample_cubic_host
against the checker of tests/_cubic.py for every layout word and dtype, with and without a matrix; consequences (a), (b) and (d); the
clamp; the mixed ratios; the rule against torch's CPU antialiased bicubic; the refusals; load_views and load_files on the
host-answered kinds.  GPU (-m gpu): the bits of every view against api.resample_cubic_host in sentinel arenas, the count of decoded
tiles, stale staging, NULL arguments, changing rectangles, the workspace, a rejected tile, misuse, load_views on goldens."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _cubic
from _cubic import Cubic
from _kit import (BF16, BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _offsets, _torch_dtype, _upload, built,
                  consts_from, declared, expect, exported, gpu, mixed_consts, po, table)
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_resample_cubic_host", "xpnghip_decode_varsize_device_batch_views_cubic"]
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
AA = api.FILTER_TRIANGLE_AA

IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
PERM = [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0]                       # R <- B, G <- R, B <- G: not symmetric, so a transposed index shows
GRAY = [0.299, 0.587, 0.114, 0] * 3
RANGE = [3, -2, 0.5, -300, -2, 3, 0, 300, 1, 1, -2, 40]            # leaves 0 .. 255 on both sides
DENSE = [0.70710678, -0.31830989, 0.57721566, 12.345678, 0.14142135, 1.6180339, -0.69314718, -7.3890561, -0.43429448, 0.26179939, 1.2020569,
         31.415926]
MATS = [IDENT, PERM, GRAY, RANGE, DENSE]


def _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, colour=None):
    ch = (word >> 8) or r.shape[2]
    raw = api.resample_cubic_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, colour=colour)
    shape = (ch, OH, OW) if word & 1 else (OH, OW, ch)
    return np.frombuffer(raw, BITS[dtype]).reshape(shape)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_cubic_symbols_are_declared_listed_and_exported():
    assert set(NEW) <= set(declared("xpng_hip.h", "xpnghip_")) and set(NEW) <= set(api.HIP_SYMBOLS) and set(NEW) <= exported(api.HIP_SO)
    assert api.hip_lib().xpnghip_abi_version() == 2
    import xpng_amd
    assert "resample_cubic_host" in xpng_amd.__all__ and callable(xpng_amd.resample_cubic_host)
    assert callable(api.MixedContext.decode_batch_views_cubic)


HOST_RASTERS = [(1, 1), (2, 1), (1, 2), (3, 3), (17, 4), (45, 31), (130, 9)]   # tests/test_resample.py's
HOST_SIZES = [(1, 1), (3, 5), (8, 8), (37, 29)]                   # (OW, OH)


def _host_rects(w, h, OW, OH):
    rects = [None, (w - 1, h - 1, 1, 1), (w - 1, 0, 1, h)]       # whole, 1 x 1 at the last pixel, the rightmost column
    if w >= OW and h >= OH:
        rects.append((w - OW, h - OH, OW, OH))                    # of the output's size
    if w >= 5 and h >= 5:
        rects.append((2, 2, w - 4, h - 4))                        # strictly inside: 2 px of other pixels on every side
    return rects


@pytest.mark.parametrize("px", [3, 4])
def test_resample_cubic_host_equals_the_checker(px):
    """Every layout word x dtype with four different (scale, bias) pairs, both flips, without a matrix and with one (the five
    matrices in turn; with a matrix three of the layout words in turn), on the bits.  A tap outside the rectangle would show on the
    rectangles strictly inside their raster (consequence c).  With it the mirror (b), the identity matrix against no matrix (d), the
    rectangle of the output's size against the slice of the float call's table (a), and the triangle filter where both axes shrink
    by more than 2x, which must differ."""
    rng = np.random.default_rng(300 + px)
    inside = crops = differs = n = 0
    least = np.inf
    for (w, h) in HOST_RASTERS:
        r = rng.integers(0, 256, (h, w, px), dtype=np.uint8)
        for (OW, OH) in HOST_SIZES:
            for rect in _host_rects(w, h, OW, OH):
                want = [Cubic(r, rect, flip, OH, OW) for flip in (False, True)]
                least = min(least, want[0].min_w, want[1].min_w)
                rw, rh = rect[2:] if rect else (w, h)
                rx, ry = rect[:2] if rect else (0, 0)
                inside += rect is not None and rect[:2] == (2, 2)
                for dtype in DTYPES:
                    scale, bias = mixed_consts(dtype)
                    for word in WORDS:
                        ch = (word >> 8) or px
                        got = [_lib(r, rect, flip, OW, OH, word, dtype, scale, bias) for flip in (False, True)]
                        for flip in (0, 1):
                            exp = want[flip].bits(word, dtype, scale, bias)
                            assert got[flip].shape == exp.shape and np.array_equal(got[flip], exp), \
                                (px, (w, h), (OW, OH), rect, flip, dtype, hex(word), np.argwhere(got[flip] != exp)[:4])
                        ax = 2 if word & 1 else 1
                        assert np.array_equal(got[1], np.flip(got[0], axis=ax)), ("mirror", (w, h), (OW, OH), rect, dtype, hex(word))
                        assert np.array_equal(got[0], _lib(r, rect, False, OW, OH, word, dtype, scale, bias, colour=IDENT)), ("identity", (w, h), rect)
                        if (rw, rh) == (OW, OH):                   # (a): a pure crop, the float call's table at the crop's bytes
                            tab = table(dtype, scale[:ch], bias[:ch])
                            crop = expect(r[ry:ry + rh, rx:rx + rw], bool(word & 1), bool(word & 2), ch, tab)
                            assert np.array_equal(got[0], crop), ("crop", (w, h), (OW, OH), rect, dtype, hex(word))
                            crops += 1
                        if rw > 2 * OW and rh > 2 * OH and w > 3:
                            tri = api.resample_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, filter=AA)
                            assert tri != got[0].tobytes()
                            differs += 1
                # with a matrix: the resampling is the one above, only the colour step is redone
                for flip in (0, 1):
                    n += 1
                    m = MATS[n % 5]
                    z = want[flip].recolour(m)
                    for dtype in DTYPES:
                        scale, bias = mixed_consts(dtype)
                        for word in (WORDS[n % 12], WORDS[(n + 5) % 12], WORDS[(n + 7) % 12]):
                            got = _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, colour=m)
                            assert np.array_equal(got, z.bits(word, dtype, scale, bias)), ("matrix", n % 5, px, (w, h), (OW, OH), rect, flip, dtype, hex(word))
    print("smallest W", least)
    assert inside >= 8 and crops >= 36 * 5 and differs >= 36 and 0 < least
    # the matrix as a (3, 4) array and as 12 numbers are the same call
    r = rng.integers(0, 256, (9, 11, px), dtype=np.uint8)
    assert api.resample_cubic_host(r, (5, 7), api.layout(), F32, colour=np.asarray(DENSE).reshape(3, 4)) == api.resample_cubic_host(r, (5, 7), api.layout(), F32, colour=DENSE)


def test_the_clamp_is_exercised():
    """5 x 5 random bytes to 37 x 29: the cubic overshoots on both sides, the rule clamps there, and the library gives the checker's
    bits - with scale 1 and bias 0 in f32 the elements are v itself."""
    r = np.random.default_rng(5).integers(0, 256, (5, 5, 4), dtype=np.uint8)
    z = Cubic(r, None, False, 29, 37)
    print("unclamped range", float(z.raw.min()), float(z.raw.max()))
    assert z.raw.min() < 0 and z.raw.max() > 255 and z.v.min() == 0 and z.v.max() == 255
    got = _lib(r, None, False, 37, 29, api.layout(), F32, [1.0] * 4, [0.0] * 4).view(np.float32)
    assert np.array_equal(got, z.v) and int((z.raw != z.v).sum()) > 20
    for m in (RANGE, DENSE):                                        # the matrix takes the CLAMPED values
        for dtype in DTYPES:
            scale, bias = mixed_consts(dtype)
            for word in WORDS:
                assert np.array_equal(_lib(r, None, True, 37, 29, word, dtype, scale, bias, colour=m), Cubic(r, None, True, 29, 37, m).bits(word, dtype, scale, bias))


def test_mixed_ratios():
    """A 9 x 200 rectangle to 37 x 29: x grows (s = 1), y shrinks (the stretched window); and its transpose."""
    rng = np.random.default_rng(9)
    for (w, h, rect, OW, OH) in [(13, 204, (2, 2, 9, 200), 37, 29), (204, 13, (2, 2, 200, 9), 29, 37)]:
        r = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for flip in (False, True):
            z = Cubic(r, rect, flip, OH, OW)
            xa, xb, ya, yb = z.span
            assert xa.min() == 0 and ya.min() == 0 and xb.max() == rect[2] - 1 and yb.max() == rect[3] - 1
            for m in (None, DENSE):
                z.recolour(m)
                for dtype in DTYPES:
                    scale, bias = mixed_consts(dtype)
                    for word in WORDS:
                        got = _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, colour=m)
                        assert np.array_equal(got, z.bits(word, dtype, scale, bias)), ((w, h), flip, m is None, dtype, hex(word))


TORCH_SHAPES = [(7, 9, 3, 5), (17, 33, 4, 7), (64, 64, 5, 5), (100, 37, 37, 29), (445, 300, 3, 5), (33, 65, 32, 64), (50, 50, 50, 20),
                (20, 50, 40, 7), (2, 1000, 1, 3), (129, 131, 7, 128),                         # tests/test_resample.py's ten
                (5, 5, 37, 29), (1, 1, 4, 7), (3, 2, 8, 8), (16, 16, 16, 16)]                 # (h, w, OH, OW)
TORCH_BOUND = 2.0 ** -9


def test_rule_against_torch_bicubic_antialias():
    """The checker (its clamped v) against torch's CPU F.interpolate(bicubic, align_corners=False, antialias=True) of the cropped
    fp32 raster, clamped to 0 .. 255.  torch normalises the weights of a window first and sums weighted taps, the rule divides the
    weighted sum by the sum of the weights at the end, so the two differ in the last bits: with this checker the largest
    difference over these shapes was 2.14e-4 in byte units (2^-13 * 1.75, on 2 x 1000 -> 1 x 3: up to 1334 taps in a row; 1.75e-4
    on 445 x 300 -> 3 x 5, at most 1.07e-4 on the others).  The bound is 2^-9: 8x that (1.71e-3), rounded up to a power of two, for another vector path of another torch build (the margin of
    tests/test_resample.py's test_rule_against_torch_interpolate_antialias); a wrong window, kernel constant or half-pixel
    convention is off by whole grey levels on random bytes."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(7)
    worst = 0.0
    for (h, w, OH, OW) in TORCH_SHAPES:
        r = rng.integers(0, 256, (h + 3, w + 2, 3), dtype=np.uint8)
        rect = (2, 1, w, h)
        v = Cubic(r, rect, False, OH, OW).v
        crop = torch.from_numpy(r[1:1 + h, 2:2 + w].astype(np.float32)).permute(2, 0, 1)[None]
        t = F.interpolate(crop, size=(OH, OW), mode="bicubic", align_corners=False, antialias=True).clamp(0.0, 255.0)[0].permute(1, 2, 0).numpy()
        d = float(np.abs(t.astype(np.float64) - v.astype(np.float64)).max())
        print("cubic rule vs torch", (h, w, OH, OW), d)
        worst = max(worst, d)
        assert d <= TORCH_BOUND, ((h, w, OH, OW), d)
    print("cubic rule vs torch, worst", worst)


def test_resample_cubic_host_refusals():
    lib = api.hip_lib()
    r = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out = np.full(4 * 4 * 4 * 4 + 4, 0x5A5A5A5A, np.uint32)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    u64 = C.c_uint64

    def call(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, colour=None, o=None):
        ra = None if rect is None else (u64 * 4)(*rect)
        cm = None if colour is None else (C.c_float * 12)(*colour)
        return lib.xpnghip_resample_cubic_host(pxsz, raster, w, h, ra, flip, ow, oh, layout, dtype, scale, bias, cm, out.ctypes.data if o is None else o)

    def refused(words, **kw):
        """with and without a matrix; the text is xpnghip_resample_colour_host's, but for the function's name"""
        for colour in (None, DENSE):
            assert call(colour=colour, **kw) != 0, kw
            msg = api._err()
            assert all(w in msg for w in words), (words, msg)
            a = dict(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, o=out.ctypes.data)
            a.update(kw)
            ra = None if a["rect"] is None else (u64 * 4)(*a["rect"])
            assert lib.xpnghip_resample_colour_host(a["pxsz"], a["raster"], a["w"], a["h"], ra, a["flip"], a["ow"], a["oh"], a["layout"], a["dtype"],
                                                    a["scale"], a["bias"], AA, (C.c_float * 12)(*DENSE), a["o"]) != 0
            assert api._err().replace("resample_colour_host", "resample_cubic_host") == msg

    assert call() == 0 and call(colour=DENSE) == 0
    out[:] = 0x5A5A5A5A
    refused(["{0, 0, 0, 3}", "7 x 5"], rect=(0, 0, 0, 3))           # zero size
    refused(["{2, 0, 6, 1}", "7 x 5"], rect=(2, 0, 6, 1))           # x + w > W
    refused(["{0, 5, 1, 1}"], rect=(0, 5, 1, 1))
    refused(["4 x 0", "16384"], oh=0)
    refused(["0 x 4"], ow=0)
    refused(["16385 x 4"], ow=16385)
    refused(["4 x 16385"], oh=16385)
    refused(["flip 2"], flip=2)
    refused(["dtype 0"], dtype=0)
    refused(["dtype 4"], dtype=4)
    refused(["layout", "0x4"], layout=0x004)
    refused(["layout", "0x500"], layout=0x500)
    refused(["scale[1]", "nan"], scale=(C.c_float * 4)(1, float("nan"), 1, 1))
    refused(["bias[2]", "inf"], bias=(C.c_float * 4)(0, 0, float("inf"), 0))
    refused(["null"], raster=None)
    refused(["null"], o=0)
    refused(["aligned", "%x" % (out.ctypes.data + 2)], o=out.ctypes.data + 2)          # f32 at 2 mod 4
    refused(["aligned"], o=out.ctypes.data + 1, dtype=F16)
    refused(["pxsz is 5"], pxsz=5)
    refused(["0 x 5"], w=0)
    for e, bad, word in ((5, float("nan"), "nan"), (11, float("inf"), "inf"), (6, 65537.0, "65537")):
        m = list(DENSE)
        m[e] = bad
        assert call(colour=m) != 0
        msg = api._err()
        assert "[%d][%d]" % (e // 4, e % 4) in msg and word in msg and "colour" in msg, msg
        with pytest.raises(api.XpngError) as ex:
            api.resample_cubic_host(r, (4, 4), api.layout(), F32, colour=m)
        assert "[%d][%d]" % (e // 4, e % 4) in str(ex.value)
    assert (out == 0x5A5A5A5A).all()                                # a refused call writes nothing
    assert call(o=out.ctypes.data + 2, dtype=BF16) == 0             # (2 mod 4 is fine for a 2-byte element)
    with pytest.raises(api.XpngError) as e:
        api.resample_cubic_host(r, (4, 4), 0, F32, rect=(0, 0, 8, 1))
    assert "{0, 0, 8, 1}" in str(e.value)
    for bad in ([1.0] * 11, np.zeros((4, 3)), "gray"):
        with pytest.raises(api.XpngError) as ex:
            api.resample_cubic_host(r, (4, 4), api.layout(), F32, colour=bad)
        assert "colour matrix" in str(ex.value)
    # the device entry point refuses a NULL context like its siblings
    p1, n1 = (C.c_void_p * 1)(0), (u64 * 1)(0)
    assert lib.xpnghip_decode_varsize_device_batch_views_cubic(None, 1, p1, n1, 1, None, 1, None, p1, (C.c_uint32 * 2)(4, 4), None, None, 0, F16, None, None,
                                                               None, None) != 0
    assert "null context" in api._err()
    # the entry points with a filter word keep their domain
    with pytest.raises(api.XpngError) as e:
        api.resample_host(r, (4, 4), 0, F32, filter=2)
    assert "filter 2" in str(e.value) and "XPNGHIP_FILTER_TRIANGLE_AA" in str(e.value)


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


def test_load_views_and_load_files_bicubic_answer_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(37, 25, 3), (1000, 1000, 3), (16, 39, 4)]
    views = [(0, (1, 2, 23, 34), True), (2, None, False), (0, None, False), (1, (100, 200, 300, 150), False), (2, (3, 1, 35, 5), True),
             (0, (23, 35, 1, 1), False)]
    sizes = [(6, 5), (3, 7), (40, 30), (2, 2), (9, 4), (1, 1)]     # (OH, OW): per-view sizes
    cols = [PERM, None, RANGE, None, np.asarray(DENSE).reshape(3, 4), GRAY]
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    for dtype in DTYPES:
        for ch, lay, bgr in ((3, "chw", False), (4, "hwc", True)):
            scale, bias = consts_from(mean[:ch], std[:ch])
            word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
            kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch])
            got = tensors.load_views(paths, views, sizes, colour=cols, interpolation="bicubic", **kw)
            plain = tensors.load_views(paths, views, sizes, interpolation="bicubic", **kw)
            tri = tensors.load_views(paths, views, sizes, **kw)
            for v, ((i, rect, flip), (oh, ow)) in enumerate(zip(views, sizes)):
                for g, m in ((got[v], cols[v]), (plain[v], None)):
                    exp = Cubic(want[i], rect, flip, oh, ow, m).bits(word, dtype, scale, bias)
                    assert g.device.type == "cpu" and g.is_contiguous() and g.dtype == _torch_dtype(dtype) and tuple(g.shape) == exp.shape
                    assert np.array_equal(_bits(g, dtype), exp), (dtype, ch, lay, v, m is None)
            assert not torch.equal(plain[0], tri[0]) and not torch.equal(plain[2], tri[2])     # the default is still the triangle
            whole = tensors.load_views(paths, views, (6, 5), stack=True, colour=cols, interpolation="bicubic", **kw)
            for v, (i, rect, flip) in enumerate(views):
                raw = api.resample_cubic_host(want[i], (6, 5), word, dtype, scale, bias, rect=rect, flip=flip, colour=cols[v])
                assert np.array_equal(_bits(whole[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), ("stack", v)
            # load_files: one view per file
            crops, flips = [(1, 2, 23, 34), (100, 200, 300, 150), (2, 0, 37, 5)], [True, False, True]
            fkw = dict(size=(6, 5), crops=crops, flips=flips, antialias=True, **kw)
            files = tensors.load_files(paths, interpolation="bicubic", **fkw)
            stacked = tensors.load_files(paths, interpolation="bicubic", stack=True, **fkw)
            old = tensors.load_files(paths, **fkw)
            for i, g in enumerate(files):
                exp = Cubic(want[i], crops[i], flips[i], 6, 5).bits(word, dtype, scale, bias)
                assert np.array_equal(_bits(g, dtype), exp) and np.array_equal(_bits(stacked[i], dtype), exp), ("files", dtype, ch, lay, i)
            assert not torch.equal(files[0], old[0])
    # misuse: bicubic needs antialias=True, and a size; other words are refused
    o1 = [torch.zeros((3, 4, 4), dtype=torch.float16)]
    with pytest.raises(api.XpngError) as e:
        tensors.load_views(paths, [(0, None, False)], (4, 4), out=o1, device="cpu", interpolation="bicubic", antialias=False)
    assert "antialias=True" in str(e.value) and "bicubic" in str(e.value)
    with pytest.raises(api.XpngError) as e:
        tensors.load_views(paths, [(0, None, False)], (4, 4), out=o1, device="cpu", interpolation="lanczos")
    assert "lanczos" in str(e.value)
    assert float(o1[0].abs().sum()) == 0.0
    for bad, word in ((dict(size=(4, 4)), "antialias=True"), (dict(antialias=True), "size"), (dict(), "antialias=True")):
        with pytest.raises(api.XpngError) as e:
            tensors.load_files(paths, device="cpu", dtype=torch.float16, interpolation="bicubic", **bad)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, device="cpu", dtype=torch.float16, size=(4, 4), antialias=True, interpolation="nearest")


# ---- GPU ----------------------------------------------------------------------------------------------------------------
GPU_SIZES = [(3, 5), (37, 29)]                                    # (OW, OH): rows narrower than one 16-byte store; an odd width
# tests/test_resample.py's batches: the 889-wide image has a tile boundary inside the rectangles across x = 444
RGB_DIMS = [(3, 3), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100)]
RGBA_DIMS = [(4, 4), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100)]


def _views(dims, p):
    """(image, rectangle, flip, (OW, OH)) of pass p: the edge rectangles, a rectangle of each output size, one strictly inside, the
    mixed 9 x 200 and the 80 x 300 across the tile boundary (they overlap), the strong downscale 90 x 1000 beside a rectangle
    inside it.  More views than images; several of one image overlap; image 3 (pass 0) or image 0 (pass 1) has none.  The two output
    sizes alternate over the views and swap between the passes."""
    w0, h0 = dims[0]
    views = [(0, (0, 0, w0, h0)), (0, (w0 - 1, h0 - 1, 1, 1)), (1, (16, 3, 1, 1)), (1, (16, 0, 1, 4)), (1, (0, 0, 17, 4)),
             (2, (0, 0, 64, 64)), (2, (0, 63, 64, 1)), (2, (2, 2, 60, 60)), (2, (10, 20, 37, 29)), (2, (27, 35, 37, 29)), (2, (61, 59, 3, 5)), (2, (1, 7, 3, 5)),
             (3, (10, 20, 2, 3)), (3, (200, 140, 245, 304)),
             (4, (440, 100, 9, 200)), (4, (400, 50, 80, 300)), (5, (3, 50, 90, 1000)), (5, (20, 30, 60, 500))]
    views = [v for v in views if v[0] != (3, 0)[p]]
    return [(i, rect, (k // 2) % 2, GPU_SIZES[(k + p) % 2]) for k, (i, rect) in enumerate(views)]


def view_args(views):
    return [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [(v[3][1], v[3][0]) for v in views]   # sizes as (OH, OW)


@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): the dims, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "noise"]
    out = {}
    for mode, alpha in FORMATS:
        dims = RGBA_DIMS if alpha else RGB_DIMS
        rasters = [synth_raster(kinds[(i + 1) % 4], w, h, alpha, seed=i + 31) for i, (w, h) in enumerate(dims)]
        out[(mode, alpha)] = (dims, rasters, [po.encode_tiles(mode, r) for r in rasters])
    return out


def run_cubic(ctx, mode, d_b, lens, views, word, dtype, scale, bias, colours=None, offs=None, expect_status=0, arena=None):
    """the views' elements as bit patterns, flat, out of a sentinel-filled arena whose every other byte is checked.  Buffer i starts
    i % 8 elements into its 16-byte aligned region: every start of a row modulo 16 bytes."""
    ch = api.layout_channels(word, ctx.pxsz)
    vi, rects, flips, sizes = view_args(views)
    ar = arena or Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
    ctx.decode_batch_views_cubic(mode, [t.data_ptr() for t in d_b], lens, vi, ar.ptrs, word, dtype, sizes, scale[:ch], bias[:ch], rects=rects, flips=flips,
                                 colours=colours, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return [g.view(BITS[dtype]) for g in ar.fetch()]


def host_rule(raster, view, col, word, dtype, scale, bias):
    i, rect, flip, (OW, OH) = view
    ch = api.layout_channels(word, raster.shape[2])
    return np.frombuffer(api.resample_cubic_host(raster, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=bool(flip), colour=col), BITS[dtype])


@pytest.mark.gpu
def test_one_cubic_view_in_one_tile_of_a_two_tile_image(gpu, po):
    """The smallest case: the lower tile of a 200 x 2000 image alone."""
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
        for col in (None, PERM):
            got = run_cubic(ctx, 1, d_b, [len(blob)], views, word, F16, scale, bias, colours=col and [col])
            assert ctx.last_decode_tiles() == 1
            assert np.array_equal(got[0], host_rule(r, views[0], col, word, F16, scale, bias))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_cubic_bits(gpu, batches, mode, alpha, dtype):
    """Every element of every view equals api.resample_cubic_host and every sentinel is intact, for all 12 layout words, both
    passes of the view list (each view at both output sizes) - one without matrices, the other with one per view (None beside a matrix: the
    identity, which gives the bits of no matrix); the launch held exactly the tiles of api.view_tiles."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for wi, word in enumerate(WORDS):
            for p, with_cols in ((wi % 2, False), ((wi + 1) % 2, True)):   # every word: one pass without matrices, the other with them
                views = _views(dims, p)
                vi, rects, _, _ = view_args(views)
                assert len(views) > len(dims) and (3, 0)[p] not in vi
                sel = api.view_tiles(dims, vi, rects)
                colours = [(MATS + [None])[(v + wi) % 6] for v in range(len(views))] if with_cols else None
                got = run_cubic(ctx, mode, d_b, lens, views, word, dtype, scale, bias, colours=colours)
                assert ctx.last_decode_tiles() == len(sel) < ctx.n_tiles
                for v, view in enumerate(views):
                    w = host_rule(rasters[view[0]], view, colours and colours[v], word, dtype, scale, bias)
                    assert np.array_equal(got[v], w), (hex(word), dtype, p, v, view, with_cols, np.argwhere(got[v] != w)[:4].ravel())
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cubic_stale_staging_is_never_read(gpu, po):
    """decode_batch_as_float on batch A, then a cubic views call on batch B = 255 - A whose rectangles end and start exactly on tile
    boundaries - the tiles beside them still hold A's pixels in the staging raster, and the cubic window is the widest the project
    has - then decode_batch_as_float on A again with the pointers it had."""
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
        got = run_cubic(ctx, 1, db, [len(b) for b in bb], views, word, dtype, scale, bias, colours=[None, DENSE, None, GRAY])
        assert ctx.last_decode_tiles() == 4                        # tiles 0, 2 and 3 of image 0 and the one of image 1
        for v, view in enumerate(views):
            assert np.array_equal(got[v], host_rule(B[view[0]], view, [IDENT, DENSE, IDENT, GRAY][v], word, dtype, scale, bias)), v
        full.refill()
        ctx.decode_batch_as_float(1, ins, [len(b) for b in ba], full.ptrs, word, dtype, scale[:3], bias[:3])
        assert ctx.decode_status() == 0 and ctx.last_decode_tiles() == ctx.n_tiles
        for g, f in zip(full.fetch(), first):
            assert np.array_equal(g.view(np.uint16), f)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cubic_null_arguments_changing_rectangles_and_the_workspace(gpu, po):
    """One pointer array, four calls: rectangles, then NULL view_image, rects and flips (every whole image, no flip), then the first
    again with the host's size walk, then other rectangles.  The workspace grows by the views call's amounts - 64 bytes per view
    and 4 per tile - and by nothing more while colours is NULL; the first call with matrices adds 48 bytes per view."""
    from xpng_amd.synth import synth_raster
    dims = [(17, 4), (64, 64), (130, 90), (100, 110), (5, 7)]
    rasters = [synth_raster(["photo", "noise", "gray"][i % 3], w, h, False, seed=i + 40) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    r1 = [(0, 0, 17, 4), (3, 4, 50, 55), (10, 10, 110, 70), (0, 0, 100, 110), (1, 2, 3, 4)]
    r2 = [(1, 1, 15, 2), (0, 0, 64, 64), (100, 0, 30, 90), (40, 50, 60, 60), (0, 0, 5, 7)]
    flips = [1, 0, 1, 0, 1]
    OW, OH = 21, 13
    dtype, word = F16, api.layout(planar=True, bgr=True, channels=4)
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(dims, 3)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        full = Arena([2 * 4 * w * h for (w, h) in dims], 2)
        ctx.decode_batch_as_float(1, ins, lens, full.ptrs, word, dtype, scale, bias)
        assert ctx.decode_status() == 0
        ws = ctx.workspace_bytes()
        ar = Arena([2 * 4 * OW * OH] * len(dims), 2)
        ident = list(range(len(dims)))

        def call(vi, rects, fl, offs=None, colours=None):
            ar.refill()
            ctx.decode_batch_views_cubic(1, ins, lens, vi, ar.ptrs, word, dtype, (OH, OW), scale, bias, rects=rects, flips=fl, tile_offs=offs, colours=colours)
            assert ctx.decode_status() == 0
            return [g.view(np.uint16).copy() for g in ar.fetch()]

        a = call(ident, r1, flips)
        grown = 64 * len(dims) + 4 * ctx.n_tiles
        assert ctx.workspace_bytes() - ws == grown                  # the views call's tables, and no matrix table
        b = call(None, None, None)
        c = call(ident, r1, flips, offs=_offsets(blobs, ctx))
        d = call(None, r2, flips)
        assert ctx.workspace_bytes() - ws == grown
        e = call(ident, r2, flips, colours=[DENSE] * len(dims))
        assert ctx.workspace_bytes() - ws == grown + 48 * len(dims)
        for i, r in enumerate(rasters):
            def rule(rect, flip, col=None):
                return host_rule(r, (i, rect, flip, (OW, OH)), col, word, dtype, scale, bias)
            assert np.array_equal(a[i], rule(r1[i], flips[i])) and np.array_equal(b[i], rule(None, 0)) and np.array_equal(c[i], a[i]), i
            assert np.array_equal(d[i], rule(r2[i], flips[i])) and np.array_equal(e[i], rule(r2[i], flips[i], DENSE)), i
        assert any(not np.array_equal(x, y) for x, y in zip(a, b)) and any(not np.array_equal(x, y) for x, y in zip(a, d))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cubic_rejected_tile_and_misuse(gpu, batches):
    """The second tile of the 889-wide image gets type byte 0x7F: the call reports 1, every element of the view across the boundary
    with no tap inside that tile is exact, and so is every other view.  Then the misuse list of the views call without the filter
    line: every refusal names its value, has the views-colour call's text, and leaves every byte of the arena as it was."""
    dims, rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, channels=3)
    scale, bias = mixed_consts(F16)
    views = [v for v in _views(dims, 1)]
    ctx = gpu.MixedContext(dims, 4)
    try:
        k = 4
        offs = _offsets(blobs, ctx)
        tx, ty, tw, th = ctx.tile(ctx.first_tile[k] + 1)           # the image's second tile: the right half
        assert 440 <= tx < 480 < tx + tw and ty == 0
        bad = bytearray(blobs[k])
        bad[offs[k][1] + 3] = 0x7F                                 # top byte of the tile's first little-endian word
        bb = blobs[:k] + [bytes(bad)] + blobs[k + 1:]
        got = run_cubic(ctx, 1, _upload(bb), [len(b) for b in bb], views, word, F16, scale, bias, expect_status=1)
        clean = 0
        for v, view in enumerate(views):
            i, rect, flip, (OW, OH) = view
            w = host_rule(rasters[i], view, None, word, F16, scale, bias).reshape(3, OH, OW)
            g = got[v].reshape(w.shape)
            if i != k:
                assert np.array_equal(g, w), v
                continue
            xa, xb = _cubic.span(OW, rect[2], bool(flip))           # relative to the rectangle, inclusive
            ya, yb = _cubic.span(OH, rect[3], False)
            hitx = (rect[0] + xb >= tx) & (rect[0] + xa < tx + tw)
            hity = (rect[1] + yb >= ty) & (rect[1] + ya < ty + th)
            hit = hity[:, None] & hitx[None, :]
            assert hit.any()
            clean += int((~hit).sum())
            assert np.array_equal(g[:, ~hit], w[:, ~hit]), v
        assert clean > 100
        vi, rects, flips, sizes = view_args(views)
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * oh * ow for (oh, ow) in sizes], 4)
        ws = ctx.workspace_bytes()
        n = len(views)

        def refused(words, **kw):
            a = dict(mode=1, d_blobs=ins, lens=lens, view_image=vi, d_outs=outs.ptrs, layout=word, dtype=F16, sizes=sizes, scale=scale[:3], bias=bias[:3],
                     rects=rects, flips=flips)
            a.update(kw)
            for cols in (None, [DENSE] * n):
                with pytest.raises(gpu.XpngError) as e:
                    ctx.decode_batch_views_cubic(colours=cols, **a)
                assert all(w in str(e.value) for w in words), (words, str(e.value))
                assert outs.untouched(), words
            with pytest.raises(gpu.XpngError) as p:                    # the views call's own text, word for word behind the symbol's name
                ctx.decode_batch_views(filter=AA, **a)
            assert str(p.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]

        refused(["view_image[2]", "is 6", "6 images"], view_image=vi[:2] + [6] + vi[3:])
        refused(["view_image is NULL", "nviews is %d" % n, "nimg 6"], view_image=None)
        refused(["{0, 0, 18, 4}", "view 0", "image 1", "17 x 4"], rects=[(0, 0, 18, 4)] + rects[1:])
        refused(["{0, 0, 0, 5}", "view 3"], rects=rects[:3] + [(0, 0, 0, 5)] + rects[4:])
        refused(["37 x 0", "view 0"], sizes=[(0, 37)] + sizes[1:])
        refused(["16385 x 29", "view 5"], sizes=sizes[:5] + [(29, 16385)] + sizes[6:])
        refused(["flip 2", "view 1"], flips=[0, 2] + flips[2:])
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
        # the matrices' refusals name the view and the entry
        nan = [list(DENSE) for _ in range(n)]
        nan[4][6] = float("nan")
        with pytest.raises(gpu.XpngError) as e:
            ctx.decode_batch_views_cubic(1, ins, lens, vi, outs.ptrs, word, F16, sizes, scale[:3], bias[:3], rects=rects, flips=flips, colours=nan)
        assert all(w in str(e.value) for w in ("view 4", "[1][2]", "nan")) and outs.untouched()
        with pytest.raises(gpu.XpngError) as e:
            ctx.decode_batch_views_cubic(1, ins, lens, vi, outs.ptrs, word, F16, sizes, scale[:3], bias[:3], rects=rects, flips=flips, colours=[DENSE] * 3)
        assert "colours has 3 entries" in str(e.value)
        # nviews outside 1 .. 65535 and a context that is not mixed, through the raw entry point
        lib = api.hip_lib()
        p1, n1, s1 = (C.c_void_p * 1)(outs.ptrs[0]), (C.c_uint64 * 6)(*lens), (C.c_uint32 * 2)(4, 4)
        b6 = (C.c_void_p * 6)(*ins)
        z1 = (C.c_uint32 * 1)(0)
        assert lib.xpnghip_decode_varsize_device_batch_views_cubic(ctx._h, 1, b6, n1, 6, None, 0, z1, p1, s1, None, None, word, F16, None, None, None, None) != 0
        assert "nviews is 0" in api._err()
        assert lib.xpnghip_decode_varsize_device_batch_views_cubic(ctx._h, 1, b6, n1, 6, None, 65536, z1, p1, s1, None, None, word, F16, None, None, None, None) != 0
        assert "nviews is 65536" in api._err() and "65535" in api._err()
        one = gpu.Context(64, 64, 4)
        try:
            assert lib.xpnghip_decode_varsize_device_batch_views_cubic(one._h, 1, b6, n1, 1, None, 1, z1, p1, s1, None, None, word, F16, None, None, None, None) != 0
            assert "not a mixed context" in api._err()
        finally:
            one.close()
        assert outs.untouched() and ctx.workspace_bytes() == ws     # nothing was allocated for a refused call
        # the context still works after all that
        got = run_cubic(ctx, 1, d_b, lens, views, word, F16, scale, bias)
        for v, view in enumerate(views):
            assert np.array_equal(got[v], host_rule(rasters[view[0]], view, None, word, F16, scale, bias)), v
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_views_bicubic_on_goldens(gpu):
    """Two views per reference-written file with random_colour_jitter matrices, stacked: every view equals
    api.resample_cubic_host of api.load of its file.  And load_files(interpolation="bicubic") on the same files and crops."""
    import torch
    from xpng_amd import tensors
    paths = sorted(p for p in glob.glob(os.path.join(GOLD, "imgfull_*.xpng")) if 11 < os.path.getsize(p) < 200000)[:6]
    assert len(paths) == 6
    want = [gpu.load(p) for p in paths]
    dims = [(r.shape[1], r.shape[0]) for r in want]
    g = torch.Generator().manual_seed(22)
    used = [0, 1, 2, 3, 5]                                          # file 4 has no view
    big_r = tensors.random_resized_crops([dims[i] for i in used], generator=g)
    small_r = tensors.random_resized_crops([dims[i] for i in used], scale=(0.05, 0.14), generator=g)
    views = [(i, r, k % 2 == 1) for k, (i, r) in enumerate(zip(used, big_r))] + [(i, r, k % 2 == 0) for k, (i, r) in enumerate(zip(used, small_r))]
    cols = tensors.random_colour_jitter(len(views), p=0.9, gray_p=0.3, generator=g)
    cols[3] = None
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    for lay, bgr, dtype in (("chw", False, F16), ("hwc", True, F32)):
        kw = dict(layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype), mean=IMAGENET_MEAN, std=IMAGENET_STD)
        whole = tensors.load_views(paths, views, (32, 48), stack=True, colour=cols, interpolation="bicubic", **kw)
        assert whole.is_cuda and tuple(whole.shape) == (10,) + ((3, 32, 48) if lay == "chw" else (32, 48, 3))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for v, (i, rect, flip) in enumerate(views):
            raw = api.resample_cubic_host(want[i], (32, 48), word, dtype, scale, bias, rect=rect, flip=flip, colour=cols[v])
            assert np.array_equal(_bits(whole[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (lay, v, paths[i], rect)
        crops = [tuple(int(x) for x in r) for r in tensors.random_resized_crops(dims, generator=g)]
        files = tensors.load_files(paths, size=(12, 20), crops=crops, flips=[i % 2 == 0 for i in range(6)], antialias=True, interpolation="bicubic",
                                   stack=True, **kw)
        for i in range(6):
            raw = api.resample_cubic_host(want[i], (12, 20), word, dtype, scale, bias, rect=crops[i], flip=i % 2 == 0)
            assert np.array_equal(_bits(files[i], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), ("files", lay, i)
